// The scoring kernels of a beam-search step, ONE copy of their arithmetic for the entry points of csrc/decoder.hip
// (emoasr_beam_scores_topk, emoasr_ctc_prefix_init / _score and their ragged twins) and of csrc/decode_grid.hip (the fusion grid:
// one LM weight per row, several searches over one utterance's frames).
#pragma once
#include <math.h>
#include "common.h"

namespace {

#define EMO_DPP_I(old_, v_, ctrl_, rmask_) __builtin_amdgcn_update_dpp((old_), (v_), (ctrl_), (rmask_), 0xf, false)
// wave-wide max / min through DPP moves: quad swaps, half-row and row mirrors, the GFX9 row broadcasts; the result of lane 63
__device__ __forceinline__ float topk_wave_max(float v) {
#define EMO_STEP(ctrl_, rm_) v = fmaxf(v, __builtin_bit_cast(float, EMO_DPP_I(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), ctrl_, rm_)))
  EMO_STEP(0xB1, 0xf); EMO_STEP(0x4E, 0xf); EMO_STEP(0x141, 0xf); EMO_STEP(0x140, 0xf); EMO_STEP(0x142, 0xa); EMO_STEP(0x143, 0xc);
#undef EMO_STEP
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ int topk_wave_min(int v) {
#define EMO_STEP(ctrl_, rm_) v = min(v, EMO_DPP_I(v, v, ctrl_, rm_))
  EMO_STEP(0xB1, 0xf); EMO_STEP(0x4E, 0xf); EMO_STEP(0x141, 0xf); EMO_STEP(0x140, 0xf); EMO_STEP(0x142, 0xa); EMO_STEP(0x143, 0xc);
#undef EMO_STEP
  return __builtin_amdgcn_readlane(v, 63);
}

// log-softmax of the decoder row + mu * log-softmax of the LM row + top-k, one launch, one workgroup of 1024 threads per
// hypothesis (the beam search never needs the full score rows: three launches and ~130 us per step become one of ~20 us).
//   s[v] = (dec[v] - lse(dec)) + mu * (lm[v] - lse(lm));  vals / idx = the k largest s (ties -> lowest index);
//   lm_at = lm[idx] - lse(lm).   lm == NULL: no LM term.
// Selection: every thread keeps the best of its own strided elements; a round is one wave reduction + one barrier, then
// only the owner of the winner rescans its elements.  The body is csrc/beam_scores_topk_body.h.

// dynamic LDS of beam_scores_topk_body.h: the score row + the 16 waves' k survivors (value, index), and the LM row when it fits
// (*lm_lds); 0 when the plan does not fit
inline int beam_scores_topk_lds_bytes(int V, int k, bool has_lm, int* lm_lds) {
  int bytes = V * 4 + 16 * k * 8;
  if ((size_t)bytes > 150 * 1024) return 0;
  *lm_lds = has_lm && (size_t)bytes + (size_t)V * 4 <= 150 * 1024;
  if (*lm_lds) bytes += V * 4;
  return bytes;
}

#define EMO_LOG0 (-1e10f)
__device__ __forceinline__ float np_logaddexp(float a, float b) {
  // numpy.logaddexp semantics for finite inputs
  const float d = a - b;
  return d > 0.f ? a + log1pf(expf(-d)) : b + log1pf(expf(d));
}

// One wave per (beam m, candidate c).  x: CTC log-probs [T, V].
// r_prev: the parent's state [T,2]: prev_states + (parent[m]*cw_prev + pcand[m]) * T*2, or init_state
// when prev_states == NULL.  Outputs log_psi [nb, cw] and states [nb, cw, T, 2].
// The recursion over t is sequential (and kept in the reference's float32 operation order: ctc_score.py:47-76),
// but everything it consumes is not: per chunk of 64 frames the lanes fetch the parent state and the two
// emission columns (one memory round trip per chunk instead of four per frame) and compute phi; lane 0 then
// runs the 64 dependent steps out of LDS and the lanes write the new state rows back coalesced.
// RAGGED (the batched joint search): row m belongs to search m / W, whose emissions are the rows xoff[s] .. xoff[s + 1] - 1 of x;
// every state is a [Tn = Tmax, 2] slot of which the search uses its first T_s rows.  The fusion grid: search m / W runs over the
// frames of utterance sutt[m / W] -- several searches share one utterance's emissions.
// The body is csrc/ctc_prefix_body.h.

// initial state of Tn_ frames at x_, by one thread: r[t,1] = running sum of the blank log-probs (float32, step by step),
// r[t,0] = LOG_0
#define EMO_CTC_PREFIX_INIT_ROWS(Tn_, V_, x_, blank_, r_)                       \
  float acc = 0.f;                                                              \
  for (int t = 0; t < (Tn_); ++t) {                                             \
    acc = t == 0 ? (x_)[blank_] : acc + (x_)[(long)t * (V_) + (blank_)];        \
    (r_)[2 * t] = EMO_LOG0;                                                     \
    (r_)[2 * t + 1] = acc;                                                      \
  }

}  // namespace
