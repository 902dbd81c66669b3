// CTC error correction (asr/test_asr_correct.py:39-172): what sits between the recogniser's greedy path and the masked LM.
//
//   emoasr_ctc_token_conf  per utterance: the tokens of the greedy path (maximal runs of equal non-blank frames -- the CTC collapse),
//                          and for each the frame of the run where softmax(logits[t])[token] is largest (earliest on ties), that
//                          probability, and the token count.  The reference's aggregate_logits, which copies a [T, V] soft-max to
//                          the host per utterance.
//   emoasr_correct_fuse    per row: argmax_{v < n_cols} (1 - w) softmax(asr)[v] + w softmax(lm)[v] (lowest column on ties) and the
//                          winning value; the LM row's log-sum-exp is formed here.  No probability row leaves the block.
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

// exp(x - c) for an f32 x and a double c: the difference is formed exactly and split into an f32 head and tail, so the result
// carries expf's error alone (not the half ulp of |x - c|, which is 2.4e-7 relative for a probability of 1e-2).
__device__ __forceinline__ float exp_diff(float x, double c) {
  if (x == -INFINITY) return 0.f;
  const double d = (double)x - c;
  const float hi = (float)d;
  const float lo = (float)(d - (double)hi);
  const float e = expf(hi);
  return e + e * lo;
}

// One wave per utterance, 64 frames per pass (the walk of ctc.hip's collapse_kernel, which numbers the tokens the same way).  A
// lane with a non-blank frame holds p = softmax(logits[t])[id]; a segmented shuffle scan leaves each run's best (p, t) at the run's
// first lane: runs are contiguous, so "the lane o further on belongs to my token" is the whole segment test.  A run that goes on
// into the next 64 frames is carried in registers and written once, when it ends.
template <typename T>
__global__ __launch_bounds__(64) void token_conf_kernel(int B, int Tn, int V, const T* __restrict__ logits, long ld,
                                                        const float* __restrict__ lse, const int* __restrict__ best,
                                                        const int* __restrict__ elens, int blank, int* __restrict__ frame,
                                                        float* __restrict__ conf, int* __restrict__ ntok) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const int len = max(min(elens[b], Tn), 0);
  const long r0 = (long)b * Tn;
  int n = 0, carry_v = -1, ct = 0;
  float cp = 0.f;
  for (int t0 = 0; t0 < len; t0 += 64) {
    const int t = t0 + lane;
    const bool in = t < len;
    int v = in ? best[r0 + t] : blank;
    if (v < 0 || v >= V) v = blank;     // (an id outside the row is never used as a column)
    int prev = __shfl_up(v, 1, 64);
    if (lane == 0) prev = carry_v;
    const bool nb = in && v != blank;
    const bool keep = nb && v != prev;
    const unsigned long long mask = __ballot(keep);
    const int j = n + __popcll(mask & ((2ull << lane) - 1ull)) - 1;    // token of this frame (lane 63: 2 << 63 wraps to all ones)
    float p = -1.f;
    int pt = t;
    if (nb) p = exp_diff(to_f32(logits[(r0 + t) * ld + v]), (double)lse[r0 + t]);
    const int seg = nb ? j : -1 - lane;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float op = __shfl_down(p, o, 64);
      const int ot = __shfl_down(pt, o, 64);
      const int os = __shfl_down(seg, o, 64);
      if (lane + o < 64 && os == seg && op > p) { p = op; pt = ot; }   // (strictly larger: the earlier frame keeps a tie)
    }
    const bool goes_on = lane == 0 && nb && !keep;                       // the run carried in from the frames before
    if (goes_on && !(p > cp)) { p = cp; pt = ct; }
    const bool head = keep || goes_on;
    const int v63 = __shfl(v, 63, 64);
    bool cont = false;                                                   // does the last run reach into the next pass?
    if (t0 + 64 < len) {
      int nx = best[r0 + t0 + 64];
      if (nx < 0 || nx >= V) nx = blank;
      cont = v63 != blank && nx == v63;
    }
    const unsigned long long heads = __ballot(head);
    const int hl = heads ? 63 - __clzll(heads) : 0;
    if (head && !(cont && lane == hl)) { conf[r0 + j] = p; frame[r0 + j] = pt; }
    if (cont) { cp = __shfl(p, hl, 64); ct = __shfl(pt, hl, 64); }
    n += __popcll(mask);
    carry_v = v63;
  }
  if (lane == 0) ntok[b] = n;
}

// the 8-column groups of a 16-byte aligned row as 16-byte loads, the ragged end (or an unaligned row) by element
template <typename T>
__device__ __forceinline__ int vec_body(const T* row, int V) {
  return (((uintptr_t)row & 15) == 0) ? (V & ~7) : 0;
}

// One block per row.  Pass 1: the LM row's maximum and sum of exponentials (running, as electra.hip's sample_rows).  Pass 2: the
// mixed probability of every column below n_cols, and its arg-max.
template <typename TA, typename TL>
__global__ __launch_bounds__(256) void correct_fuse_kernel(int Va, int Vl, int n_cols, const TA* __restrict__ asr, long lda,
                                                           const float* __restrict__ asr_lse, const int* __restrict__ asr_rows,
                                                           long asr_nrows, const TL* __restrict__ lm, long ldl, float w,
                                                           int* __restrict__ out_id, float* __restrict__ out_val) {
  __shared__ float red[16];
  __shared__ float bval[4];
  __shared__ int bcol[4];
  const long i = blockIdx.x;
  long ra = asr_rows ? (long)asr_rows[i] : i;
  ra = ra < 0 ? 0 : (ra >= asr_nrows ? asr_nrows - 1 : ra);
  const TA* arow = asr + ra * lda;
  const TL* lrow = lm + i * ldl;
  const int tid = threadIdx.x;

  float mx = -INFINITY, se = 0.f;
  auto take = [&](float x) {
    if (x > mx) { se = se * expf(mx - x) + 1.f; mx = x; }
    else if (x != -INFINITY) se += expf(x - mx);
  };
  const int lbody = vec_body(lrow, Vl);
  for (int v0 = tid * 8; v0 < lbody; v0 += 256 * 8) {
    float x[8];
    load8(lrow + v0, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) take(x[e]);
  }
  for (int v = lbody + tid; v < Vl; v += 256) take(to_f32(lrow[v]));
  const float bm = block_max(mx, red);
  se = block_sum(mx == -INFINITY ? 0.f : se * expf(mx - bm), red);
  const double lse_l = (double)bm + log((double)se);
  const double lse_a = (double)asr_lse[ra];

  const float wa = 1.f - w;
  float best = -INFINITY;
  int col = 0x7fffffff;
  auto mix = [&](int v, float a, float l) {
    const float p = wa * exp_diff(a, lse_a) + w * exp_diff(l, lse_l);
    if (p > best) { best = p; col = v; }     // (columns ascend within a thread: the first maximum stays)
  };
  const int body = min(vec_body(arow, n_cols), vec_body(lrow, n_cols));
  for (int v0 = tid * 8; v0 < body; v0 += 256 * 8) {
    float a[8], l[8];
    load8(arow + v0, a);
    load8(lrow + v0, l);
#pragma unroll
    for (int e = 0; e < 8; ++e) mix(v0 + e, a[e], l[e]);
  }
  for (int v = body + tid; v < n_cols; v += 256) mix(v, to_f32(arow[v]), to_f32(lrow[v]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(col, o, 64);
    if (ob > best || (ob == best && oc < col)) { best = ob; col = oc; }
  }
  if ((tid & 63) == 0) { bval[tid >> 6] = best; bcol[tid >> 6] = col; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k)
      if (bval[k] > best || (bval[k] == best && bcol[k] < col)) { best = bval[k]; col = bcol[k]; }
    out_id[i] = min(max(col, 0), n_cols - 1);
    out_val[i] = best;
  }
}

template <typename TA>
int fuse_launch(int dtype_lm, int n, int Va, int Vl, int n_cols, const void* asr, long lda, const float* asr_lse,
                const int* asr_rows, long asr_nrows, const void* lm, long ldl, float w, int* out_id, float* out_val,
                hipStream_t s) {
  EMO_DISPATCH(dtype_lm, (correct_fuse_kernel<TA, T><<<n, 256, 0, s>>>(Va, Vl, n_cols, (const TA*)asr, lda, asr_lse, asr_rows,
                                                                       asr_nrows, (const T*)lm, ldl, w, out_id, out_val)));
  return 0;
}

}  // namespace

extern "C" int emoasr_ctc_token_conf(int dtype, int B, int Tn, int V, const void* logits, long ld, const float* lse,
                                     const int* best, const int* elens, int blank, int* frame, float* conf, int* ntok,
                                     void* stream) {
  if (B == 0) return 0;
  EMO_CHECK(B > 0 && Tn >= 1 && V >= 1 && ld >= V, "ctc_token_conf: B=%d T=%d V=%d ld=%ld", B, Tn, V, ld);
  EMO_CHECK(logits && lse && best && elens && frame && conf && ntok, "ctc_token_conf: null argument");
  EMO_DISPATCH(dtype, (token_conf_kernel<T><<<B, 64, 0, (hipStream_t)stream>>>(B, Tn, V, (const T*)logits, ld, lse, best, elens,
                                                                               blank, frame, conf, ntok)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_correct_fuse(int dtype_asr, int dtype_lm, int n, int V_asr, int V_lm, int n_cols, const void* asr,
                                   long ld_asr, const float* asr_lse, const int* asr_rows, long asr_nrows, const void* lm,
                                   long ld_lm, float w, int* out_id, float* out_val, void* stream) {
  if (n == 0) return 0;
  EMO_CHECK(n > 0 && n_cols >= 1 && n_cols <= V_asr && n_cols <= V_lm && ld_asr >= V_asr && ld_lm >= V_lm,
            "correct_fuse: n=%d V_asr=%d V_lm=%d n_cols=%d ld_asr=%ld ld_lm=%ld", n, V_asr, V_lm, n_cols, ld_asr, ld_lm);
  EMO_CHECK(asr_nrows >= 1 && (asr_rows || asr_nrows >= n), "correct_fuse: %ld recogniser rows for n=%d", asr_nrows, n);
  EMO_CHECK(w >= 0.f && w <= 1.f, "correct_fuse: lm weight %g outside [0, 1]", (double)w);
  EMO_CHECK(asr && asr_lse && lm && out_id && out_val, "correct_fuse: null argument");
  int rc;
  if (dtype_asr == EMO_BF16) {
    rc = fuse_launch<bf16>(dtype_lm, n, V_asr, V_lm, n_cols, asr, ld_asr, asr_lse, asr_rows, asr_nrows, lm, ld_lm, w, out_id,
                           out_val, (hipStream_t)stream);
  } else if (dtype_asr == EMO_F32 || dtype_asr == EMO_F32X3) {
    rc = fuse_launch<float>(dtype_lm, n, V_asr, V_lm, n_cols, asr, ld_asr, asr_lse, asr_rows, asr_nrows, lm, ld_lm, w, out_id,
                            out_val, (hipStream_t)stream);
  } else {
    emo_set_error("bad dtype %d", dtype_asr);
    return 1;
  }
  if (rc) return rc;
  EMO_LAUNCH_CHECK();
  return 0;
}
