// Kernels of the joint CTC / attention FUSION GRID (modeling/beam_search_device.py:joint_beam_search_device_grid; DESIGN.md
// section 24).  A search is an (utterance, lm_weight) pair: S searches of width W occupy rows s * W .. s * W + W - 1 as in the
// batched search (csrc/decode_batch.hip), sutt[s] is the utterance of search s (searches of one utterance are consecutive), the
// frames of utterance u are the rows moff[u] .. moff[u + 1] - 1 of everything stacked over frames, and the LM weight is mu[s].
// Every kernel here compiles the body its scalar twin compiles (csrc/attn_group_body.h, csrc/beam_scores_topk_body.h,
// csrc/ctc_prefix_body.h, csrc/beam_update_batch_body.h): a row's bits are those of the twin run on that row's search.
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"
#include "attn_group.h"
#include "beam_score_step.h"
#include "beam_update_batch.h"

namespace {

// One workgroup per (group g, head h).  groups[g] = {first row, rows (1..32), utterance}: the rows of consecutive searches of
// ONE utterance, so a K / V tile is fetched once for all of them.  Rows of the group beyond its count are never written; a table
// entry that does not fit the launch (rows outside 0..nb, more rows than the instantiation holds, no such utterance) is skipped.
template <typename T, int DK, int TK, int WB>
__global__ __launch_bounds__(G_THREADS) void attn_step_cells_kernel(int nb, int U, int H, const T* __restrict__ q,
                                                                    const T* __restrict__ kv, const int* __restrict__ moff,
                                                                    const int* __restrict__ groups, float scale, T* __restrict__ out) {
#define EMO_ATTN_GROUP_OF_BLOCK                                                              \
  const int g = blockIdx.x, h = blockIdx.y;                                                  \
  const int row0 = groups[3 * g], W = groups[3 * g + 1], u = groups[3 * g + 2];              \
  if (W < 1 || W > WB || row0 < 0 || row0 + W > nb || u < 0 || u >= U) return;               \
  const long r0 = moff[u];                                                                   \
  const int Ts = moff[u + 1] - moff[u];
#define EMO_ATTN_ROW(w) ((long)row0 + w)
#include "attn_group_body.h"
#undef EMO_ATTN_ROW
#undef EMO_ATTN_GROUP_OF_BLOCK
}

template <typename T>
int launch_cells(int G, int max_rows, int nb, int U, int H, int dk, const void* q, const void* kv, const int* moff, const int* groups,
                 float scale, void* out, hipStream_t s) {
  dim3 grid(G, H);
#define EMO_ATTN_GROUP_LAUNCH(DK, TK, WB) \
  attn_step_cells_kernel<T, DK, TK, WB><<<grid, G_THREADS, 0, s>>>(nb, U, H, (const T*)q, (const T*)kv, moff, groups, scale, (T*)out)
  switch (dk) {
    EMO_ATTN_GROUP_CASE(32, 64, max_rows)
    EMO_ATTN_GROUP_CASE(64, 64, max_rows)
    EMO_ATTN_GROUP_CASE(128, 32, max_rows)
    default:
      emo_set_error("attn_step_cells: head width %d (supported: 32, 64, 128)", dk);
      return 1;
  }
#undef EMO_ATTN_GROUP_LAUNCH
  return 0;
}

template <typename T>
__global__ __launch_bounds__(1024) void beam_scores_topk_rows_kernel(int V, int k, const T* __restrict__ dec, long ldd,
                                                                     const float* __restrict__ lm, long ldl,
                                                                     const float* __restrict__ mu_row, float* __restrict__ vals,
                                                                     int* __restrict__ idx, float* __restrict__ lm_at, int lm_lds) {
  const float mu = lm ? mu_row[blockIdx.x] : 0.f;
#include "beam_scores_topk_body.h"
}

__global__ __launch_bounds__(64) void ctc_prefix_cells_kernel(int Tn, int V, int cw, const float* __restrict__ x,
                                                              const float* __restrict__ prev_states, int cw_prev,
                                                              const int* __restrict__ parent, const int* __restrict__ pcand,
                                                              const int* __restrict__ last, const int* __restrict__ out_len,
                                                              const int* __restrict__ cands, int blank, int eos,
                                                              float* __restrict__ log_psi, float* __restrict__ states,
                                                              const int* __restrict__ xoff, int W, const int* __restrict__ sutt) {
  constexpr bool RAGGED = true;
  const float* init_state = nullptr;   // (the searches always start from a previous state)
#define EMO_CTC_FRAMES_OF(s) sutt[s]
#include "ctc_prefix_body.h"
#undef EMO_CTC_FRAMES_OF
}

// One workgroup (one wave) per utterance u: lane 0 computes the initial state once, into the slot of the utterance's first
// search; the lanes then copy it to the slots of its other searches.
__global__ __launch_bounds__(64) void ctc_prefix_init_cells_kernel(int S, int V, const float* __restrict__ x, int blank,
                                                                   float* __restrict__ r, const int* __restrict__ xoff,
                                                                   const int* __restrict__ sutt, long r_stride) {
  const int u = blockIdx.x, lane = threadIdx.x;
  int s0 = -1;
  for (int s = 0; s < S; ++s)
    if (sutt[s] == u) { s0 = s; break; }
  if (s0 < 0) return;   // (uniform: no search of this launch runs over the utterance)
  const int Tn = xoff[u + 1] - xoff[u];
  float* first = r + s0 * r_stride;
  if (lane == 0) {
    const float* xu = x + (long)xoff[u] * V;
    EMO_CTC_PREFIX_INIT_ROWS(Tn, V, xu, blank, first)
  }
  __syncthreads();
  for (int s = s0 + 1; s < S; ++s) {
    if (sutt[s] != u) continue;
    float* dst = r + s * r_stride;
    for (int i = lane; i < 2 * Tn; i += 64) dst[i] = first[i];
  }
}

__global__ __launch_bounds__(256) void beam_update_cells_kernel(emoasr_beam_update_batch_t b, const float* __restrict__ mu) {
#define EMO_UPDATE_MU(s) mu[s]
#include "beam_update_batch_body.h"
#undef EMO_UPDATE_MU
}

__global__ void beam_cells_tail_kernel(emoasr_beam_update_batch_t b) { beam_batch_tail_body(b); }

}  // namespace

extern "C" int emoasr_attn_step_cells(int dtype, int G, int max_rows, int nb, int U, int dd, int H, const void* q, const void* kv,
                                      const int* moff, const int* groups, void* out, void* stream) {
  EMO_CHECK(q && kv && moff && groups && out, "attn_step_cells: missing arguments");
  EMO_CHECK(G >= 1 && max_rows >= 1 && max_rows <= G_MAXW, "attn_step_cells: %d groups of up to %d rows (1..32)", G, max_rows);
  EMO_CHECK(nb >= 1 && U >= 1, "attn_step_cells: %d rows, %d utterances", nb, U);
  EMO_CHECK(H >= 1 && dd % H == 0, "attn_step_cells: dd=%d H=%d", dd, H);
  EMO_CHECK(((size_t)kv & 15) == 0, "attn_step_cells: the memory must be 16-byte aligned");
  const float scale = 1.f / sqrtf((float)(dd / H));
  EMO_DISPATCH(dtype, if (launch_cells<T>(G, max_rows, nb, U, H, dd / H, q, kv, moff, groups, scale, out, (hipStream_t)stream)) return 1);
  EMO_LAUNCH_CHECK();
  return 0;
}

/* host-side check of a group table before it is uploaded: every row 0 .. nb - 1 in exactly one group, in order; 1..max_rows
 * rows per group; utterances inside 0 .. U - 1 */
extern "C" int emoasr_cell_groups_check(int G, const int* groups_host, int max_rows, int nb, int U) {
  EMO_CHECK(groups_host && G >= 1 && max_rows >= 1 && max_rows <= G_MAXW, "cell groups: missing, or %d rows per group outside 1..32", max_rows);
  int next = 0;
  for (int g = 0; g < G; ++g) {
    const int row0 = groups_host[3 * g], n = groups_host[3 * g + 1], u = groups_host[3 * g + 2];
    EMO_CHECK(row0 == next && n >= 1 && n <= max_rows && u >= 0 && u < U, "cell groups: group %d = {row %d, %d rows, utterance %d} (next row %d, "
              "up to %d rows, %d utterances)", g, row0, n, u, next, max_rows, U);
    next += n;
  }
  EMO_CHECK(next == nb, "cell groups: the groups cover %d of %d rows", next, nb);
  return 0;
}

extern "C" int emoasr_beam_scores_topk_rows(int dtype, int M, int V, int k, const void* dec, long ldd, const float* lm, long ldl,
                                            const float* mu_row, float* vals, int* idx, float* lm_at, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(k >= 1 && k <= V, "beam_scores_topk_rows: k=%d V=%d", k, V);
  EMO_CHECK(!lm || mu_row, "beam_scores_topk_rows: an LM operand without the rows' weights");
  int lm_lds = 0;
  const int bytes = beam_scores_topk_lds_bytes(V, k, lm != nullptr, &lm_lds);
  EMO_CHECK(bytes > 0, "beam_scores_topk_rows: V=%d, k=%d too large for the LDS plan", V, k);
  if (dtype == EMO_BF16) {
    if (bytes > 60 * 1024) hipFuncSetAttribute((const void*)beam_scores_topk_rows_kernel<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    beam_scores_topk_rows_kernel<bf16><<<M, 1024, bytes, (hipStream_t)stream>>>(V, k, (const bf16*)dec, ldd, lm, ldl, mu_row, vals, idx, lm_at, lm_lds);
  } else if (emo_is_f32(dtype)) {
    if (bytes > 60 * 1024) hipFuncSetAttribute((const void*)beam_scores_topk_rows_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    beam_scores_topk_rows_kernel<float><<<M, 1024, bytes, (hipStream_t)stream>>>(V, k, (const float*)dec, ldd, lm, ldl, mu_row, vals, idx, lm_at, lm_lds);
  } else {
    emo_set_error("bad dtype %d", dtype);
    return 1;
  }
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_prefix_init_cells(int S, int U, int V, const float* x, const int* xoff, const int* sutt, int blank, float* r,
                                            long r_stride, void* stream) {
  EMO_CHECK(S >= 1 && U >= 1 && x && xoff && sutt && r, "ctc_prefix_init_cells: missing arguments");
  ctc_prefix_init_cells_kernel<<<U, 64, 0, (hipStream_t)stream>>>(S, V, x, blank, r, xoff, sutt, r_stride);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_prefix_score_cells(int nb, int W, int Tmax, int V, int cw, const float* x, const int* xoff, const int* sutt,
                                             const float* prev_states, int cw_prev, const int* parent, const int* pcand,
                                             const int* last, const int* out_len, const int* cands, int blank, int eos,
                                             float* log_psi, float* states, void* stream) {
  if (nb == 0) return 0;
  EMO_CHECK(W >= 1 && W <= 32 && nb % W == 0, "ctc_prefix_score_cells: %d rows in groups of %d (1..32)", nb, W);
  EMO_CHECK(cw >= 1 && cw <= 32, "ctc_prefix_score_cells: cw=%d outside 1..32", cw);
  EMO_CHECK(x && xoff && sutt && prev_states && Tmax >= 1, "ctc_prefix_score_cells: missing arguments");
  ctc_prefix_cells_kernel<<<nb * cw, 64, 0, (hipStream_t)stream>>>(Tmax, V, cw, x, prev_states, cw_prev, parent, pcand, last, out_len,
                                                                   cands, blank, eos, log_psi, states, xoff, W, sutt);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_beam_update_cells(const emoasr_beam_update_batch_t* b, const float* mu, void* stream) {
  EMO_CHECK(b && mu && b->pos && b->ctl && b->u.state && b->u.vals && b->u.cands && b->u.score && b->u.n_ids, "beam_update_cells: missing arguments");
  EMO_CHECK(b->S >= 1 && b->max_pos >= 1, "beam_update_cells: %d searches, %d positions", b->S, b->max_pos);
  EMO_CHECK(b->u.bw >= 1 && b->u.bw <= 32 && b->u.cw >= 1 && b->u.cw <= 32, "beam_update_cells: beam %d / candidates %d outside 1..32",
            b->u.bw, b->u.cw);
  beam_update_cells_kernel<<<b->S, 256, 0, (hipStream_t)stream>>>(*b, mu);
  beam_cells_tail_kernel<<<1, 64, 0, (hipStream_t)stream>>>(*b);
  EMO_LAUNCH_CHECK();
  return 0;
}
