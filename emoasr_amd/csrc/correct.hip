// CTC error correction (asr/test_asr_correct.py:39-172): what sits between the recogniser's greedy path and the masked LM.
//
//   emoasr_ctc_token_conf  per utterance: the tokens of the greedy path (maximal runs of equal non-blank frames -- the CTC collapse),
//                          and for each the frame of the run where softmax(logits[t])[token] is largest (earliest on ties), that
//                          probability, and the token count.  The reference's aggregate_logits, which copies a [T, V] soft-max to
//                          the host per utterance.
//   emoasr_correct_fuse    per row: argmax_{v < n_cols} (1 - w) softmax(asr)[v] + w softmax(lm)[v] (lowest column on ties) and the
//                          winning value; the LM row's log-sum-exp is formed here.  No probability row leaves the block.
//   emoasr_correct_mask_grid  the masked LM inputs of NT thresholds at once, their counts, and the masked positions as two row lists
//                          (LM row, recogniser row) in (threshold, utterance, token) order -- a scan over the counts, no atomics.
//   emoasr_correct_fuse_grid  emoasr_correct_fuse for up to 16 weights in one read of the two rows: both probabilities are formed
//                          once per column, every weight keeps its own running (value, column).
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

// the log-sum-exp of one LM row over all Vl columns, by the whole block (running maximum and sum, as electra.hip's sample_rows)
template <typename TL>
__device__ __forceinline__ double lm_row_lse(const TL* lrow, int Vl, int tid, float* red) {
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
  return (double)bm + log((double)se);
}

// f(v, a, l) for the columns v < n_cols of this thread, ascending: 8-column groups where both rows are aligned, else by element
template <typename TA, typename TL, typename F>
__device__ __forceinline__ void each_column(const TA* arow, const TL* lrow, int n_cols, int tid, F f) {
  const int body = min(vec_body(arow, n_cols), vec_body(lrow, n_cols));
  for (int v0 = tid * 8; v0 < body; v0 += 256 * 8) {
    float a[8], l[8];
    load8(arow + v0, a);
    load8(lrow + v0, l);
#pragma unroll
    for (int e = 0; e < 8; ++e) f(v0 + e, a[e], l[e]);
  }
  for (int v = body + tid; v < n_cols; v += 256) f(v, to_f32(arow[v]), to_f32(lrow[v]));
}

// the larger (value, column) of the wave, the lowest column on ties, in every lane
__device__ __forceinline__ void wave_argmax(float& best, int& col) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(col, o, 64);
    if (ob > best || (ob == best && oc < col)) { best = ob; col = oc; }
  }
}

// One block per row.  Pass 1: the LM row's maximum and sum of exponentials.  Pass 2: the mixed probability of every column below
// n_cols, and its arg-max.
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
  const double lse_l = lm_row_lse(lrow, Vl, tid, red);
  const double lse_a = (double)asr_lse[ra];

  const float wa = 1.f - w;
  float best = -INFINITY;
  int col = 0x7fffffff;
  each_column(arow, lrow, n_cols, tid, [&](int v, float a, float l) {
    const float p = wa * exp_diff(a, lse_a) + w * exp_diff(l, lse_l);
    if (p > best) { best = p; col = v; }     // (columns ascend within a thread: the first maximum stays)
  });
  wave_argmax(best, col);
  if ((tid & 63) == 0) { bval[tid >> 6] = best; bcol[tid >> 6] = col; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k)
      if (bval[k] > best || (bval[k] == best && bcol[k] < col)) { best = bval[k]; col = bcol[k]; }
    out_id[i] = min(max(col, 0), n_cols - 1);
    out_val[i] = best;
  }
}

// correct_fuse_kernel for up to NW weights: the two passes over the rows are the single kernel's; in pass 2 the two probabilities of
// a column are formed once and every weight keeps its own running (value, column).  Per weight the arithmetic and the reductions
// are the single kernel's, so its ids and values are that kernel's bit for bit.  Weights from nw on (the bucket's padding) are
// walked with w = 0 and never written.
struct FuseWeights { float w[EMO_CORRECT_MAX_WEIGHTS]; };

template <typename TA, typename TL, int NW>
__global__ __launch_bounds__(256) void correct_fuse_grid_kernel(int Vl, int n_cols, const TA* __restrict__ asr, long lda,
                                                                const float* __restrict__ asr_lse,
                                                                const int* __restrict__ asr_rows, long asr_nrows,
                                                                const TL* __restrict__ lm, long ldl, FuseWeights ws, int nw, long n,
                                                                int* __restrict__ out_id, float* __restrict__ out_val) {
  __shared__ float red[16];
  __shared__ float bval[NW][4];
  __shared__ int bcol[NW][4];
  const long i = blockIdx.x;
  long ra = asr_rows ? (long)asr_rows[i] : i;
  ra = ra < 0 ? 0 : (ra >= asr_nrows ? asr_nrows - 1 : ra);
  const TA* arow = asr + ra * lda;
  const TL* lrow = lm + i * ldl;
  const int tid = threadIdx.x;
  const double lse_l = lm_row_lse(lrow, Vl, tid, red);
  const double lse_a = (double)asr_lse[ra];

  float wl[NW], wa[NW], best[NW];
  int col[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    wl[k] = ws.w[k];
    wa[k] = 1.f - wl[k];
    best[k] = -INFINITY;
    col[k] = 0x7fffffff;
  }
  each_column(arow, lrow, n_cols, tid, [&](int v, float a, float l) {
    const float pa = exp_diff(a, lse_a), pl = exp_diff(l, lse_l);
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      const float p = wa[k] * pa + wl[k] * pl;
      if (p > best[k]) { best[k] = p; col[k] = v; }
    }
  });
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    wave_argmax(best[k], col[k]);
    if ((tid & 63) == 0) { bval[k][tid >> 6] = best[k]; bcol[k][tid >> 6] = col[k]; }
  }
  __syncthreads();
  if (tid < nw) {
    float b = bval[tid][0];
    int c = bcol[tid][0];
    for (int k = 1; k < 4; ++k)
      if (bval[tid][k] > b || (bval[tid][k] == b && bcol[tid][k] < c)) { b = bval[tid][k]; c = bcol[tid][k]; }
    out_id[(long)tid * n + i] = min(max(c, 0), n_cols - 1);
    out_val[(long)tid * n + i] = b;
  }
}

// One wave per (threshold, utterance).  mask_count_kernel writes the masked LM input row and the pair's count; mask_list_kernel
// finds the pair's place in the lists as the sum of the counts of the pairs before it (the pairs are numbered th * B + b, which is
// the lists' order) and writes its masked tokens there in token order.  Both walk the tokens 64 at a time and make the same
// comparison, conf < th.
__global__ __launch_bounds__(64) void mask_count_kernel(int B, int Tn, const int* __restrict__ hyp, const int* __restrict__ ntok,
                                                        const float* __restrict__ conf, const float* __restrict__ ths, int mask_id,
                                                        int pad_id, int* __restrict__ ys, int* __restrict__ num_masked) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int b = pair % B;
  const float th = ths[pair / B];
  const int n = max(min(ntok[b], Tn), 0);
  const long r0 = (long)b * Tn, y0 = (long)pair * Tn;
  int count = 0;
  for (int j0 = 0; j0 < Tn; j0 += 64) {
    const int j = j0 + lane;
    const bool m = j < n && conf[r0 + j] < th;
    if (j < Tn) ys[y0 + j] = j < n ? (m ? mask_id : hyp[r0 + j]) : pad_id;
    count += __popcll(__ballot(m));
  }
  if (lane == 0) num_masked[pair] = count;
}

__global__ __launch_bounds__(64) void mask_list_kernel(int B, int Tn, const int* __restrict__ ntok, const float* __restrict__ conf,
                                                       const int* __restrict__ frame, const float* __restrict__ ths,
                                                       const int* __restrict__ num_masked, int* __restrict__ lm_rows,
                                                       int* __restrict__ asr_rows) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  int off = 0;
  for (int q = lane; q < pair; q += 64) off += num_masked[q];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) off += __shfl_xor(off, o, 64);
  const int b = pair % B;
  const float th = ths[pair / B];
  const int n = max(min(ntok[b], Tn), 0);
  const long r0 = (long)b * Tn, y0 = (long)pair * Tn;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const bool m = j < n && conf[r0 + j] < th;
    const unsigned long long mask = __ballot(m);
    if (m) {
      const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
      lm_rows[pos] = (int)(y0 + j);
      asr_rows[pos] = (int)(r0 + min(max(frame[r0 + j], 0), Tn - 1));
    }
    off += __popcll(mask);
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

template <typename TA, typename TL>
int fuse_grid_launch(int n, int Vl, int n_cols, const TA* asr, long lda, const float* asr_lse, const int* asr_rows, long asr_nrows,
                     const TL* lm, long ldl, const FuseWeights& ws, int nw, int* out_id, float* out_val, hipStream_t s) {
#define EMO_FUSE_GRID(NW) \
  correct_fuse_grid_kernel<TA, TL, NW><<<n, 256, 0, s>>>(Vl, n_cols, asr, lda, asr_lse, asr_rows, asr_nrows, lm, ldl, ws, nw, n, \
                                                         out_id, out_val)
  if (nw == 1) EMO_FUSE_GRID(1);
  else if (nw <= 4) EMO_FUSE_GRID(4);
  else if (nw <= 8) EMO_FUSE_GRID(8);
  else EMO_FUSE_GRID(EMO_CORRECT_MAX_WEIGHTS);
#undef EMO_FUSE_GRID
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

extern "C" int emoasr_correct_mask_grid(int B, int Tn, int NT, const int* hyp, const int* ntok, const float* conf, const int* frame,
                                        const float* ths, int mask_id, int pad_id, int* ys, int* num_masked, int* lm_rows,
                                        int* asr_rows, void* stream) {
  if (B == 0 || NT == 0) return 0;
  EMO_CHECK(B > 0 && Tn >= 1 && NT > 0 && (long)NT * B * Tn <= 0x7fffffffL, "correct_mask_grid: B=%d T=%d NT=%d", B, Tn, NT);
  EMO_CHECK(hyp && ntok && conf && frame && ths && ys && num_masked && lm_rows && asr_rows, "correct_mask_grid: null argument");
  mask_count_kernel<<<NT * B, 64, 0, (hipStream_t)stream>>>(B, Tn, hyp, ntok, conf, ths, mask_id, pad_id, ys, num_masked);
  EMO_LAUNCH_CHECK();
  mask_list_kernel<<<NT * B, 64, 0, (hipStream_t)stream>>>(B, Tn, ntok, conf, frame, ths, num_masked, lm_rows, asr_rows);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_correct_fuse_grid(int dtype_asr, int dtype_lm, int n, int V_asr, int V_lm, int n_cols, const void* asr,
                                        long ld_asr, const float* asr_lse, const int* asr_rows, long asr_nrows, const void* lm,
                                        long ld_lm, const float* weights, int NW, int* out_id, float* out_val, void* stream) {
  if (n == 0 || NW == 0) return 0;
  EMO_CHECK(n > 0 && n_cols >= 1 && n_cols <= V_asr && n_cols <= V_lm && ld_asr >= V_asr && ld_lm >= V_lm,
            "correct_fuse_grid: n=%d V_asr=%d V_lm=%d n_cols=%d ld_asr=%ld ld_lm=%ld", n, V_asr, V_lm, n_cols, ld_asr, ld_lm);
  EMO_CHECK(asr_nrows >= 1 && (asr_rows || asr_nrows >= n), "correct_fuse_grid: %ld recogniser rows for n=%d", asr_nrows, n);
  EMO_CHECK(NW >= 1 && NW <= EMO_CORRECT_MAX_WEIGHTS, "correct_fuse_grid: %d weights, at most %d per launch", NW,
            EMO_CORRECT_MAX_WEIGHTS);
  EMO_CHECK(asr && asr_lse && lm && weights && out_id && out_val, "correct_fuse_grid: null argument");
  FuseWeights ws = {};
  for (int k = 0; k < NW; ++k) {     // (the weights are HOST floats: they travel as a kernel argument)
    EMO_CHECK(weights[k] >= 0.f && weights[k] <= 1.f, "correct_fuse_grid: lm weight %g outside [0, 1]", (double)weights[k]);
    ws.w[k] = weights[k];
  }
  const bool a16 = dtype_asr == EMO_BF16, l16 = dtype_lm == EMO_BF16;
  EMO_CHECK(a16 || dtype_asr == EMO_F32 || dtype_asr == EMO_F32X3, "bad dtype %d", dtype_asr);
  EMO_CHECK(l16 || dtype_lm == EMO_F32 || dtype_lm == EMO_F32X3, "bad dtype %d", dtype_lm);
  hipStream_t s = (hipStream_t)stream;
  if (a16 && l16) fuse_grid_launch(n, V_lm, n_cols, (const bf16*)asr, ld_asr, asr_lse, asr_rows, asr_nrows, (const bf16*)lm, ld_lm, ws, NW, out_id, out_val, s);
  else if (a16) fuse_grid_launch(n, V_lm, n_cols, (const bf16*)asr, ld_asr, asr_lse, asr_rows, asr_nrows, (const float*)lm, ld_lm, ws, NW, out_id, out_val, s);
  else if (l16) fuse_grid_launch(n, V_lm, n_cols, (const float*)asr, ld_asr, asr_lse, asr_rows, asr_nrows, (const bf16*)lm, ld_lm, ws, NW, out_id, out_val, s);
  else fuse_grid_launch(n, V_lm, n_cols, (const float*)asr, ld_asr, asr_lse, asr_rows, asr_nrows, (const float*)lm, ld_lm, ws, NW, out_id, out_val, s);
  EMO_LAUNCH_CHECK();
  return 0;
}
