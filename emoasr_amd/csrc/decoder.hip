// Transformer-decoder side kernels: token embedding (+ sqrt(d) scale, absolute positional
// encoding, dropout) forward/backward, and the label-smoothing cross-entropy (loss + gradient).
//
// Reference: asr/modeling/decoders/transformer.py:99 (self.pe(self.embed(ys_in))),
// asr/modeling/transformer.py:43-45, asr/criteria.py:5-46 (LabelSmoothingLoss: 1-eps on the label,
// eps/(V-1) on every other class, summed over t < ylens[b], optional /ylen and /B).
#include "common.h"
#include "../../include/emoasr_hip.h"
#include "beam_score_step.h"

namespace {

// out[m, :] = (table[ids[m], :] * scale + pe[m % L, :]) * dropout(seed, m*d + c)
template <typename T>
__global__ __launch_bounds__(256) void embed_fwd_kernel(int M, int L, int d, const int* __restrict__ ids,
                                                        const T* __restrict__ table,
                                                        const float* __restrict__ pe, float scale, float p,
                                                        uint64_t seed, T* __restrict__ out) {
  const long n = (long)M * d;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = i % d;
    const long m = i / d;
    float v = to_f32(table[(long)ids[m] * d + c]) * scale;
    if (pe) v += pe[(m % L) * d + c];
    out[i] = from_f32<T>(v * dropout_scale(seed, (uint64_t)i, p));
  }
}

// dtable[ids[m], :] += dout[m, :] * scale * dropout(seed, m*d + c)
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_kernel(int M, int d, const int* __restrict__ ids,
                                                        const T* __restrict__ dout, float scale, float p,
                                                        uint64_t seed, float* __restrict__ dtable) {
  const long n = (long)M * d;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = i % d;
    const long m = i / d;
    atomicAdd(&dtable[(long)ids[m] * d + c], to_f32(dout[i]) * scale * dropout_scale(seed, (uint64_t)i, p));
  }
}

// One block per row m.  w[m] = 0 for padded positions, else the row weight (1/B, /ylen).
//   loss[m] = -w * ((1-eps) * logp[y] + eps/(V-1) * (sum_v logp[v] - logp[y]))
//   grad[m, v] = gscale * w * (softmax[v] - q[v])        (sum_v q = 1)
template <typename T>
__global__ __launch_bounds__(256) void lsm_loss_kernel(int V, const T* __restrict__ logits, long ld,
                                                       const int* __restrict__ labels,
                                                       const float* __restrict__ w, float eps,
                                                       float* __restrict__ loss, float gscale,
                                                       const float* __restrict__ gscale_dev,
                                                       T* __restrict__ grad, long ldg) {
  __shared__ float red[16];
  const long m = blockIdx.x;
  const T* row = logits + m * ld;
  const float wm = w[m];
  if (wm == 0.f) {
    if (threadIdx.x == 0) loss[m] = 0.f;
    if (grad) for (int v = threadIdx.x; v < V; v += 256) grad[m * ldg + v] = from_f32<T>(0.f);
    return;
  }
  float mx = -INFINITY, sum = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) { const float x = to_f32(row[v]); mx = fmaxf(mx, x); sum += x; }
  mx = block_max(mx, red);
  sum = block_sum(sum, red);
  float se = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) se += __expf(to_f32(row[v]) - mx);
  se = block_sum(se, red);
  const float lse = mx + logf(se);
  const int y = labels[m];
  const float lpy = to_f32(row[y]) - lse;
  const float off = eps / (V - 1);
  if (threadIdx.x == 0) loss[m] = -wm * ((1.f - eps) * lpy + off * (sum - V * lse - lpy));
  if (grad) {
    const float gs = (gscale_dev ? gscale * gscale_dev[0] : gscale) * wm;
    for (int v = threadIdx.x; v < V; v += 256) {
      const float pv = __expf(to_f32(row[v]) - lse);
      grad[m * ldg + v] = from_f32<T>(gs * (pv - (v == y ? 1.f - eps : off)));
    }
  }
}

inline int ew_grid(long n) { long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

}  // namespace

extern "C" int emoasr_embed_fwd(int dtype, int M, int L, int d, const int* ids, const void* table,
                                const float* pe, float scale, float drop_p, uint64_t seed, void* out,
                                void* stream) {
  if (M == 0) return 0;
  EMO_DISPATCH(dtype, (embed_fwd_kernel<T><<<ew_grid((long)M * d), 256, 0, (hipStream_t)stream>>>(
                          M, L, d, ids, (const T*)table, pe, scale, drop_p, seed, (T*)out)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_embed_bwd(int dtype, int M, int d, const int* ids, const void* dout, float scale,
                                float drop_p, uint64_t seed, float* dtable, void* stream) {
  if (M == 0) return 0;
  EMO_DISPATCH(dtype, (embed_bwd_kernel<T><<<ew_grid((long)M * d), 256, 0, (hipStream_t)stream>>>(
                          M, d, ids, (const T*)dout, scale, drop_p, seed, dtable)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_lsm_loss(int dtype, int M, int V, const void* logits, long ld, const int* labels,
                               const float* w, float lsm_prob, float* loss, float gscale,
                               const float* gscale_dev, void* grad, long ldg, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(V >= 2, "lsm_loss: V=%d", V);
  EMO_DISPATCH(dtype, (lsm_loss_kernel<T><<<M, 256, 0, (hipStream_t)stream>>>(
                          V, (const T*)logits, ld, labels, w, lsm_prob, loss, gscale, gscale_dev, (T*)grad, ldg)));
  EMO_LAUNCH_CHECK();
  return 0;
}

// =======================================================================================
// Beam-search side kernels (asr/modeling/decoders/transformer.py:161-294, ctc_score.py:13-85)
// =======================================================================================
namespace {

// out[m, v] = log_softmax(x[m, :V])[v] + mu * add[m, v]        (add optional, row stride lda)
template <typename T>
__global__ __launch_bounds__(256) void log_softmax_kernel(int V, const T* __restrict__ x, long ldx,
                                                          const float* __restrict__ add, long lda, float mu,
                                                          float* __restrict__ out, long ldo) {
  __shared__ float red[16];
  const long m = blockIdx.x;
  const T* row = x + m * ldx;
#include "log_softmax_body.h"
  for (int v = threadIdx.x; v < V; v += 256) {
    float r = to_f32(row[v]) - lse;
    if (add) r += mu * add[m * lda + v];
    out[m * ldo + v] = r;
  }
}

// k largest of each row, descending, ties -> lowest index.  k <= 64.  One block per row: k rounds of
// block-wide arg-max over a private copy in LDS (V floats).
__global__ __launch_bounds__(256) void topk_kernel(int V, int k, const float* __restrict__ x, long ldx,
                                                   const float* __restrict__ aux, long ldaux,
                                                   float* __restrict__ vals, int* __restrict__ idx,
                                                   float* __restrict__ aux_out) {
  extern __shared__ float buf[];  // [V]
  __shared__ float rv[4];
  __shared__ int ri[4];
  const long m = blockIdx.x;
  for (int v = threadIdx.x; v < V; v += 256) buf[v] = x[m * ldx + v];
  __syncthreads();
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int v = threadIdx.x; v < V; v += 256) {
      const float c = buf[v];
      if (c > best || (c == best && v < bi)) { best = c; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = best; ri[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w)
        if (rv[w] > best || (rv[w] == best && ri[w] < bi)) { best = rv[w]; bi = ri[w]; }
      if (bi == 0x7fffffff) bi = 0;
      vals[m * k + j] = best;
      idx[m * k + j] = bi;
      if (aux_out) aux_out[m * k + j] = aux[m * ldaux + bi];
      buf[bi] = -INFINITY;
    }
    __syncthreads();
  }
}

// The bodies of the kernels below are csrc/beam_scores_topk_body.h and csrc/ctc_prefix_body.h (shared with csrc/decode_grid.hip).
template <typename T>
__global__ __launch_bounds__(1024) void beam_scores_topk_kernel(int V, int k, const T* __restrict__ dec, long ldd,
                                                                const float* __restrict__ lm, long ldl, float mu,
                                                                float* __restrict__ vals, int* __restrict__ idx,
                                                                float* __restrict__ lm_at, int lm_lds) {
#include "beam_scores_topk_body.h"
}

template <bool RAGGED>
__global__ __launch_bounds__(64) void ctc_prefix_kernel(int Tn, int V, int cw, const float* __restrict__ x,
                                                        const float* __restrict__ prev_states, int cw_prev,
                                                        const int* __restrict__ parent, const int* __restrict__ pcand,
                                                        const float* __restrict__ init_state,
                                                        const int* __restrict__ last, const int* __restrict__ out_len,
                                                        const int* __restrict__ cands, int blank, int eos,
                                                        float* __restrict__ log_psi, float* __restrict__ states,
                                                        const int* __restrict__ xoff, int W) {
#define EMO_CTC_FRAMES_OF(s) s
#include "ctc_prefix_body.h"
#undef EMO_CTC_FRAMES_OF
}

template <bool RAGGED>
__global__ void ctc_prefix_init_kernel(int Tn, int V, const float* __restrict__ x, int blank,
                                       float* __restrict__ r, const int* __restrict__ xoff, long r_stride) {
  if (threadIdx.x != 0) return;
  if constexpr (RAGGED) {   // one block per search: its own frames, its own state slot
    const int s = blockIdx.x;
    x += (long)xoff[s] * V;
    Tn = xoff[s + 1] - xoff[s];
    r += s * r_stride;
  } else {
    if (blockIdx.x != 0) return;
  }
  EMO_CTC_PREFIX_INIT_ROWS(Tn, V, x, blank, r)
}

}  // namespace

extern "C" int emoasr_log_softmax(int dtype, int M, int V, const void* x, long ldx, const float* add, long lda,
                                  float mu, float* out, long ldo, void* stream) {
  if (M == 0) return 0;
  EMO_DISPATCH(dtype, (log_softmax_kernel<T><<<M, 256, 0, (hipStream_t)stream>>>(V, (const T*)x, ldx, add, lda, mu,
                                                                                out, ldo)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_topk(int M, int V, int k, const float* x, long ldx, const float* aux, long ldaux,
                           float* vals, int* idx, float* aux_out, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(k >= 1 && k <= V, "topk: k=%d V=%d", k, V);
  EMO_CHECK((size_t)V * 4 <= 150 * 1024, "topk: V=%d too large for an LDS row", V);
  if ((size_t)V * 4 > 60 * 1024)
    hipFuncSetAttribute((const void*)topk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, V * 4);
  topk_kernel<<<M, 256, sizeof(float) * V, (hipStream_t)stream>>>(V, k, x, ldx, aux, ldaux, vals, idx, aux_out);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_beam_scores_topk(int dtype, int M, int V, int k, const void* dec, long ldd, const float* lm, long ldl,
                                       float mu, float* vals, int* idx, float* lm_at, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(k >= 1 && k <= V, "beam_scores_topk: k=%d V=%d", k, V);
  int lm_lds = 0;   // the LM row staged in LDS as well
  const int bytes = beam_scores_topk_lds_bytes(V, k, lm != nullptr, &lm_lds);
  EMO_CHECK(bytes > 0, "beam_scores_topk: V=%d, k=%d too large for the LDS plan", V, k);
  if (dtype == EMO_BF16) {
    if (bytes > 60 * 1024) hipFuncSetAttribute((const void*)beam_scores_topk_kernel<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    beam_scores_topk_kernel<bf16><<<M, 1024, bytes, (hipStream_t)stream>>>(V, k, (const bf16*)dec, ldd, lm, ldl, mu, vals, idx, lm_at, lm_lds);
  } else if (emo_is_f32(dtype)) {
    if (bytes > 60 * 1024) hipFuncSetAttribute((const void*)beam_scores_topk_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    beam_scores_topk_kernel<float><<<M, 1024, bytes, (hipStream_t)stream>>>(V, k, (const float*)dec, ldd, lm, ldl, mu, vals, idx, lm_at, lm_lds);
  } else {
    emo_set_error("bad dtype %d", dtype);
    return 1;
  }
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_prefix_init(int T, int V, const float* x, int blank, float* r, void* stream) {
  ctc_prefix_init_kernel<false><<<1, 64, 0, (hipStream_t)stream>>>(T, V, x, blank, r, nullptr, 0);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_prefix_score(int nb, int T, int V, int cw, const float* x, const float* prev_states,
                                       int cw_prev, const int* parent, const int* pcand, const float* init_state,
                                       const int* last, const int* out_len, const int* cands, int blank, int eos,
                                       float* log_psi, float* states, void* stream) {
  if (nb == 0) return 0;
  EMO_CHECK(cw >= 1 && cw <= 1024, "ctc_prefix_score: cw=%d", cw);
  EMO_CHECK(prev_states || init_state, "ctc_prefix_score: no previous state");
  ctc_prefix_kernel<false><<<nb * cw, 64, 0, (hipStream_t)stream>>>(T, V, cw, x, prev_states, cw_prev, parent, pcand,
                                                                     init_state, last, out_len, cands, blank, eos,
                                                                     log_psi, states, nullptr, 1);
  EMO_LAUNCH_CHECK();
  return 0;
}

// ---- the ragged twins (batched joint search): S searches of W rows each, x the stacked emissions [sum T_s, V] ----
extern "C" int emoasr_ctc_prefix_init_ragged(int S, int V, const float* x, const int* xoff, int blank, float* r, long r_stride,
                                             void* stream) {
  EMO_CHECK(S >= 1 && x && xoff && r, "ctc_prefix_init_ragged: missing arguments");
  ctc_prefix_init_kernel<true><<<S, 64, 0, (hipStream_t)stream>>>(0, V, x, blank, r, xoff, r_stride);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_prefix_score_ragged(int nb, int W, int Tmax, int V, int cw, const float* x, const int* xoff,
                                              const float* prev_states, int cw_prev, const int* parent, const int* pcand,
                                              const int* last, const int* out_len, const int* cands, int blank, int eos,
                                              float* log_psi, float* states, void* stream) {
  if (nb == 0) return 0;
  EMO_CHECK(W >= 1 && W <= 32 && nb % W == 0, "ctc_prefix_score_ragged: %d rows in groups of %d (1..32)", nb, W);
  EMO_CHECK(cw >= 1 && cw <= 32, "ctc_prefix_score_ragged: cw=%d outside 1..32", cw);
  EMO_CHECK(x && xoff && prev_states && Tmax >= 1, "ctc_prefix_score_ragged: missing arguments");
  ctc_prefix_kernel<true><<<nb * cw, 64, 0, (hipStream_t)stream>>>(Tmax, V, cw, x, prev_states, cw_prev, parent, pcand, nullptr,
                                                                    last, out_len, cands, blank, eos, log_psi, states, xoff, W);
  EMO_LAUNCH_CHECK();
  return 0;
}
