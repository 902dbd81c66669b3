// Location-aware additive attention of the LAS decoder (decoders/las.py:289-342): ONE decoder position for all rows, forward and
// backward.  The step's input is its own previous (dropped) attention weights, so the positions are sequential; everything that is
// not (key projection, query projection, the LSTM products) stays on the GEMMs and arrives here as operands.
//
//   f[t][c]  = sum_k filt[c][k] * aw_prev[t + k - 100]                     (Conv1d(1, 10, 201, padding 100), no bias)
//   e[t]     = w_score . tanh(pk[t] + pq + W_conv f[t] + b_conv)            (pk = W_key eouts[t] + b_key, pq = W_query q + b_query)
//   aw       = softmax_t(e)   (t >= elens[b]: e = -FLT_MAX, as the reference's masked_fill(finfo.min))
//   awd[t]   = aw[t] * keep(seed, step, b, t) / (1 - p)                     (the weights the NEXT position convolves)
//   ctx      = sum_t awd[t] * eouts[t]
//
// Forward: two launches.  las_score_kernel runs one block per (32-frame tile, row): the tile's strip of aw_prev with its halo of 100
// on each side and the 10 x 201 filter are staged in LDS once, the 32 x 10 location features are formed there, then every wave walks
// its frames with lane l owning the 8 attention channels 8l .. 8l+7 (W_conv rows, pq and w_score in registers; A <= 512).
// las_ctx_kernel (one block per (64 context columns, row)) takes the soft-max statistics of the row -- T floats, re-read by every
// block -- and forms the dropped weights and the context.
// Backward: one launch with the same (tile, row) grid.  The tanh image is recomputed per tile (never stored); the soft-max's inner
// product sum_s aw[s] daw[s] equals sum_s awd[s] dawd[s] = awd . dawd_next + dctx . ctx, which every block forms from the STORED
// dropped weights and context, so no second pass over the row is needed.  Gradients that cross tiles or rows (the query, the
// previous weights through the transposed convolution, w_score / W_conv / b_conv / the filter) are reduced per block in LDS and
// added with plain f32 atomics; d(key projection) and d(eouts) are owned by exactly one lane and accumulate without atomics.
#include <algorithm>
#include <cfloat>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int LAS_C = EMOASR_LAS_CONV_CHANNELS, LAS_K = EMOASR_LAS_CONV_WIDTH, LAS_HALO = (LAS_K - 1) / 2;
constexpr int LAS_TT = 32;                          // frames per tile
constexpr int LAS_STRIP = LAS_TT + 2 * LAS_HALO;    // 232 <= 256: one thread per strip element in the transposed convolution
constexpr int LAS_MAX_A = 512;                      // one 8-channel group per lane
constexpr int LAS_CTX_COLS = 64;

__device__ __forceinline__ uint64_t las_idx(const emoasr_las_attend_t& a, int b, int t) {
  return ((uint64_t)a.step * (uint64_t)a.B + (uint64_t)b) * (uint64_t)a.T + (uint64_t)t;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T> __device__ __forceinline__ float exp_t(float x) {
  if constexpr (sizeof(T) == 4) return expf(x); else return __expf(x);
}

// the strip aw_prev[t0 - 100 .. t0 + 32 + 100) (zero outside [0, T) and when there is no previous step) and the filter -> LDS
__device__ __forceinline__ void las_stage(const float* __restrict__ awp_row, const float* __restrict__ filt, int T, int t0,
                                          float* s_strip, float* s_filt) {
  for (int j = threadIdx.x; j < LAS_STRIP; j += 256) {
    const int t = t0 - LAS_HALO + j;
    s_strip[j] = (awp_row && t >= 0 && t < T) ? awp_row[t] : 0.f;
  }
  for (int j = threadIdx.x; j < LAS_C * LAS_K; j += 256) s_filt[j] = filt[j];
}

__device__ __forceinline__ void las_feat(const float* s_strip, const float* s_filt, float* s_feat) {
  for (int o = threadIdx.x; o < LAS_TT * LAS_C; o += 256) {
    const int tt = o / LAS_C, c = o % LAS_C;
    float acc = 0.f;
    for (int k = 0; k < LAS_K; ++k) acc += s_filt[c * LAS_K + k] * s_strip[tt + k];
    s_feat[o] = acc;
  }
}

// the lane's 8 channels of one frame's tanh image
template <typename T>
__device__ __forceinline__ void las_th8(const T* __restrict__ pk8, const float (&pqb)[8], const float (&wc)[8][LAS_C],
                                        const float* feat_t, float (&th)[8]) {
  float v[8], f[LAS_C];
  load8<T>(pk8, v);
#pragma unroll
  for (int c = 0; c < LAS_C; ++c) f[c] = feat_t[c];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float x = v[e] + pqb[e];
#pragma unroll
    for (int c = 0; c < LAS_C; ++c) x += wc[e][c] * f[c];
    th[e] = tanh_t<T>(x);
  }
}

template <typename T>
__device__ __forceinline__ void las_lane_params(const emoasr_las_attend_t& a, int b, int a0, float (&pqb)[8], float (&wc)[8][LAS_C],
                                                float (&ws)[8]) {
  load8<T>(static_cast<const T*>(a.pq) + (long)b * a.A + a0, pqb);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    pqb[e] += a.b_conv[a0 + e];
    ws[e] = a.w_score[a0 + e];
#pragma unroll
    for (int c = 0; c < LAS_C; ++c) wc[e][c] = a.w_conv[(a0 + e) * LAS_C + c];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void las_score_kernel(const emoasr_las_attend_t a) {
  __shared__ float s_strip[LAS_STRIP], s_filt[LAS_C * LAS_K], s_feat[LAS_TT * LAS_C];
  const int b = blockIdx.y, t0 = blockIdx.x * LAS_TT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = a.elens ? min(a.elens[b], a.T) : a.T;
  if (t0 >= len) {   // a wholly masked tile (block-uniform)
    for (int tt = threadIdx.x; tt < LAS_TT && t0 + tt < a.T; tt += 256) a.scores[(long)b * a.T + t0 + tt] = -FLT_MAX;
    return;
  }
  las_stage(a.aw_prev ? a.aw_prev + (long)b * a.T : nullptr, a.filt, a.T, t0, s_strip, s_filt);
  __syncthreads();
  las_feat(s_strip, s_filt, s_feat);
  __syncthreads();
  const int a0 = lane * 8;
  const bool act = a0 < a.A;
  float pqb[8], wc[8][LAS_C], ws[8];
  if (act) las_lane_params<T>(a, b, a0, pqb, wc, ws);
  const T* pk = static_cast<const T*>(a.pk) + (long)b * a.pk_bstride;
  for (int tt = wave; tt < LAS_TT; tt += 4) {
    const int t = t0 + tt;
    if (t >= a.T) break;
    if (t >= len) {
      if (lane == 0) a.scores[(long)b * a.T + t] = -FLT_MAX;
      continue;
    }
    float part = 0.f;
    if (act) {
      float th[8];
      las_th8<T>(pk + (long)t * a.A + a0, pqb, wc, s_feat + tt * LAS_C, th);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += ws[e] * th[e];
    }
    part = wave_sum(part);
    if (lane == 0) a.scores[(long)b * a.T + t] = part;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void las_ctx_kernel(const emoasr_las_attend_t a) {
  __shared__ float red[16];
  __shared__ float s_acc[32][LAS_CTX_COLS + 1];
  const int b = blockIdx.y;
  const float* sc = a.scores + (long)b * a.T;
  float m = -FLT_MAX;
  for (int t = threadIdx.x; t < a.T; t += 256) m = fmaxf(m, sc[t]);
  m = block_max(m, red);
  float s = 0.f;
  for (int t = threadIdx.x; t < a.T; t += 256) s += exp_t<T>(sc[t] - m);
  s = block_sum(s, red);
  const float inv = 1.f / s;
  const int dg = threadIdx.x & 7, tl = threadIdx.x >> 3;
  const int d0 = blockIdx.x * LAS_CTX_COLS + dg * 8;
  const T* eo = static_cast<const T*>(a.eouts) + (long)b * a.eo_bstride;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = tl; t < a.T; t += 32) {
    const float w = exp_t<T>(sc[t] - m) * inv * dropout_scale(a.seed, las_idx(a, b, t), a.drop_p);
    if (blockIdx.x == 0 && dg == 0) a.aw[(long)b * a.T + t] = w;
    if (d0 < a.D && w != 0.f) {
      float v[8];
      load8<T>(eo + (long)t * a.D + d0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w * v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) s_acc[tl][dg * 8 + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < LAS_CTX_COLS) {
    float t = 0.f;
    for (int r = 0; r < 32; ++r) t += s_acc[r][threadIdx.x];
    const int d = blockIdx.x * LAS_CTX_COLS + threadIdx.x;
    if (d < a.D) static_cast<T*>(a.ctx)[(long)b * a.ctx_ld + d] = from_f32<T>(t);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.lse) a.lse[b] = m + logf(s);
}

// dynamic LDS of the backward, in floats: strip | filter | feat | dfeat | red (16: four doubles, 8-byte aligned) | dctx [D] | acc [12][A]
__host__ __device__ inline int las_bwd_lds_floats(int A, int D) {
  return LAS_STRIP + LAS_C * LAS_K + 2 * LAS_TT * LAS_C + 16 + D + (2 + LAS_C) * A;
}

template <typename T>
__global__ __launch_bounds__(256) void las_attend_bwd_kernel(const emoasr_las_attend_t a) {
  extern __shared__ float las_lds[];
  float* s_strip = las_lds;
  float* s_filt = s_strip + LAS_STRIP;
  float* s_feat = s_filt + LAS_C * LAS_K;
  float* s_dfeat = s_feat + LAS_TT * LAS_C;
  float* s_red = s_dfeat + LAS_TT * LAS_C;
  float* s_dctx = s_red + 16;
  float* s_acc = s_dctx + a.D;   // [0]: d w_score, [1]: sum_t dpre (d query projection, d b_conv), [2 + c]: d W_conv[:, c]
  const int b = blockIdx.y, t0 = blockIdx.x * LAS_TT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int len = a.elens ? min(a.elens[b], a.T) : a.T;
  if (t0 >= len) return;   // masked frames carry no weight: nothing flows through them (block-uniform)
  const float* awd = a.aw + (long)b * a.T;
  const float* dawn = a.daw ? a.daw + (long)b * a.T : nullptr;
  const T* dctx = static_cast<const T*>(a.dctx) + (long)b * a.dctx_ld;
  const T* ctx = static_cast<const T*>(a.ctx) + (long)b * a.ctx_ld;
  las_stage(a.aw_prev ? a.aw_prev + (long)b * a.T : nullptr, a.filt, a.T, t0, s_strip, s_filt);
  for (int d = threadIdx.x; d < a.D; d += 256) s_dctx[d] = to_f32(dctx[d]);
  for (int i = threadIdx.x; i < LAS_TT * LAS_C; i += 256) s_dfeat[i] = 0.f;
  for (int i = threadIdx.x; i < (2 + LAS_C) * a.A; i += 256) s_acc[i] = 0.f;
  // S = sum_s aw[s] daw[s] = awd . dawd_next + dctx . ctx
  // (this sum and dctx . eouts[t] below cancel in the soft-max's gradient -- entirely at T = 1 -- so both are formed in f64)
  double sp = 0.0;
  if (dawn)
    for (int t = threadIdx.x; t < a.T; t += 256) sp += (double)awd[t] * (double)dawn[t];
  for (int d = threadIdx.x; d < a.D; d += 256) sp += (double)to_f32(dctx[d]) * (double)to_f32(ctx[d]);
  sp = wave_sum_f64(sp);
  double* s_red64 = reinterpret_cast<double*>(s_red);
  if (lane == 0) s_red64[wave] = sp;
  __syncthreads();
  const float S = (float)(s_red64[0] + s_red64[1] + s_red64[2] + s_red64[3]);
  las_feat(s_strip, s_filt, s_feat);
  __syncthreads();
  const int a0 = lane * 8;
  const bool act = a0 < a.A;
  float pqb[8], wc[8][LAS_C], ws[8];
  if (act) las_lane_params<T>(a, b, a0, pqb, wc, ws);
  float acc_ws[8], acc_sum[8], acc_wc[8][LAS_C];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc_ws[e] = acc_sum[e] = 0.f;
#pragma unroll
    for (int c = 0; c < LAS_C; ++c) acc_wc[e][c] = 0.f;
  }
  const T* pk = static_cast<const T*>(a.pk) + (long)b * a.pk_bstride;
  const T* eo = static_cast<const T*>(a.eouts) + (long)b * a.eo_bstride;
  const float lse = a.lse[b];
  for (int tt = wave; tt < LAS_TT; tt += 4) {
    const int t = t0 + tt;
    if (t >= len) break;   // (len <= T; wave-uniform)
    const float awd_t = awd[t];
    // the context sum's two gradients: dawd[t] = dctx . eouts[t], deouts[t] += awd[t] dctx
    double g = 0.0;
    for (int d0 = lane * 8; d0 < a.D; d0 += 512) {
      float v[8];
      load8<T>(eo + (long)t * a.D + d0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) g += (double)v[e] * (double)s_dctx[d0 + e];
      if (a.deouts && awd_t != 0.f) {
        float* o = a.deouts + ((long)b * a.T + t) * a.D + d0;
        float w[8];
        load8<float>(o, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] += awd_t * s_dctx[d0 + e];
        store8<float>(o, w);
      }
    }
    g = wave_sum_f64(g);
    const float dawd = (float)(g + (dawn ? (double)dawn[t] : 0.0));
    float th[8], part = 0.f;
    if (act) {
      las_th8<T>(pk + (long)t * a.A + a0, pqb, wc, s_feat + tt * LAS_C, th);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += ws[e] * th[e];
    }
    const float ev = wave_sum(part);
    const float aw_t = exp_t<T>(ev - lse);
    const float de = aw_t * (dawd * dropout_scale(a.seed, las_idx(a, b, t), a.drop_p) - S);
    float dfe[LAS_C];
#pragma unroll
    for (int c = 0; c < LAS_C; ++c) dfe[c] = 0.f;
    if (act) {
      float dp[8];
      const float* f = s_feat + tt * LAS_C;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dp[e] = de * ws[e] * (1.f - th[e] * th[e]);
        acc_ws[e] += de * th[e];
        acc_sum[e] += dp[e];
#pragma unroll
        for (int c = 0; c < LAS_C; ++c) {
          acc_wc[e][c] += dp[e] * f[c];
          dfe[c] += dp[e] * wc[e][c];
        }
      }
      float* o = a.dpk + ((long)b * a.T + t) * a.A + a0;
      float w[8];
      load8<float>(o, w);
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] += dp[e];
      store8<float>(o, w);
    }
#pragma unroll
    for (int c = 0; c < LAS_C; ++c) {
      dfe[c] = wave_sum(dfe[c]);
      if (lane == 0) s_dfeat[tt * LAS_C + c] = dfe[c];
    }
  }
  if (act) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      atomicAdd(&s_acc[a0 + e], acc_ws[e]);
      atomicAdd(&s_acc[a.A + a0 + e], acc_sum[e]);
#pragma unroll
      for (int c = 0; c < LAS_C; ++c) atomicAdd(&s_acc[(2 + c) * a.A + a0 + e], acc_wc[e][c]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (2 + LAS_C) * a.A; i += 256) {
    const float v = s_acc[i];
    if (v == 0.f) continue;
    const int k = i / a.A, ch = i % a.A;
    if (k == 0) {
      atomicAdd(a.dw_score + ch, v);
    } else if (k == 1) {
      atomicAdd(a.db_conv + ch, v);
      atomicAdd(a.dpq + (long)b * a.A + ch, v);
    } else {
      atomicAdd(a.dw_conv + ch * LAS_C + (k - 2), v);
    }
  }
  // through the convolution: the previous weights (transposed convolution over the tile's halo) and the filter
  if (a.daw_prev) {
    for (int j = threadIdx.x; j < LAS_STRIP; j += 256) {
      const int s = t0 - LAS_HALO + j;
      if (s < 0 || s >= a.T) continue;
      float acc = 0.f;
      for (int tt = 0; tt < LAS_TT; ++tt) {
        const int k = j - tt;   // s - t + 100
        if (k < 0 || k >= LAS_K) continue;
#pragma unroll
        for (int c = 0; c < LAS_C; ++c) acc += s_dfeat[tt * LAS_C + c] * s_filt[c * LAS_K + k];
      }
      if (acc != 0.f) atomicAdd(a.daw_prev + (long)b * a.T + s, acc);
    }
  }
  if (a.aw_prev) {
    for (int o = threadIdx.x; o < LAS_C * LAS_K; o += 256) {
      const int c = o / LAS_K, k = o % LAS_K;
      float acc = 0.f;
      for (int tt = 0; tt < LAS_TT; ++tt) acc += s_dfeat[tt * LAS_C + c] * s_strip[tt + k];
      if (acc != 0.f) atomicAdd(a.dfilt + o, acc);
    }
  }
}

__global__ __launch_bounds__(256) void las_dropmask_kernel(const emoasr_las_attend_t a, unsigned char* __restrict__ mask) {
  const long n = (long)a.B * a.T;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int b = (int)(i / a.T), t = (int)(i % a.T);
    mask[i] = (a.drop_p <= 0.f || dropout_keep(a.seed, las_idx(a, b, t), a.drop_p)) ? 1 : 0;
  }
}

int las_check(const emoasr_las_attend_t* a, const char* who) {
  EMO_CHECK(a && a->B > 0 && a->T > 0, "%s: B and T must be positive", who);
  EMO_CHECK(a->A > 0 && a->A % 8 == 0 && a->A <= LAS_MAX_A, "%s: attn_dim A=%d must be a multiple of 8, at most %d", who, a->A,
            LAS_MAX_A);
  EMO_CHECK(a->D > 0 && a->D % 8 == 0, "%s: enc_hidden_size D=%d must be a multiple of 8", who, a->D);
  EMO_CHECK(a->B <= 65535, "%s: B=%d rows exceed the grid", who, a->B);
  EMO_CHECK(a->pk && a->pq && a->filt && a->w_conv && a->b_conv && a->w_score && a->eouts, "%s: NULL operand", who);
  EMO_CHECK(a->pk_bstride == 0 || a->pk_bstride >= (long)a->T * a->A, "%s: pk_bstride", who);
  EMO_CHECK(a->eo_bstride == 0 || a->eo_bstride >= (long)a->T * a->D, "%s: eo_bstride", who);
  EMO_CHECK(a->drop_p >= 0.f && a->drop_p < 1.f, "%s: drop_p=%f", who, (double)a->drop_p);
  EMO_CHECK(a->aw && a->ctx && a->ctx_ld >= a->D && a->ctx_ld % 8 == 0, "%s: aw / ctx (ctx_ld=%ld)", who, a->ctx_ld);
  return 0;
}

}  // namespace

extern "C" int emoasr_las_attend_fwd(int dtype, const emoasr_las_attend_t* a, void* stream) {
  if (las_check(a, "las_attend_fwd")) return 1;
  EMO_CHECK(a->scores, "las_attend_fwd: the score scratch is NULL");
  hipStream_t s = (hipStream_t)stream;
  const dim3 g1(cdiv(a->T, LAS_TT), a->B), g2(cdiv(a->D, LAS_CTX_COLS), a->B);
  EMO_DISPATCH(dtype, (las_score_kernel<T><<<g1, 256, 0, s>>>(*a)));
  EMO_LAUNCH_CHECK();
  EMO_DISPATCH(dtype, (las_ctx_kernel<T><<<g2, 256, 0, s>>>(*a)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_las_attend_bwd(int dtype, const emoasr_las_attend_t* a, void* stream) {
  if (las_check(a, "las_attend_bwd")) return 1;
  EMO_CHECK(a->lse && a->dctx && a->dctx_ld >= a->D && a->dctx_ld % 8 == 0, "las_attend_bwd: lse / dctx (dctx_ld=%ld)", a->dctx_ld);
  EMO_CHECK(a->dpq && a->dpk && a->dw_score && a->dw_conv && a->db_conv && a->dfilt, "las_attend_bwd: NULL gradient buffer");
  EMO_CHECK(a->pk_bstride == (long)a->T * a->A, "las_attend_bwd: the key projection must be dense [B,T,A]");
  const size_t lds = sizeof(float) * (size_t)las_bwd_lds_floats(a->A, a->D);
  EMO_CHECK(lds <= 64 * 1024, "las_attend_bwd: A=%d, D=%d need %zu bytes of LDS (64 KB per block)", a->A, a->D, lds);
  const dim3 g(cdiv(a->T, LAS_TT), a->B);
  EMO_DISPATCH(dtype, (las_attend_bwd_kernel<T><<<g, 256, lds, (hipStream_t)stream>>>(*a)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_las_dropmask(const emoasr_las_attend_t* a, unsigned char* mask, void* stream) {
  EMO_CHECK(a && a->B > 0 && a->T > 0 && mask, "las_dropmask: B, T, mask");
  const long n = (long)a->B * a->T;
  const int grid = (int)std::min<long>((n + 255) / 256, 4096);
  las_dropmask_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(*a, mask);
  EMO_LAUNCH_CHECK();
  return 0;
}
