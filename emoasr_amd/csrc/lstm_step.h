// Device code shared by the slot-addressed single-step LSTM kernels: the transducer beam search's round (csrc/rnnt_beam.hip) and the
// RNN LM's shallow-fusion step (csrc/rnnlm.hip).  A handful of hypotheses against a whole weight matrix: the weights are streamed
// once, the hypotheses' input rows sit in LDS.
#pragma once
#include "common.h"

namespace {

template <typename T> __device__ __forceinline__ float rnd(float x) { return to_f32(from_f32<T>(x)); }

// acc[i] += sum_e w[k0 + e] * x_i[k0 + e] for this lane's 16-byte pieces of one weight row, every hypothesis i < nb.
// xs: f32 [NB][ldx] in LDS.  8 lanes share a row (sub = lane's piece index): pieces k0 = sub * VEC, + 8 * VEC, ...
template <typename T, int NB>
__device__ __forceinline__ void row_dots(const T* __restrict__ w, int K, const float* __restrict__ xs, int ldx, int nb, int sub,
                                         float (&acc)[NB]) {
  constexpr int VEC = 16 / sizeof(T);
  for (int k = sub * VEC; k < K; k += 8 * VEC) {
    float wv[VEC];
    if constexpr (sizeof(T) == 2) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(w + k);
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[e] = (float)v[e];
    } else {
      const f32x4 v = *reinterpret_cast<const f32x4*>(w + k);
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[e] = v[e];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      if (i < nb) {
        const float* x = xs + i * ldx + k;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += wv[e] * x[e];
        acc[i] += s;
      }
    }
  }
}
__device__ __forceinline__ float group_sum8(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  return v;
}

typedef __attribute__((ext_vector_type(4))) float f32x4_;
__device__ __forceinline__ f32x4_ rows16_dot(const bf16* __restrict__ wrow0, long ldw, int K, const bf16* __restrict__ xs, int ldxs,
                                             int lane) {
  // wrow0: first of the wave's 16 rows; lane <-> (row lane & 15, k piece 8 * (lane >> 4)) of each 32-wide k step
  const bf16* wp = wrow0 + (long)(lane & 15) * ldw + 8 * (lane >> 4);
  const bf16* xp = xs + (lane & 15) * ldxs + 8 * (lane >> 4);
  f32x4_ acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int k = 0; k < K; k += 32) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(wp + k);
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(xp + k);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
  return acc;   // acc[r] = D[row 4 * (lane >> 4) + r][hypothesis lane & 15]
}

}  // namespace
