// The Gumbel(0, 1) variate behind emoasr_gumbel_noise / emoasr_sample_rows (electra.hip) and the sampling epilogue of the large-tile
// product (gemm_big.hip: emoasr_ce_head_sample_fwd): one device function, so that every sampler draws the same noise for the same
// (seed, row, column).
#pragma once
#include "common.h"

// Gumbel(0, 1) variate of element idx: k = 24-bit counter hash, u = (k + 0.5) * 2^-24 in (0, 1), g = -log(-log(u)).
// k + 0.5 has 25 significant bits: for u >= 0.5 the complement 1 - u = (2^24 - 1 - k + 0.5) * 2^-24 is formed instead (exact in
// f32) and -log(u) = -log1p(-(1 - u)), so no u rounds to 1 and every g is finite: -2.86 < g < 17.4.
__device__ __forceinline__ float gumbel_of(uint64_t seed, uint64_t idx) {
  const uint32_t k = dropout_hash(seed, idx) & 0xFFFFFFu;
  float e;
  if (k < 0x800000u) {
    e = -logf(((float)k + 0.5f) * 5.9604644775390625e-8f);
  } else {
    e = -log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 5.9604644775390625e-8f));
  }
  return -logf(e);
}
