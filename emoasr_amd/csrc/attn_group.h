// The grouped single-query cross-attention of the batched searches, ONE copy of its arithmetic for
//   * emoasr_attn_step_group (csrc/decode_batch.hip): a workgroup serves the W rows of one search against that search's memory;
//   * emoasr_attn_step_cells (csrc/decode_grid.hip): a workgroup serves up to 32 rows of consecutive searches of one utterance.
// A row's bits depend on its own query and on the memory's tiles counted from the memory's first row only: not on WB, not on the
// other rows of the workgroup (no reduction crosses queries; TK depends on DK alone).
#pragma once
#include <math.h>
#include "common.h"

namespace {

constexpr int G_MAXW = 32;    // queries of a group
constexpr int G_THREADS = 256;

template <typename T> struct Chunk16;   // 16 bytes of a K / V row
template <> struct Chunk16<float> {
  static constexpr int N = 4;
  f32x4 v;
  __device__ __forceinline__ float get(int i) const { return v[i]; }
  __device__ __forceinline__ void zero() { v = f32x4{0.f, 0.f, 0.f, 0.f}; }
};
template <> struct Chunk16<bf16> {
  static constexpr int N = 8;
  bf16x8 v;
  __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
  __device__ __forceinline__ void zero() {
    for (int i = 0; i < 8; ++i) v[i] = (bf16)0.f;
  }
};

// the WB / (DK, TK) dispatch of both entry points: EMO_ATTN_GROUP_LAUNCH(DK, TK, WB) is the caller's launch statement
#define EMO_ATTN_GROUP_CASE(DK, TK, W_)                         \
  case DK:                                                      \
    if ((W_) <= 8) EMO_ATTN_GROUP_LAUNCH(DK, TK, 8);            \
    else if ((W_) <= 16) EMO_ATTN_GROUP_LAUNCH(DK, TK, 16);     \
    else if ((W_) <= 24) EMO_ATTN_GROUP_LAUNCH(DK, TK, 24);     \
    else EMO_ATTN_GROUP_LAUNCH(DK, TK, 32);                     \
    break;

}  // namespace
