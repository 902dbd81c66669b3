// Pieces shared by the large-tile kernels (gemm_big.hip: NT products, gemm_big_tn.hip: TN products): LDS-DMA staging, counted
// waits on it, and the XCD-contiguous block order.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void* lds_void_ptr;

// block pid of nblk -> position in a list dealt to the eight XCDs in contiguous ranges (the hardware hands block i to XCD i % 8)
__device__ __forceinline__ int xcd_remap_big(int pid, int nblk) {
  const int per = nblk / 8, rem = nblk - per * 8;
  const int x = pid % 8, slot = pid / 8;
  return x * per + min(x, rem) + slot;
}

// 16 bytes per lane from a buffer straight into LDS: lane l lands at lds + 16 l (lds wave-uniform); an offset the descriptor's
// bounds check rejects lands zeros
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds, unsigned voff, unsigned soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_ptr)lds, 16, voff, soff, 0, 0);
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  static_assert(N == 8 || N == 6 || N == 4 || N == 3 || N == 2, "wait_vmcnt: unexpected piece count");
}
