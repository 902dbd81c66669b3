// Fused kernels of the Conformer convolution module (asr/modeling/conformer.py:98-143), bf16, channels-last [B, T, C]:
//
//   forward   GLU -> depthwise Conv1d(k <= 31) -> BatchNorm partial statistics                  (was 2 launches)
//   backward  BatchNorm/Swish input gradient -> depthwise data gradient -> GLU backward,
//             + the depthwise weight-gradient partial sums                                       (was 4 launches)
//
// The element-wise kernels they replace moved every intermediate through HBM ([M, C] each: GLU output, BatchNorm input
// gradient, depthwise data gradient).  Here a workgroup of 256 threads x 256 channels walks a STRIP of up to S consecutive
// 32-frame tiles of one utterance.  Once per strip it reads the depthwise taps coalesced through LDS into registers
// (per-thread reads of w[ch][j] are 64 cache lines per wave-instruction) and, in the backward, puts the per-channel BatchNorm
// constants into LDS.  The staged rows -- the upstream element-wise function computed on the way in, 16-byte loads -- live in
// 64-row LDS rings: the first tile stages its 62 rows (tile + 15 halo rows on each side), every further tile only its 32 new
// rows, so the halo is staged once per strip and not once per tile (1.97-2.00 x the batch's rows at S = 1, 1.33-1.38 x at
// S = 3 for the stacked shapes of bench.py), and the sigmoids of the GLU follow the rows.  Every thread then takes the window
// of its two channels from the ring.  The arithmetic, its order and every rounding to bf16 are those of the separate kernels
// (convmodule.hip, elementwise.hip): c, the BatchNorm partials (one pair per 32-frame tile at the tile's table position) and
// dg are bit-identical to the unfused sequence for every S.  The weight-gradient sums stay in registers across the strip: the
// dense entry point flushes them per tile (the unfused kernel's table: bit-identical dw / dbias BELOW 1024 TILES, B cdiv(T, 32)
// < 1024 -- from 1024 rows on emo_dwconv_bwd_w_reduce folds the table in four slices that meet in float atomics, where
// emoasr_dwconv_bwd_w always folds in one: dw / dbias are then the same sums in another order, within the order-independent f32
// bound of an f64 reference and not run-to-run deterministic; measured at 32 x 1024 frames, tests/test_conv_kernels_gpu.py), the
// stacked one per strip into a compact table with one row per live strip -- no zero rows for the grid's empty corners, under
// 1024 rows for the benchmark's steps, so emo_dwconv_bwd_w_reduce runs as one slice without float atomics (run-to-run
// deterministic).
// S: option "conv_strip" (strip_tiles below).  Step of bench.py, parent 25.02 ms: S = 1 24.71, 2 24.74, 3 24.63, 4 24.63,
// 8 25.40, the rule 24.66 (profiles/conv_strip_step.txt); per-kernel times not measured yet.
// Registers (gfx950): backward 208, forward 209 (GLU) / 196, no scratch; 70 KB / 48 KB LDS: two workgroups per CU.
#include <algorithm>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int CF_TT = 32;     // output frames per tile (= DW_TT of convmodule.hip: same BatchNorm / weight-gradient partial tables)
constexpr int CF_MAXK = 31;
constexpr int CF_CB = 256;                     // channels (= threads) per workgroup (128: 2-3 workgroups per CU, measured
                                              // 10 % slower: twice the weight staging and barriers per channel)
constexpr int CF_ROWS_P = 64;                 // rows of an LDS ring (>= 32 + 30, a power of two; staged 32 at a time in 4 sweeps of 8)

// Work split of the compute phases (both kernels): a thread owns TWO adjacent channels (packed f32x2 multiplies and adds:
// half the VALU instructions of one channel per thread) and one HALF of the tile -- 16 of the 32 output frames of a
// convolution, or 16 of the (up to) 31 taps of the weight gradient, whose sums over the 32 frames then keep the frame order
// of the unfused kernel.  Every tap is ONE fused multiply-add (emo_mac2 of common.h, v_pk_fma_f32), as in the kernels these
// replace (emo_mac): round 4 -- the two kernels are VALU-bound, the stencils were half of their instructions.
typedef __attribute__((ext_vector_type(2))) float f2;
__device__ __forceinline__ f2 unpack2(unsigned u) { return f2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }
__device__ __forceinline__ unsigned pack2(f2 v) {
  const bf16 lo = (bf16)v[0], hi = (bf16)v[1];
  return (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
}
__device__ __forceinline__ unsigned lds_pair(const bf16* base, int row, int pair) {
  return *reinterpret_cast<const unsigned*>(base + row * CF_CB + 2 * pair);
}

// ---- the strip walk (both kernels) --------------------------------------------------------------------------------
// A workgroup owns up to S consecutive 32-frame tiles of ONE utterance.  The staged rows live in 64-row LDS rings: the row of
// frame t sits in slot (t + pad) & 63 -- u = t + pad >= 0 is the "ring row" below.  A tile at t0 reads ring rows t0 .. t0 + 31 +
// 2 pad (62 of the 64 slots for K = 31).  The strip's first tile stages all 64 slots (zeros where the tile has no use for the
// row, as the one-tile kernels did); every further tile stages only its 32 NEW rows t0 + 2 pad .. t0 + 2 pad + 31, which land on
// the slots of the previous tile's first rows, so one barrier separates a tile's stencil reads from the next tile's staging.
// Slots a tile does not own hold stale rows of the same utterance (the one-tile kernels held zeros there); they only meet zero
// taps (K < 31) or sums that are never stored, so finite inputs give the same bits.  A stale row that holds Inf / NaN turns
// 0 * Inf into a NaN within pad frames of it, where the one-tile kernels kept those frames finite.
// Zeros outside [0, Tn) are Conv1d's padding: every staged row is bounds-checked against its own utterance.
__device__ __forceinline__ int ring_row(int u) { return (u & (CF_ROWS_P - 1)) * CF_CB; }

// ---- forward: c[b,t,ch] = bias[ch] + sum_j w[ch,j] * z[b, t + j - pad, ch],  z = GLU(g) = g[:, :C] * sigmoid(g[:, C:]) ----
// GLU = false: x is the [B, T, C] input itself (the plain depthwise convolution; flip = 1 gives the data gradient).
// S: tiles per strip.  The BatchNorm partials stay one (sum, m2) pair per 32-frame tile at the table position of the tile.
template <bool GLU>
__global__ __launch_bounds__(CF_CB) void cf_dwconv_kernel(int Tn, int C, int K, const bf16* __restrict__ x,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        bf16* __restrict__ y, int flip, float* __restrict__ part, int S,
                                                        const RowSegs sg) {
  __shared__ __attribute__((aligned(16))) bf16 zs[CF_ROWS_P * CF_CB];  // the ring
  __shared__ __attribute__((aligned(16))) bf16 os[CF_TT * CF_CB];    // the output tile (stored rows, BatchNorm partials)
  const int tid = threadIdx.x;
  const int cb = blockIdx.y * CF_CB;                 // first channel of this workgroup
  const int ldx = GLU ? 2 * C : C;
  int b = blockIdx.z;
  if (sg.n > 1) {   // stacked micro-batches: this utterance's segment (own padded length, own partial-statistics table)
    const int si = rowsegs_of_utt(sg, b);
    Tn = sg.T[si];
    x += sg.row[si] * ldx;
    y += sg.row[si] * C;
    if (part) part += sg.part[si];
    b -= sg.b0[si];
  }
  const int nx = (Tn + CF_TT - 1) / CF_TT;           // tiles of this utterance
  const int tile0 = blockIdx.x * S;
  if (tile0 >= nx) return;                           // (the grid follows the longest segment)
  const int ntile = min(S, nx - tile0);
  const int pad = (K - 1) / 2;
  const int nch = min(CF_CB, C - cb);                // channels present (multiple of 8)
  // ---- this thread's taps, once per strip: w[ch][K] is read coalesced through LDS (per-thread reads of w[ch * K + j] are 64
  //      different cache lines per wave-instruction: 62 such gathers per thread cost more than the convolution) ----
  const int pr = tid & (CF_CB / 2 - 1), half = tid / (CF_CB / 2);
  f2 wr[CF_MAXK];
  {
    float* wsm = reinterpret_cast<float*>(zs);   // CF_CB * K floats <= the bytes of zs
    for (int idx = tid; idx < nch * K; idx += CF_CB) wsm[idx] = w[(long)cb * K + idx];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CF_MAXK; ++j) {
      const int jj = flip ? K - 1 - j : j;
      wr[j] = (j < K && 2 * pr < nch) ? f2{wsm[(2 * pr) * K + jj], wsm[(2 * pr + 1) * K + jj]} : f2{0.f, 0.f};
    }
    __syncthreads();
  }
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(x + (long)b * Tn * ldx);
  const int ch8 = (tid & (CF_CB / 8 - 1)) * 8;
  const int c0 = cb + 2 * pr;
  const f2 bv = (bias && 2 * pr < nch) ? f2{bias[c0], bias[c0 + 1]} : f2{0.f, 0.f};
  // 32 ring rows from u0 on (zeros outside the utterance and past the rows tile t0 reads); a thread's loads are all issued
  // before the first is used
  auto stage32 = [&](int t0, int u0) {
    Vec16<bf16> sa[CF_TT / 8], sb[GLU ? CF_TT / 8 : 1];
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int u = u0 + tid / (CF_CB / 8) + it * 8;
      const int t = u - pad;
      const bool ok = u - t0 < CF_TT + K - 1 && t >= 0 && t < Tn && ch8 < nch;
      const unsigned off = ok ? (unsigned)(((long)t * ldx + cb + ch8) * 2) : EMO_OOB;
      sa[it] = buf_load16<bf16>(rs, off);
      if constexpr (GLU) sb[it] = buf_load16<bf16>(rs, ok ? off + (unsigned)(C * 2) : EMO_OOB);
    }
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int u = u0 + tid / (CF_CB / 8) + it * 8;
      Vec16<bf16> a = sa[it];
      if constexpr (GLU) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a.v[e] = (bf16)((float)a.v[e] * sigmoidf_((float)sb[it].v[e]));
      }
      store16(&zs[ring_row(u) + ch8], a);
    }
  };
  for (int k = 0; k < ntile; ++k) {
    const int tile = tile0 + k, t0 = tile * CF_TT;
    if (k == 0) {
      stage32(t0, t0);
      stage32(t0, t0 + CF_TT);
    } else {
      stage32(t0, t0 + 2 * pad);   // (the barrier after the previous tile's stencils is the one behind its output tile)
    }
    __syncthreads();
    // ---- 16 output frames x 2 channels per thread ----
    if (2 * pr < nch) {
      f2 win[CF_TT / 2 + CF_MAXK - 1];
#pragma unroll
      for (int i = 0; i < CF_TT / 2 + CF_MAXK - 1; ++i) win[i] = unpack2(*reinterpret_cast<const unsigned*>(zs + ring_row(t0 + half * (CF_TT / 2) + i) + 2 * pr));
#pragma unroll
      for (int i = 0; i < CF_TT / 2; ++i) {
        f2 acc = bv;
#pragma unroll
        for (int j = 0; j < CF_MAXK; ++j) acc = emo_mac2(wr[j], win[i + j], acc);
        *reinterpret_cast<unsigned*>(os + (half * (CF_TT / 2) + i) * CF_CB + 2 * pr) = pack2(acc);
      }
    }
    __syncthreads();
    // ---- full-row stores of the tile; BatchNorm partials per channel in frame order ----
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int row = tid / (CF_CB / 8) + it * 8;
      if (t0 + row < Tn && ch8 < nch)
        *reinterpret_cast<bf16x8*>(y + ((long)b * Tn + t0 + row) * C + cb + ch8) = *reinterpret_cast<const bf16x8*>(os + row * CF_CB + ch8);
    }
    if (part && tid < nch) {
      float out[CF_TT];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < CF_TT; ++i) {
        out[i] = t0 + i < Tn ? (float)os[i * CF_CB + tid] : 0.f;
        s += out[i];
      }
      const int n = min(CF_TT, Tn - t0);
      const float mb = s / n;
      float m2 = 0.f;
#pragma unroll
      for (int i = 0; i < CF_TT; ++i) {
        const float d = out[i] - mb;
        m2 += i < n ? d * d : 0.f;
      }
      float* p = part + ((long)b * nx + tile) * 2 * C + cb + tid;
      p[0] = s;
      p[C] = m2;
    }
    // (the next tile's staging overwrites ring rows this tile's stencils have read -- all of them before the barrier above -- and
    // its output tile is written behind the next barrier, which every thread reaches after these stores)
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------
//   dbn = ds * swish'(gamma * xhat + beta),  dc = gamma * invstd * (dbn - mean(dbn) - xhat * mean(dbn * xhat))   (bf16)
//   dz[t] = sum_j w[K-1-j] * dc[t + j - pad]                                                                      (bf16)
//   dg[:, :C] = dz * sigmoid(gb),  dg[:, C:] = dz * ga * sigmoid(gb) * (1 - sigmoid(gb))
//   wpart[row][j][ch] = sum_t dc[t] * z[t + j - pad],  wpart[row][K][ch] = sum_t dc[t]                (z = GLU(g), bf16)
// tot: [2][C] means from the BatchNorm fold (emoasr_bn_swish_bwd_sums).
// The weight-gradient sums stay in registers and are flushed
//   per_tile = 1: after every tile, to row (utterance * tiles + tile): the [tile][K+1][C] table of the unfused kernel, so the
//                 reduce adds the same numbers in the same order (dense entry point; bit-identical dw / dbias below 1024 tiles,
//                 where the reduce is one slice);
//   per_tile = 0: once per strip, in frame order over the strip's tiles, to a COMPACT table: row = strips of the earlier
//                 segments + utterance-in-segment * strips-per-utterance + strip.  Only live strips have a row; a workgroup
//                 without frames writes nothing.
constexpr int CF_BWD_LDS = 2 * CF_ROWS_P * CF_CB * 2 + 6 * CF_CB * 4;   // the two rings + the per-channel constants
__global__ __launch_bounds__(CF_CB, 2) void cf_conv_bwd_kernel(int Tn, int C, int K, const bf16* __restrict__ ds,
                                                             const bf16* __restrict__ cv, const float* __restrict__ mean,
                                                             const float* __restrict__ var, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             const float* __restrict__ tot, const bf16* __restrict__ g,
                                                             const float* __restrict__ w, bf16* __restrict__ dg,
                                                             float* __restrict__ wpart, int S, int per_tile, const RowSegs sg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* dcs = reinterpret_cast<bf16*>(smem);                       // [64][CB] ring: BatchNorm input gradient
  bf16* zs = dcs + CF_ROWS_P * CF_CB;                                // [64][CB] ring: GLU output
  float* cst = reinterpret_cast<float*>(zs + CF_ROWS_P * CF_CB);     // [6][CB]  mean, invstd, gamma, beta, the two BatchNorm means
  // (the raw GLU halves of the tile's own frames are re-read from global memory in the GLU backward -- L2-resident, this
  // workgroup staged them microseconds ago; two more [32][CB] images would leave ONE workgroup per CU)
  const int tid = threadIdx.x;
  const int cb = blockIdx.y * CF_CB;
  const int nch = min(CF_CB, C - cb);
  int b = blockIdx.z;
  long row0 = 0;    // first row of this utterance in the partial table
  if (sg.n > 1) {   // stacked micro-batches: this utterance's segment (own padded length, batch statistics and means)
    const int si = rowsegs_of_utt(sg, b);
    for (int k = 0; k < 8; ++k)
      if (k < si) row0 += (long)(sg.b0[k + 1] - sg.b0[k]) * (((sg.T[k] + CF_TT - 1) / CF_TT + S - 1) / S);
    Tn = sg.T[si];
    ds += sg.row[si] * C; cv += sg.row[si] * C; g += sg.row[si] * 2 * C; dg += sg.row[si] * 2 * C;
    mean += (long)si * C; var += (long)si * C; tot += (long)si * 2 * C;
    b -= sg.b0[si];
  }
  const int nx = (Tn + CF_TT - 1) / CF_TT;
  const int tile0 = blockIdx.x * S;
  if (tile0 >= nx) return;   // (the grid follows the longest segment: no frames, and no row in the partial table)
  const int ntile = min(S, nx - tile0);
  row0 += per_tile ? (long)b * nx : (long)b * ((nx + S - 1) / S) + blockIdx.x;
  const int pad = (K - 1) / 2;
  const int ch8 = (tid & (CF_CB / 8 - 1)) * 8;
  const bool chok = ch8 < nch;
  const int pr = tid & (CF_CB / 2 - 1), half = __builtin_amdgcn_readfirstlane(tid / (CF_CB / 2));   // (wave-uniform: scalar row and tap offsets)
  // ---- once per strip: the per-channel constants into LDS, the flipped taps of this thread's two channels into registers
  //      (read coalesced through LDS, see cf_dwconv_kernel) ----
  {
    const int cc = cb + tid;
    const bool ok = tid < nch;
    cst[0 * CF_CB + tid] = ok ? mean[cc] : 0.f; cst[1 * CF_CB + tid] = ok ? rsqrtf(var[cc] + eps) : 0.f;
    cst[2 * CF_CB + tid] = ok ? gamma[cc] : 0.f; cst[3 * CF_CB + tid] = ok ? beta[cc] : 0.f;
    cst[4 * CF_CB + tid] = ok ? tot[cc] : 0.f; cst[5 * CF_CB + tid] = ok ? tot[C + cc] : 0.f;
  }
  f2 wr[CF_MAXK];
  {
    float* wsm = reinterpret_cast<float*>(smem);
    for (int idx = tid; idx < nch * K; idx += CF_CB) wsm[idx] = w[(long)cb * K + idx];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CF_MAXK; ++j)
      wr[j] = (j < K && 2 * pr < nch) ? f2{wsm[(2 * pr) * K + (K - 1 - j)], wsm[(2 * pr + 1) * K + (K - 1 - j)]} : f2{0.f, 0.f};
    __syncthreads();
  }
  const __amdgpu_buffer_rsrc_t rsd = make_rsrc(ds + (long)b * Tn * C), rsc = make_rsrc(cv + (long)b * Tn * C);
  const __amdgpu_buffer_rsrc_t rsg = make_rsrc(g + (long)b * Tn * 2 * C);
  // 32 ring rows from u0 on: z = GLU(g) and the BatchNorm input gradient (zeros outside the utterance and past the rows tile t0
  // reads)
  auto stage32 = [&](int t0, int u0) {
    Vec16<bf16> ga[CF_TT / 8], gb[CF_TT / 8], dvs[CF_TT / 8], yvs[CF_TT / 8];
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int u = u0 + tid / (CF_CB / 8) + it * 8;
      const int t = u - pad;
      const bool ok = u - t0 < CF_TT + K - 1 && t >= 0 && t < Tn && chok;
      const unsigned goff = ok ? (unsigned)(((long)t * 2 * C + cb + ch8) * 2) : EMO_OOB;
      ga[it] = buf_load16<bf16>(rsg, goff);
      gb[it] = buf_load16<bf16>(rsg, ok ? goff + (unsigned)(C * 2) : EMO_OOB);
    }
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int u = u0 + tid / (CF_CB / 8) + it * 8;
      Vec16<bf16> z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z.v[e] = (bf16)((float)ga[it].v[e] * sigmoidf_((float)gb[it].v[e]));
      store16(&zs[ring_row(u) + ch8], z);
    }
    // ... then the BatchNorm input gradient of the same rows
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int u = u0 + tid / (CF_CB / 8) + it * 8;
      const int t = u - pad;
      const bool ok = u - t0 < CF_TT + K - 1 && t >= 0 && t < Tn && chok;
      const unsigned off = ok ? (unsigned)(((long)t * C + cb + ch8) * 2) : EMO_OOB;
      dvs[it] = buf_load16<bf16>(rsd, off);
      yvs[it] = buf_load16<bf16>(rsc, off);
    }
    float mu[8], is[8], gm[8], bt[8], m1[8], m2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mu[j] = cst[0 * CF_CB + ch8 + j]; is[j] = cst[1 * CF_CB + ch8 + j]; gm[j] = cst[2 * CF_CB + ch8 + j];
      bt[j] = cst[3 * CF_CB + ch8 + j]; m1[j] = cst[4 * CF_CB + ch8 + j]; m2[j] = cst[5 * CF_CB + ch8 + j];
    }
#pragma unroll
    for (int it = 0; it < CF_TT / 8; ++it) {
      const int u = u0 + tid / (CF_CB / 8) + it * 8;
      const int t = u - pad;
      const bool ok = u - t0 < CF_TT + K - 1 && t >= 0 && t < Tn && chok;
      const Vec16<bf16> dv = dvs[it], yv = yvs[it];
      Vec16<bf16> o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = ((float)yv.v[e] - mu[e]) * is[e];
        const float dbn = (float)dv.v[e] * dswishf_(gm[e] * xh + bt[e]);
        o.v[e] = ok ? (bf16)(gm[e] * is[e] * (dbn - m1[e] - xh * m2[e])) : (bf16)0.f;
      }
      store16(&dcs[ring_row(u) + ch8], o);
    }
  };
  const bool active = 2 * pr < nch;
  const int c0 = cb + 2 * pr;
  // weight-gradient sums: 16 taps x 2 channels, over the frames in frame order
  constexpr int TAPS = (CF_MAXK + 1) / 2;   // 16
  const int j0 = half * TAPS;
  f2 acc[TAPS];
#pragma unroll
  for (int j = 0; j < TAPS; ++j) acc[j] = f2{0.f, 0.f};
  f2 sb = f2{0.f, 0.f};
  for (int k = 0; k < ntile; ++k) {
    const int t0 = (tile0 + k) * CF_TT;
    if (k == 0) {
      stage32(t0, t0);
      stage32(t0, t0 + CF_TT);
    } else {
      __syncthreads();             // the previous tile's stencil reads are done: its first rows' slots take the new rows
      stage32(t0, t0 + 2 * pad);
    }
    __syncthreads();
    if (active) {
    // ---- data gradient of the depthwise convolution + GLU backward: 16 frames x 2 channels ----
    {
      auto dcrow = [&](int i) { return unpack2(*reinterpret_cast<const unsigned*>(dcs + ring_row(t0 + half * (CF_TT / 2) + i) + 2 * pr)); };
      f2 dcw[CF_TT / 2 + CF_MAXK - 1];
#pragma unroll
      for (int i = 0; i < CF_MAXK - 1; ++i) dcw[i] = dcrow(i);
      bf16* dgb = dg + (long)b * Tn * 2 * C + c0;
#pragma unroll
      for (int i = 0; i < CF_TT / 2; ++i) {
        if (i % 8 == 0) {   // (the window slides 8 frames at a time: registers)
          if (i) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int e = 0; e < 8; ++e) dcw[CF_MAXK - 1 + i + e] = dcrow(CF_MAXK - 1 + i + e);
        }
        f2 a2 = f2{0.f, 0.f};
#pragma unroll
        for (int j = 0; j < CF_MAXK; ++j) a2 = emo_mac2(wr[j], dcw[i + j], a2);
        const f2 d = unpack2(pack2(a2));   // the data gradient is stored as bf16 by the unfused kernel
        const int fr = half * (CF_TT / 2) + i;
        const bool fok = t0 + fr < Tn;
        const bf16* gp = g + ((long)b * Tn + (fok ? t0 + fr : 0)) * 2 * C + c0;
        const f2 a = fok ? unpack2(*reinterpret_cast<const unsigned*>(gp)) : f2{0.f, 0.f};
        const f2 gt = fok ? unpack2(*reinterpret_cast<const unsigned*>(gp + C)) : f2{0.f, 0.f};
        const f2 sgm = f2{sigmoidf_(gt[0]), sigmoidf_(gt[1])};
        if (fok) {
          *reinterpret_cast<unsigned*>(dgb + (long)(t0 + fr) * 2 * C) = pack2(d * sgm);
          *reinterpret_cast<unsigned*>(dgb + (long)(t0 + fr) * 2 * C + C) = pack2(d * a * sgm * (f2{1.f, 1.f} - sgm));
        }
      }
    }
    // ---- weight-gradient sums of this tile's 32 frames (dc is zero past the utterance's end), 8 frames at a time: the
    //      window of z slides through registers, so the sums, the taps and the window fit beside each other ----
    {
      auto zrow = [&](int i) { return unpack2(*reinterpret_cast<const unsigned*>(zs + ring_row(t0 + j0 + i) + 2 * pr)); };
      f2 zw[CF_TT + TAPS - 1];   // ring rows t0 + j0 .. t0 + j0 + 46 (<= t0 + 62)
#pragma unroll
      for (int i = 0; i < TAPS - 1; ++i) zw[i] = zrow(i);
#pragma unroll
      for (int c = 0; c < CF_TT / 8; ++c) {
        f2 dcc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          zw[8 * c + TAPS - 1 + i] = zrow(8 * c + TAPS - 1 + i);
          dcc[i] = unpack2(*reinterpret_cast<const unsigned*>(dcs + ring_row(t0 + 8 * c + i + pad) + 2 * pr));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const f2 d = dcc[i];
          sb += d;
#pragma unroll
          for (int j = 0; j < TAPS; ++j) acc[j] = emo_mac2(d, zw[8 * c + i + j], acc[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (per_tile || k == ntile - 1) {
      float* p = wpart + (row0 + (per_tile ? tile0 + k : 0)) * (K + 1) * C + c0;
#pragma unroll
      for (int j = 0; j < TAPS; ++j) {
        if (j0 + j < K) *reinterpret_cast<f2*>(p + (long)(j0 + j) * C) = acc[j];
        acc[j] = f2{0.f, 0.f};
      }
      if (half == 0) *reinterpret_cast<f2*>(p + (long)K * C) = sb;
      sb = f2{0.f, 0.f};
    }
    }
  }
}

}  // namespace

int emo_dwconv_bwd_w_reduce(int nblk, int C, int K, const float* part, float* dw, float* dbias, hipStream_t s);  // convmodule.hip

// Tiles per strip (option "conv_strip"): n >= 1 forces n, 1 is the one-tile-per-workgroup schedule; 0 = the smallest S <= 8
// that brings the launch's live strips to at most two workgroups per CU (both kernels keep two resident; a longer strip
// stages fewer halo rows and writes fewer partial rows, a shorter one leaves no CU without work).
namespace {
long live_strips(int n, const int* B, const int* T, int S) {
  long r = 0;
  for (int i = 0; i < n; ++i) r += (long)B[i] * cdiv(cdiv(T[i], CF_TT), S);
  return r;
}
int strip_tiles(int n, const int* B, const int* T, int cy) {
  if (g_opt.conv_strip > 0) return g_opt.conv_strip;
  static int cus = 0;
  if (!cus) {
    int dev = 0, v = 0;
    cus = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  int S = 1;
  while (S < 8 && live_strips(n, B, T, S) * cy > 2L * cus) ++S;
  return S;
}
int bwd_lds_attr() {
  static bool done = false;
  if (!done) {
    hipError_t e = hipFuncSetAttribute((const void*)cf_conv_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CF_BWD_LDS);
    if (e != hipSuccess) { emo_set_error("hipFuncSetAttribute(%d): %s", CF_BWD_LDS, hipGetErrorString(e)); return 1; }
    done = true;
  }
  return 0;
}
}  // namespace

// c = depthwise_conv(GLU(g)) (+ per-block BatchNorm partial statistics when part != NULL, consumed by
// emoasr_bn_stats_finalize): conformer.py:126-131 without materialising the GLU output.  g: [B*T, 2C].
extern "C" int emoasr_glu_dwconv_fwd(int dtype, int B, int Tn, int C, int K, const void* g, const float* w,
                                     const float* bias, void* c, float* part, void* stream) {
  EMO_CHECK(dtype == EMO_BF16, "glu_dwconv_fwd: bf16 only");
  EMO_CHECK(K <= CF_MAXK && (K & 1) && C % 8 == 0, "glu_dwconv_fwd: K=%d (odd, <= %d), C=%d (multiple of 8)", K, CF_MAXK, C);
  EMO_CHECK((long)Tn * 2 * C * 2 < (1L << 32), "glu_dwconv_fwd: utterance larger than 4 GiB");
  if (B * Tn == 0) return 0;
  const int S = strip_tiles(1, &B, &Tn, cdiv(C, CF_CB));
  dim3 grid(cdiv(cdiv(Tn, CF_TT), S), cdiv(C, CF_CB), B);
  cf_dwconv_kernel<true><<<grid, CF_CB, 0, (hipStream_t)stream>>>(Tn, C, K, (const bf16*)g, w, bias, (bf16*)c, 0, part, S, RowSegs{});
  EMO_LAUNCH_CHECK();
  return 0;
}

// The LDS-staged depthwise convolution on a plain [B, T, C] input (flip = 1: its data gradient); called by
// emoasr_dwconv_fwd / _fwd_stats / _bwd_x for bf16.
int emo_dwconv_lds(int B, int Tn, int C, int K, const void* x, const float* w, const float* bias, void* y, int flip,
                   float* part, hipStream_t s) {
  const int S = strip_tiles(1, &B, &Tn, cdiv(C, CF_CB));
  dim3 grid(cdiv(cdiv(Tn, CF_TT), S), cdiv(C, CF_CB), B);
  cf_dwconv_kernel<false><<<grid, CF_CB, 0, s>>>(Tn, C, K, (const bf16*)x, w, bias, (bf16*)y, flip, part, S, RowSegs{});
  EMO_LAUNCH_CHECK();
  return 0;
}

// Backward of BatchNorm(training) -> Swish ... depthwise conv ... GLU in one launch, given the BatchNorm means of
// emoasr_bn_swish_bwd_sums in `tot`:  ds = gradient w.r.t. the Swish output, cv = the depthwise convolution's output,
// g = the GLU input [B*T, 2C]  ->  dg [B*T, 2C];  dw [C, K] and dbias [C] are accumulated into.
// scratch: emoasr_dwconv_bwd_w_scratch_floats(B, Tn, C, K) floats.
extern "C" int emoasr_conv_bwd_fused(int dtype, int B, int Tn, int C, int K, const void* ds, const void* cv,
                                     const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                                     const float* tot, const void* g, const float* w, void* dg, float* dw, float* dbias,
                                     float* scratch, void* stream) {
  EMO_CHECK(dtype == EMO_BF16, "conv_bwd_fused: bf16 only");
  EMO_CHECK(K <= CF_MAXK && (K & 1) && C % 8 == 0, "conv_bwd_fused: K=%d (odd, <= %d), C=%d (multiple of 8)", K, CF_MAXK, C);
  EMO_CHECK((long)Tn * 2 * C * 2 < (1L << 32), "conv_bwd_fused: utterance larger than 4 GiB");
  EMO_CHECK(scratch != nullptr && tot != nullptr, "conv_bwd_fused: scratch and tot are required");
  if (B * Tn == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (bwd_lds_attr()) return 1;
  // strips for the halo, but one partial row per TILE: the table of the unfused kernel, summed in its order
  const int S = strip_tiles(1, &B, &Tn, cdiv(C, CF_CB));
  dim3 grid(cdiv(cdiv(Tn, CF_TT), S), cdiv(C, CF_CB), B);
  cf_conv_bwd_kernel<<<grid, CF_CB, CF_BWD_LDS, s>>>(Tn, C, K, (const bf16*)ds, (const bf16*)cv, mean, var, gamma, beta, eps, tot,
                                                   (const bf16*)g, w, (bf16*)dg, scratch, S, 1, RowSegs{});
  EMO_LAUNCH_CHECK();
  return emo_dwconv_bwd_w_reduce(cdiv(Tn, CF_TT) * B, C, K, scratch, dw, dbias, s);
}

// ---- the convolution module's per-utterance part for STACKED micro-batches (emoasr_segments_t): every kernel takes all segments
// in one launch.  Same arithmetic as calling the entry points above once per segment, in order. -------------------------------
int emo_bn_stats_finalize_seg(const RowSegs& sg, int C, float* part, float* mean, float* var, float* running_mean,
                              float* running_var, float momentum, long long* nbt, hipStream_t s);                    // convmodule.hip
int emo_bn_swish_fwd_seg(const RowSegs& sg, int C, const void* y, const float* mean, const float* var, const float* gamma,
                         const float* beta, float eps, void* z, hipStream_t s);                                       // convmodule.hip
int emo_bn_swish_bwd_sums_seg(const RowSegs& sg, int C, const void* dz, const void* y, const float* mean, const float* var,
                              const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, float* scratch,
                              float** tot_out, hipStream_t s);                                                        // convmodule.hip

namespace {
bool row_segs(const emoasr_segments_t* seg, int C, RowSegs* out, int* tmax) {
  if (!seg || seg->n < 1 || seg->n > EMOASR_MAX_SEGMENTS) return false;
  RowSegs sg{};
  sg.n = seg->n;
  *tmax = 0;
  for (int i = 0; i < seg->n; ++i) {
    if (seg->B[i] <= 0 || seg->T[i] <= 0) return false;
    sg.b0[i + 1] = sg.b0[i] + seg->B[i];
    sg.T[i] = seg->T[i];
    sg.row[i + 1] = sg.row[i] + (long)seg->B[i] * seg->T[i];
    sg.part[i + 1] = sg.part[i] + emoasr_dwconv_stats_floats(seg->B[i], seg->T[i], C);
    sg.sums[i + 1] = sg.sums[i] + (emoasr_bn_swish_bwd_scratch_floats(seg->B[i] * seg->T[i], C) / (2 * C) - 1);
    *tmax = std::max(*tmax, seg->T[i]);
  }
  *out = sg;
  return true;
}
}  // namespace

// c = depthwise_conv(GLU(g)) per segment, BatchNorm batch statistics per segment (training: bmean / bvar [n, C], the running
// statistics updated once per segment in order; eval: the running statistics), z = Swish(BatchNorm(c)).  g [M, 2C], c / z [M, C],
// part: sum over the segments of emoasr_dwconv_stats_floats(B[s], T[s], C) floats.  conformer.py:126-133.
extern "C" int emoasr_conv_module_fwd_seg(int dtype, const emoasr_segments_t* seg, int C, int K, const void* g, const float* w,
                                          const float* bias, void* c, float* part, float* bmean, float* bvar, float* running_mean,
                                          float* running_var, float momentum, long long* num_batches_tracked, const float* gamma,
                                          const float* beta, float eps, void* z, int training, void* stream) {
  EMO_CHECK(dtype == EMO_BF16, "conv_module_fwd_seg: bf16 only");
  EMO_CHECK(K <= CF_MAXK && (K & 1) && C % 8 == 0, "conv_module_fwd_seg: K=%d (odd, <= %d), C=%d (multiple of 8)", K, CF_MAXK, C);
  RowSegs sg;
  int tmax = 0;
  EMO_CHECK(row_segs(seg, C, &sg, &tmax), "conv_module_fwd_seg: bad segment description");
  EMO_CHECK((long)tmax * 2 * C * 2 < (1L << 32) && sg.row[sg.n] * 2 * C * 2 < (1L << 46), "conv_module_fwd_seg: batch too large");
  EMO_CHECK(!training || (part && bmean && bvar), "conv_module_fwd_seg: training needs the BatchNorm buffers");
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes per row and channel: g (2) in, c out; c in, z out
  EmoTimerScope timer_(EMO_TIMER_CONV_MODULE, s, 0.0, 5.0 * (double)sg.row[sg.n] * C * 2.0);
  const int S = strip_tiles(seg->n, seg->B, seg->T, cdiv(C, CF_CB));
  dim3 grid(cdiv(cdiv(tmax, CF_TT), S), cdiv(C, CF_CB), sg.b0[sg.n]);
  cf_dwconv_kernel<true><<<grid, CF_CB, 0, s>>>(tmax, C, K, (const bf16*)g, w, bias, (bf16*)c, 0, training ? part : nullptr, S, sg);
  EMO_LAUNCH_CHECK();
  if (training) {
    if (emo_bn_stats_finalize_seg(sg, C, part, bmean, bvar, running_mean, running_var, momentum, num_batches_tracked, s)) return 1;
    return emo_bn_swish_fwd_seg(sg, C, c, bmean, bvar, gamma, beta, eps, z, s);
  }
  RowSegs one{};   // eval: the same (running) statistics for every row
  one.n = 1; one.b0[1] = sg.b0[sg.n]; one.row[1] = sg.row[sg.n];
  return emo_bn_swish_fwd_seg(one, C, c, running_mean, running_var, gamma, beta, eps, z, s);
}

// scratch of emoasr_conv_module_bwd_seg: which = 0 the BatchNorm partial sums + means (floats), 1 the depthwise weight-gradient
// partials (floats)
extern "C" long emoasr_conv_module_bwd_seg_scratch_floats(const emoasr_segments_t* seg, int C, int K, int which) {
  RowSegs sg;
  int tmax = 0;
  if (!row_segs(seg, C, &sg, &tmax)) return 0;
  if (which == 0) return (sg.sums[sg.n] + 2 * sg.n) * 2 * C;   // partial rows, the means, the raw sums
  return emoasr_dwconv_bwd_w_scratch_floats(sg.b0[sg.n], tmax, C, K);
}

// dz (gradient w.r.t. the Swish output) -> dg [M, 2C] through BatchNorm(training, per-segment statistics) / Swish, the depthwise
// convolution and the GLU; dgamma / dbeta / dw / dbias accumulated.  Autograd of conformer.py:126-133.
extern "C" int emoasr_conv_module_bwd_seg(int dtype, const emoasr_segments_t* seg, int C, int K, const void* dz, const void* c,
                                          const float* bmean, const float* bvar, const float* gamma, const float* beta, float eps,
                                          float* dgamma, float* dbeta, const void* g, const float* w, void* dg, float* dw,
                                          float* dbias, float* bn_scratch, float* dw_scratch, void* stream) {
  EMO_CHECK(dtype == EMO_BF16, "conv_module_bwd_seg: bf16 only");
  EMO_CHECK(K <= CF_MAXK && (K & 1) && C % 8 == 0, "conv_module_bwd_seg: K=%d (odd, <= %d), C=%d (multiple of 8)", K, CF_MAXK, C);
  EMO_CHECK(bn_scratch && dw_scratch, "conv_module_bwd_seg: scratch required");
  RowSegs sg;
  int tmax = 0;
  EMO_CHECK(row_segs(seg, C, &sg, &tmax), "conv_module_bwd_seg: bad segment description");
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes per row and channel: dz, c in (sums); dz, c, g (2) in, dg (2) out
  EmoTimerScope timer_(EMO_TIMER_CONV_MODULE, s, 0.0, 8.0 * (double)sg.row[sg.n] * C * 2.0);
  float* tot = nullptr;
  if (emo_bn_swish_bwd_sums_seg(sg, C, dz, c, bmean, bvar, gamma, beta, eps, dgamma, dbeta, bn_scratch, &tot, s)) return 1;
  if (bwd_lds_attr()) return 1;
  // one partial row per live STRIP, compact (the kernel derives the same row index from the segment table)
  const int S = strip_tiles(seg->n, seg->B, seg->T, cdiv(C, CF_CB));
  dim3 grid(cdiv(cdiv(tmax, CF_TT), S), cdiv(C, CF_CB), sg.b0[sg.n]);
  cf_conv_bwd_kernel<<<grid, CF_CB, CF_BWD_LDS, s>>>(tmax, C, K, (const bf16*)dz, (const bf16*)c, bmean, bvar, gamma, beta, eps, tot,
                                                   (const bf16*)g, w, (bf16*)dg, dw_scratch, S, 0, sg);
  EMO_LAUNCH_CHECK();
  return emo_dwconv_bwd_w_reduce((int)live_strips(seg->n, seg->B, seg->T, S), C, K, dw_scratch, dw, dbias, s);
}
