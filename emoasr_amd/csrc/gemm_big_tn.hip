// Eight-wave 256x256 tile for the bf16 weight-gradient (TN) products: C[n1, n2] += alpha * sum_k A[k, n1] * B[k, n2], f32
// accumulation, f32 atomics across split-K slices, optional bias gradient colsum[n1] += s * sum_k A[k, n1] -- the contract of
// tn_block in gemm.hip, for products with N2 a multiple of 256 and N1 >= 256 (N1 may be ragged where lda is padded).
//
// Structure (one workgroup per CU, the layout of gemm_big.hip transposed):
//   * 512 threads = 8 waves as 2 (n1) x 4 (n2); wave tile 128 x 64 = 4 x 2 accumulators of the 32x32x16 MFMA (128 registers).
//     One register of a 32x32 accumulator is two 128-byte row segments per wave instruction: the atomic shape that runs at full rate.
//   * k-tiles of 32 rows; both operands are k-major, so a k row of a tile is one 512-byte piece of a source row.  A ring of four
//     stages (A 16 KB + B 16 KB each, 128 KB) filled by LDS-DMA, three tiles in flight; a wave instruction lands two k rows.
//     The image is lane-linear, so the bank swizzle sits on the SOURCE side: position c of k row r holds source chunk
//     c ^ ((r & 3) << 2) (16-byte chunks).  Fragments come out with ds_read_b64_tr_b16: a 32-lane half reads k rows q = 0..3, 64
//     bytes each, which the XOR puts on the four different 16-bank groups -- conflict-free (plain 512-byte rows: 4-way).
//   * one raw s_barrier per k-tile and a counted vmcnt wait (the two newest tiles stay in flight across it); the DMA for tile
//     t + 3 goes into the stage tile t - 1 used, right after the barrier that proves every wave is done with it.
//   * rows k >= K and columns n1 >= N1 land as zeros through the descriptor's bounds check; tiles past the block's k slice too.
//   * bias gradient: summed from the staged A image; the blocks of one row of tiles take the k-tiles in turn (as tn_block does).
//   * two forms: grouped plain products (BigTnGroup: a layer's weight gradients, the vocabulary head, the front-end Linear) and the
//     Conv2d weight gradient with gathered B rows over several micro-batches as one reduction (BigTnConv, below).
//   * measured (MI355X, inside the training step): a layer's nine products 174 -> 165 us against the 128x128 four-wave tile, the
//     Conv2d weight gradient of five micro-batches 5 x 216 -> 946 us; DESIGN.md section 4.1.
#include <algorithm>
#include <type_traits>
#include "mma.h"
#include "lds_dma.h"
#include "../../include/emoasr_hip.h"
#include "gemm_big_tn.h"

namespace {

// Timing-only build variants (-DEMO_TN_ABLATE=<bits>; the results are wrong): 1 no DMA after the prologue, 2 no fragment reads,
// 4 no barrier, 8 no atomic epilogue.  MFMAs alone = 7, + fragment reads = 5, + barrier = 1, everything = 0.
#ifndef EMO_TN_ABLATE
#define EMO_TN_ABLATE 0
#endif
constexpr int TN_BK = 32, TN_STAGES = 4;
constexpr int TN_OP_BYTES = TN_BK * 512;          // one operand tile: 32 k rows x 256 bf16
constexpr int TN_STAGE_BYTES = 2 * TN_OP_BYTES;   // A then B
constexpr int TN_LDS_BYTES = TN_STAGES * TN_STAGE_BYTES;

struct BigTnGroup {
  int n;
  int start[EMOASR_TN_GROUP_MAX + 1];   // first block of problem p; start[n] = blocks of the launch
  BigTnProblem p[EMOASR_TN_GROUP_MAX];
};

// byte offset of element (k row r, column col) of an operand tile image
__device__ __forceinline__ unsigned tn_img_off(int r, int col) {
  return (unsigned)(512 * r + 16 * ((col >> 3) ^ ((r & 3) << 2)) + 2 * (col & 7));
}

// Conv2d(C -> C, k3, s2) weight gradient over up to EMOASR_CONV2_WGRAD_SEGMENTS micro-batches as ONE reduction:
//   dw[n, (kh, kw, c)] += sum over segments s and rows (b, t2, f2) of dy2_s[(b, t2, f2), n] * y1_s[b, 2 t2 + kh, 2 f2 + kw, c]
// A = dy2_s (plain rows), B rows gathered: a 256-column tile lies inside one tap (C % 256 == 0), a 512-byte piece of the input row.
// Every segment's rows are padded (with zero-filled rows) to whole k-tiles, so a k-tile belongs to ONE segment and the segment
// lookup is scalar; a block's k range may cross segment boundaries.
struct BigTnConv {
  int nseg, F1, F2, C;
  int T1[EMOASR_CONV2_WGRAD_SEGMENTS], T2[EMOASR_CONV2_WGRAD_SEGMENTS], B[EMOASR_CONV2_WGRAD_SEGMENTS];
  int tile0[EMOASR_CONV2_WGRAD_SEGMENTS + 1];   // first k-tile of segment s; tile0[nseg] = k-tiles of the reduction
  const void* dy2[EMOASR_CONV2_WGRAD_SEGMENTS];
  const void* y1[EMOASR_CONV2_WGRAD_SEGMENTS];
  float* dw;
  float* dbias;
  int k_tiles_per_split;
};

// BMODE 0: ARGS = BigTnGroup (plain products, grouped).  BMODE 1: ARGS = BigTnConv.
template <int BMODE, typename ARGS>
__global__ __launch_bounds__(512) void big_tn_kernel(const ARGS G) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // blocks are numbered problem by problem, a k slice's tiles next to each other; contiguous eighths of that list per XCD
  const int bid = xcd_remap_big(blockIdx.x, gridDim.x);
  // the product this block works on: C[N1, N2] (ldc) += alpha * ..., colsum[N1] += cscale * ...
  int N1, N2, local, nk_total, ktps;
  float* Cp; long ldc; float alpha; float* colsum; float cscale;
  [[maybe_unused]] int pidx = 0;
  if constexpr (BMODE == 0) {
    while (pidx + 1 < G.n && bid >= G.start[pidx + 1]) ++pidx;
    const BigTnProblem& g = G.p[pidx];
    local = bid - G.start[pidx];
    N1 = g.N1; N2 = g.N2; nk_total = (g.K + TN_BK - 1) / TN_BK; ktps = g.k_tiles_per_split;
    Cp = g.C; ldc = g.ldc; alpha = g.alpha; colsum = g.colsum; cscale = g.colsum_scale;
  } else {
    local = bid;
    N1 = G.C; N2 = 9 * G.C; nk_total = G.tile0[G.nseg]; ktps = G.k_tiles_per_split;
    Cp = G.dw; ldc = 9 * G.C; alpha = 1.f; colsum = G.dbias; cscale = 1.f;
  }
  const int tx = N2 / 256, ty = (N1 + 255) / 256;
  const int bx = local % tx, by = (local / tx) % ty, bz = local / (tx * ty);
  const int n1_0 = by * 256, n2_0 = bx * 256;
  const int kt_begin = bz * ktps;
  const int kt_end = nk_total < kt_begin + ktps ? nk_total : kt_begin + ktps;
  if (kt_begin >= kt_end) return;   // (block-uniform)
  const int nt = kt_end - kt_begin;

  // ---- DMA source offsets: per tile and wave two pieces of each operand, a piece = two k rows (one per 32-lane half) ------------
  const int half = lane >> 5, cpos = lane & 31;
  unsigned a_cur[2], b_cur[2];
  bool a_ok[2];
  [[maybe_unused]] unsigned a_step = 0, b_step = 0;
  __amdgpu_buffer_rsrc_t rsA, rsB;
  // BMODE 1: the segment (scalar) and tile within it of the next tile to issue; per piece the lane's row (b, t2, f2), local index lr
  [[maybe_unused]] int seg = 0, lt = 0, cv_b[2], cv_t2[2], cv_f2[2], cv_lr[2];
  [[maybe_unused]] unsigned ch_a[2], ch_b[2];
  if constexpr (BMODE == 0) {
    const BigTnProblem& g = G.p[pidx];
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int r = 2 * (wave + 8 * pc) + half;
      const int ch = cpos ^ ((r & 3) << 2);
      const int na = n1_0 + ch * 8, nb = n2_0 + ch * 8;
      const long k = (long)kt_begin * TN_BK + r;
      a_ok[pc] = na < N1;
      a_cur[pc] = (unsigned)((k * g.lda + na) * 2);
      b_cur[pc] = (unsigned)((k * g.ldb + nb) * 2);
    }
    a_step = (unsigned)(TN_BK * g.lda * 2); b_step = (unsigned)(TN_BK * g.ldb * 2);
    // descriptors end behind the last readable element: every row k >= K is out of range
    const int n1_pad = (N1 + 7) / 8 * 8;
    rsA = make_rsrc_n(g.A, (unsigned)((((long)g.K - 1) * g.lda + n1_pad) * 2));
    rsB = make_rsrc_n(g.B, (unsigned)((((long)g.K - 1) * g.ldb + N2) * 2));
  } else {
    const int tap = n2_0 / G.C, c0 = n2_0 - tap * G.C, kh = tap / 3, kw = tap - 3 * kh;
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int r = 2 * (wave + 8 * pc) + half;
      const int ch = cpos ^ ((r & 3) << 2);
      a_ok[pc] = true;
      ch_a[pc] = (unsigned)((n1_0 + ch * 8) * 2);
      ch_b[pc] = (unsigned)((((kh * G.F1 + kw) * G.C) + c0 + ch * 8) * 2);
    }
    while (seg + 1 < G.nseg && kt_begin >= G.tile0[seg + 1]) ++seg;
    lt = kt_begin - G.tile0[seg];
    rsA = make_rsrc_n(G.dy2[0], 0); rsB = rsA;
  }
  // BMODE 1: (b, t2, f2) of the lane's rows of tile lt of segment seg, by division (once per block and per segment entered)
  auto conv_seek = [&]() __attribute__((always_inline)) {
    if constexpr (BMODE == 1) {
      const int per_b = G.T2[seg] * G.F2;
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) {
        const int lr = lt * TN_BK + 2 * (wave + 8 * pc) + half;
        cv_lr[pc] = lr;
        cv_b[pc] = lr / per_b;
        const int rem = lr - cv_b[pc] * per_b;
        cv_t2[pc] = rem / G.F2;
        cv_f2[pc] = rem - cv_t2[pc] * G.F2;
      }
    }
  };
  conv_seek();
  auto issue = [&](const int it) __attribute__((always_inline)) {
    const bool live = it < nt;
    char* st = smem + (it & (TN_STAGES - 1)) * TN_STAGE_BYTES + wave * 1024;
    if constexpr (BMODE == 1) {
      const int T1s = G.T1[seg], T2s = G.T2[seg], Bs = G.B[seg];
      const int rows_s = Bs * T2s * G.F2;
      rsA = make_rsrc_n(G.dy2[seg], (unsigned)((long)rows_s * G.C * 2));
      rsB = make_rsrc_n(G.y1[seg], (unsigned)((long)Bs * T1s * G.F1 * G.C * 2));
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) {
        a_ok[pc] = cv_lr[pc] < rows_s;
        a_cur[pc] = (unsigned)cv_lr[pc] * (unsigned)(G.C * 2) + ch_a[pc];
        b_cur[pc] = (unsigned)((((long)cv_b[pc] * T1s + 2 * cv_t2[pc]) * G.F1 + 2 * cv_f2[pc]) * G.C * 2) + ch_b[pc];
      }
    }
#pragma unroll
    for (int pc = 0; pc < 2; ++pc) dma16(rsA, st + pc * 8192, live && a_ok[pc] ? a_cur[pc] : EMO_OOB, 0);
#pragma unroll
    for (int pc = 0; pc < 2; ++pc)
      dma16(rsB, st + TN_OP_BYTES + pc * 8192, live && (BMODE == 0 || a_ok[pc]) ? b_cur[pc] : EMO_OOB, 0);
    if constexpr (BMODE == 0) {
#pragma unroll
      for (int pc = 0; pc < 2; ++pc) { a_cur[pc] += a_step; b_cur[pc] += b_step; }
    } else {
      ++lt;
      if (seg + 1 < G.nseg && lt >= G.tile0[seg + 1] - G.tile0[seg]) {   // (scalar: the next tile opens the next segment)
        ++seg;
        lt = 0;
        conv_seek();
      } else {
        const int T2s = G.T2[seg];
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
          cv_lr[pc] += TN_BK;
          cv_f2[pc] += TN_BK;
          while (cv_f2[pc] >= G.F2) { cv_f2[pc] -= G.F2; ++cv_t2[pc]; }
          while (cv_t2[pc] >= T2s) { cv_t2[pc] -= T2s; ++cv_b[pc]; }
        }
      }
    }
  };

  // ---- fragment read offsets (ds_read_b64_tr_b16: lane 4q + p of a 16-lane group addresses k row q, columns 4p .. 4p + 3) -------
  const int wr = wave >> 2, wc = wave & 3;
  const int q = (lane & 15) >> 2, pp = lane & 3, h16 = (lane >> 4) & 1, kb = 8 * (lane >> 5);
  unsigned a_fo[4], b_fo[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_fo[i] = tn_img_off(kb + q, wr * 128 + i * 32 + 16 * h16 + 4 * pp);
#pragma unroll
  for (int j = 0; j < 2; ++j) b_fo[j] = TN_OP_BYTES + tn_img_off(kb + q, wc * 64 + j * 32 + 16 * h16 + 4 * pp);
  // (the reads below add multiples of four k rows: (k & 3) and with it the XOR term stay those of row kb + q)
  // The reads are inline assembly: behind the intrinsic the compiler puts s_waitcnt vmcnt(0) in front of every LDS read that may
  // alias an LDS-DMA destination, which would drain the two tiles meant to stay in flight.  It does not count these reads either,
  // so tr_wait() below is the lgkmcnt wait, tied to the registers it releases.
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  unsigned a_ad[4], b_ad[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_ad[i] = lds0 + a_fo[i];
#pragma unroll
  for (int j = 0; j < 2; ++j) b_ad[j] = lds0 + b_fo[j];
  struct Frags { s16x4 a[4][2], b[2][2]; };   // [fragment][k rows 0..3 / 4..7 of the lane's eight]
#if EMO_TN_ABLATE & 2
#define TN_TR_READ(dst, addr, OFF) asm volatile("; no read" : "=v"(dst) : "v"(addr), "n"(OFF))
#else
#define TN_TR_READ(dst, addr, OFF) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))
#endif
  auto read_frags = [&](Frags& f, const unsigned stage, auto kk_c) __attribute__((always_inline)) {
    constexpr int KO = decltype(kk_c)::value * 512;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned ad = a_ad[i] + stage;
      TN_TR_READ(f.a[i][0], ad, KO);
      TN_TR_READ(f.a[i][1], ad, KO + 2048);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned ad = b_ad[j] + stage;
      TN_TR_READ(f.b[j][0], ad, KO);
      TN_TR_READ(f.b[j][1], ad, KO + 2048);
    }
  };
#undef TN_TR_READ
  // wait until at most N of the reads issued so far are outstanding; f's registers are valid from here
  auto tr_wait = [&](Frags& f, auto n_c) __attribute__((always_inline)) {
    if constexpr (decltype(n_c)::value == 0)
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]), "+v"(f.a[2][0]), "+v"(f.a[2][1]),
                     "+v"(f.a[3][0]), "+v"(f.a[3][1]), "+v"(f.b[0][0]), "+v"(f.b[0][1]), "+v"(f.b[1][0]), "+v"(f.b[1][1]));
    else
      asm volatile("s_waitcnt lgkmcnt(12)"
                   : "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]), "+v"(f.a[2][0]), "+v"(f.a[2][1]),
                     "+v"(f.a[3][0]), "+v"(f.a[3][1]), "+v"(f.b[0][0]), "+v"(f.b[0][1]), "+v"(f.b[1][0]), "+v"(f.b[1][1]));
    static_assert(decltype(n_c)::value == 0 || decltype(n_c)::value == 12, "tr_wait: 0 or one set of 12 reads");
  };
  auto join = [](const s16x4 lo, const s16x4 hi) -> bf16x8 {
    union { bf16x8 f; s16x4 hh[2]; } u;
    u.hh[0] = lo; u.hh[1] = hi;
    return u.f;
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const bool do_colsum = colsum != nullptr;
  const int cs_col = tid & 255, cs_k0 = (tid >> 8) * 16;
  float csum = 0.f;

  issue(0);
  issue(1);
  issue(2);
  for (int it = 0; it < nt; ++it) {
    wait_vmcnt<8>();                  // this wave's pieces of tile `it` have landed (tiles it + 1, it + 2 stay in flight)
    if constexpr (!(EMO_TN_ABLATE & 4)) __builtin_amdgcn_s_barrier();     // ... and everybody's; every wave is done with tile it - 1
    if constexpr (!(EMO_TN_ABLATE & 1)) issue(it + 3);
    if (do_colsum && (kt_begin + it) % tx == bx) {
      const char* st = smem + (it & (TN_STAGES - 1)) * TN_STAGE_BYTES;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        csum += to_f32(*reinterpret_cast<const bf16*>(st + tn_img_off(cs_k0 + k, cs_col)));
    }
    const unsigned stage = (unsigned)((it & (TN_STAGES - 1)) * TN_STAGE_BYTES);
    Frags f0, f1;
    read_frags(f0, stage, std::integral_constant<int, 0>{});
    read_frags(f1, stage, std::integral_constant<int, 16>{});
    tr_wait(f0, std::integral_constant<int, 12>{});   // (LDS returns in order: the first set is in)
    auto mfmas = [&](const Frags& f) __attribute__((always_inline)) {
      bf16x8 af[4], bfr[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = join(f.a[i][0], f.a[i][1]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = join(f.b[j][0], f.b[j][1]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    };
    mfmas(f0);
    tr_wait(f1, std::integral_constant<int, 0>{});
    mfmas(f1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the (zero-fill) DMAs past the slice: nothing in flight when the block ends
  if constexpr ((EMO_TN_ABLATE & 8) != 0) { if (alpha != 12345.f) return; }   // (keeps the accumulators alive)

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n2_0 + wc * 64 + j * 32 + c_col(lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = n1_0 + wr * 128 + i * 32 + c_row(r, lane);
        if (row >= N1) continue;
        atomicAdd(&Cp[(long)row * ldc + col], alpha * acc[i][j][r]);
      }
    }
  if (do_colsum && n1_0 + cs_col < N1) atomicAdd(&colsum[n1_0 + cs_col], cscale * csum);
}

}  // namespace

bool emo_tn_big_fits(int N1, int N2, int K, long lda, long ldb) {
  // the tile needs whole 256-column pieces of B and at least one full tile of A rows; offsets are 32-bit
  return N2 % 256 == 0 && N1 >= 256 && lda % 8 == 0 && ldb % 8 == 0 &&
         ((long)K + 4 * TN_BK) * lda * 2 < (1L << 32) && ((long)K + 4 * TN_BK) * ldb * 2 < (1L << 32);
}

int emo_tn_big_launch(int n, const BigTnProblem* probs, const int* splits, hipStream_t s) {
  BigTnGroup G{};
  G.n = n;
  int start = 0;
  for (int i = 0; i < n; ++i) {
    G.p[i] = probs[i];
    const int nk = (probs[i].K + TN_BK - 1) / TN_BK;
    const int want = std::max(1, std::min(splits[i], nk));
    G.p[i].k_tiles_per_split = (nk + want - 1) / want;
    const int sp = (nk + G.p[i].k_tiles_per_split - 1) / G.p[i].k_tiles_per_split;
    G.start[i] = start;
    start += (probs[i].N2 / 256) * ((probs[i].N1 + 255) / 256) * sp;
  }
  G.start[n] = start;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)big_tn_kernel<0, BigTnGroup>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_BYTES);
    if (e != hipSuccess) { emo_set_error("hipFuncSetAttribute(%d): %s", TN_LDS_BYTES, hipGetErrorString(e)); return 1; }
    attr_done = true;
  }
  big_tn_kernel<0, BigTnGroup><<<start, 512, TN_LDS_BYTES, s>>>(G);
  EMO_LAUNCH_CHECK();
  return 0;
}

bool emo_tn_big_conv_fits(int nseg, const emoasr_conv2_wgrad_seg_t* segs, int F1, int C) {
  if (C % 256 != 0 || nseg < 1 || nseg > EMOASR_CONV2_WGRAD_SEGMENTS) return false;
  for (int i = 0; i < nseg; ++i)   // 32-bit byte offsets into every segment's input
    if ((long)segs[i].B * segs[i].T1 * F1 * C * 2 >= (1L << 32)) return false;
  return true;
}

int emo_tn_big_conv_launch(int nseg, const emoasr_conv2_wgrad_seg_t* segs, int F1, int C, float* dw, float* dbias, int blocks,
                           int max_splits, hipStream_t s) {
  BigTnConv G{};
  G.nseg = nseg; G.F1 = F1; G.F2 = (F1 - 3) / 2 + 1; G.C = C; G.dw = dw; G.dbias = dbias;
  int tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    G.T1[i] = segs[i].T1; G.T2[i] = (segs[i].T1 - 3) / 2 + 1; G.B[i] = segs[i].B;
    G.dy2[i] = segs[i].dy2; G.y1[i] = segs[i].y1;
    G.tile0[i] = tiles;
    tiles += (G.B[i] * G.T2[i] * G.F2 + TN_BK - 1) / TN_BK;
  }
  G.tile0[nseg] = tiles;
  const int out_tiles = (9 * C / 256) * (C / 256);
  const int want = std::max(1, std::min(std::min(blocks / out_tiles, max_splits), tiles / 4 > 0 ? tiles / 4 : 1));
  G.k_tiles_per_split = (tiles + want - 1) / want;
  const int sp = (tiles + G.k_tiles_per_split - 1) / G.k_tiles_per_split;
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute((const void*)big_tn_kernel<1, BigTnConv>, hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_BYTES);
    if (e != hipSuccess) { emo_set_error("hipFuncSetAttribute(%d): %s", TN_LDS_BYTES, hipGetErrorString(e)); return 1; }
    attr_done = true;
  }
  big_tn_kernel<1, BigTnConv><<<out_tiles * sp, 512, TN_LDS_BYTES, s>>>(G);
  EMO_LAUNCH_CHECK();
  return 0;
}
