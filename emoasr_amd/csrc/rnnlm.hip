// One step of the RNN LM (lm/modeling/rnn.py:62-81, RNNLM.predict) for up to 32 hypotheses of a beam search, as L + 2 plain launches:
//
//   rnnlm_layer_*_kernel  x L   one LSTM layer: input rows gathered by index (layer 0: embedding rows by token id; layer l > 0: the new h
//                               of the layer below at dst[i]), previous (h, c) read from the slot pools at src[i] (src[i] < 0: the zero
//                               state), both products, bias_ih + bias_hh, the cell, new (h, c) written to the pools at dst[i]; the top
//                               layer also writes its h as compact rows for the head
//   emoasr_gemm_nt              the vocabulary head on those rows (f32 logits)
//   rnnlm_logp_kernel           log-softmax, row i written to logp[row_dst[i]] (the caller's row cache)
//
// Every index list is an int32 DEVICE array, so the call can be captured into a graph.  Each LSTM layer is an all-to-all seam (every
// gate row needs the whole h of the layer below): the launches are cut there, there is no grid barrier and no hand-off between
// workgroups.  Several rows may share one src (two children of one parent); no dst may equal any src of the same call (another
// workgroup may still be staging that slot).
//
// bf16: each 16-byte piece of the weights is read by exactly one lane of the launch, straight from global memory into the A fragment
// of v_mfma_f32_16x16x32_bf16; the hypotheses are one or two 16-row B tiles from a zero-padded LDS image (the layout of
// rnnt_beam_lstm_mfma_kernel, whose one-tile form this extends).  f32 (and f32x3) and bf16 shapes off the 32-wide k step: the VALU form.
//
// emoasr_rnnlm_step_rows is the same step for any number of rows in one call: the SAME kernel bodies compiled
// with ROWS = true take their tile of 16 / 32 rows from blockIdx.y and form the control words themselves from the batched joint
// search's arrays -- input row ids[r], source slot src_base + parent[r] (a parent outside the call's rows: the zero state), destination
// slot dst_base + r -- so that no host-made index list is needed between two captured steps.  A row's arithmetic does not depend on
// its tile or on the other rows: it gets the bits emoasr_rnnlm_step gives it.  The head's raw f32 logits are the output (the joint
// search's score kernel forms the log-softmax).
//
// Rounding follows the sequence forward (emoasr_amd/recurrence.py): products accumulate in f32, the input projection + bias is rounded
// to the compute dtype, the recurrent product is added to it and rounded again, h is stored in the compute dtype, c in f32.
#include <math.h>
#include "common.h"
#include "lstm_step.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int BT = 256;       // threads per workgroup
constexpr int NBMAX = 32;     // hypotheses per call
constexpr int UN = 8;         // VALU form: hidden units per workgroup (32 gate rows = the 32 eight-lane row groups)

struct LmLayerArgs {
  int nb, nin, H, xrows, slots;
  const void* xtab; long ldx;         // input rows xtab[xidx[i]] (nin values), xrows of them
  const int* xidx;
  const void *w_ih, *w_hh;            // [4H][nin], [4H][H]
  const float* bias;                  // [4H] = bias_ih + bias_hh
  void* ph; float* pc;                // this layer's state pools [slots][H] (T / f32)
  const int *src, *dst;
  void* hrow;                         // top layer: compact [nb][H] copy of the new h (else NULL)
  // ROWS: nb rows in tiles on blockIdx.y; xidx = ids (layer 0) or NULL (the layer below's new h at dst_base + r)
  const int* parent; int src_base, dst_base;
};

// control words of one call, read once: index of the input row / source slot (-1: zeros) / destination slot (-1: dropped).
// Out-of-range indices are turned into -1 here, so no later access leaves its array.
// ROWS: the words of rows r0 .. r0 + nb - 1 formed from (ids, parent, src_base, dst_base)
template <bool ROWS>
__device__ __forceinline__ void load_cw(const LmLayerArgs& a, int (*cw)[NBMAX], int tid, int r0, int nb) {
  if (tid < nb) {
    int x, s, d;
    if constexpr (ROWS) {
      const int r = r0 + tid, p = a.parent[r];
      d = a.dst_base + r;
      x = a.xidx ? a.xidx[r] : d;
      s = (p >= 0 && p < a.nb) ? a.src_base + p : -1;
    } else {
      x = a.xidx[tid]; s = a.src[tid]; d = a.dst[tid];
    }
    cw[0][tid] = (x >= 0 && x < a.xrows) ? x : -1;
    cw[1][tid] = (s >= 0 && s < a.slots) ? s : -1;
    cw[2][tid] = (d >= 0 && d < a.slots) ? d : -1;
  }
}

template <typename T>
__device__ __forceinline__ void cell_store(const LmLayerArgs& a, const int (*cw)[NBMAX], int i, int hi, int uu, float g_i, float g_f,
                                           float g_g, float g_o) {
  const float ig = sigmoid_t<T>(g_i), fg = sigmoid_t<T>(g_f), gg = tanh_t<T>(g_g), og = sigmoid_t<T>(g_o);
  const int s = cw[1][i], d = cw[2][i];
  const float cn = fg * (s >= 0 ? a.pc[(long)s * a.H + uu] : 0.f) + ig * gg;
  const T h = from_f32<T>(og * tanh_t<T>(cn));
  if (d >= 0) {
    a.pc[(long)d * a.H + uu] = cn;
    static_cast<T*>(a.ph)[(long)d * a.H + uu] = h;
  }
  if (a.hrow) static_cast<T*>(a.hrow)[(long)hi * a.H + uu] = h;   // hi: the row of the call (its tile's first row + i)
}

// ---- VALU form: grid = H / UN workgroups; row group grp <-> gate grp / UN, unit u0 + grp % UN; NB = 16 or 32 rows of LDS
template <typename T, int NB, bool ROWS>
__global__ __launch_bounds__(BT) void rnnlm_layer_kernel(const LmLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int r0 = ROWS ? blockIdx.y * NB : 0, nb = ROWS ? min(NB, a.nb - r0) : a.nb;
  const int nin = a.nin, H = a.H, tid = threadIdx.x, grp = tid >> 3, sub = tid & 7;
  float* xs = reinterpret_cast<float*>(smem);          // [NB][nin]
  float* hs = xs + NB * nin;                           // [NB][H]
  float* gs = hs + NB * H;                             // [NB][4 UN]
  const T* xtab = static_cast<const T*>(a.xtab);
  const T* ph = static_cast<const T*>(a.ph);
  __shared__ int cw[3][NBMAX];
  load_cw<ROWS>(a, cw, tid, r0, nb);
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    const int x = cw[0][i], s = cw[1][i];
    for (int k = tid; k < nin; k += BT) xs[i * nin + k] = x >= 0 ? to_f32(xtab[(long)x * a.ldx + k]) : 0.f;
    for (int k = tid; k < H; k += BT) hs[i * H + k] = s >= 0 ? to_f32(ph[(long)s * H + k]) : 0.f;
  }
  __syncthreads();
  const int q = grp / UN, u = blockIdx.x * UN + grp % UN;
  const long row = (long)q * H + u;
  float a_ih[NB], a_hh[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) { a_ih[i] = 0.f; a_hh[i] = 0.f; }
  row_dots<T>(static_cast<const T*>(a.w_ih) + row * nin, nin, xs, nin, nb, sub, a_ih);
  row_dots<T>(static_cast<const T*>(a.w_hh) + row * H, H, hs, H, nb, sub, a_hh);
  const float b = a.bias[row];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    if (i < nb) {
      const float pre = rnd<T>(group_sum8(a_ih[i]) + b);
      const float gate = rnd<T>(pre + group_sum8(a_hh[i]));
      if (sub == 0) gs[i * (4 * UN) + grp] = gate;
    }
  }
  __syncthreads();
  for (int e = tid; e < nb * UN; e += BT) {
    const int i = e / UN, j = e % UN;
    const float* g4 = gs + i * (4 * UN);
    cell_store<T>(a, cw, i, r0 + i, blockIdx.x * UN + j, g4[j], g4[UN + j], g4[2 * UN + j], g4[3 * UN + j]);
  }
}

// ---- bf16 on the matrix cores: grid = H / 16 workgroups of 4 waves, wave q = gate q (i, f, g, o) of the workgroup's 16 hidden units;
// NT = 1 / 2 tiles of 16 hypotheses.  acc[t][r] = D[row 4 * (lane >> 4) + r][hypothesis 16 t + (lane & 15)]
template <int NT>
__device__ __forceinline__ void rows16_dot_tiles(const bf16* __restrict__ wrow0, long ldw, int K, const bf16* __restrict__ xs, int ldxs,
                                                 int lane, f32x4_ (&acc)[NT]) {
  const bf16* wp = wrow0 + (long)(lane & 15) * ldw + 8 * (lane >> 4);
  const bf16* xp = xs + (lane & 15) * ldxs + 8 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int k = 0; k < K; k += 32) {
    const bf16x8 w = *reinterpret_cast<const bf16x8*>(wp + k);   // one weight piece feeds every tile
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(xp + t * 16 * ldxs + k);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, b, acc[t], 0, 0, 0);
    }
  }
}

template <int NT, bool ROWS>
__global__ __launch_bounds__(BT) void rnnlm_layer_mfma_kernel(const LmLayerArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NR = 16 * NT;
  const int r0 = ROWS ? blockIdx.y * NR : 0, nb = ROWS ? min(NR, a.nb - r0) : a.nb;
  const int nin = a.nin, H = a.H, tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int ldx = nin + 8, ldh = H + 8;
  bf16* xs = reinterpret_cast<bf16*>(smem);                 // [NR][nin + 8]
  bf16* hs = xs + NR * ldx;                                 // [NR][H + 8]
  float* gs = reinterpret_cast<float*>(hs + NR * ldh);      // [NR hypotheses][4 gates][16 units]
  const bf16* xtab = static_cast<const bf16*>(a.xtab);
  const bf16* ph = static_cast<const bf16*>(a.ph);
  __shared__ int cw[3][NBMAX];
  load_cw<ROWS>(a, cw, tid, r0, nb);
  __syncthreads();
  // stage the inputs in 16-byte pieces; zero rows for hypotheses >= nb, absent input rows and the zero state
  for (int p = tid; p < NR * (nin / 8); p += BT) {
    const int i = p / (nin / 8), c = (p % (nin / 8)) * 8;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)0.f;
    if (i < nb && cw[0][i] >= 0) v = *reinterpret_cast<const bf16x8*>(xtab + (long)cw[0][i] * a.ldx + c);
    *reinterpret_cast<bf16x8*>(xs + i * ldx + c) = v;
  }
  for (int p = tid; p < NR * (H / 8); p += BT) {
    const int i = p / (H / 8), c = (p % (H / 8)) * 8;
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)0.f;
    if (i < nb && cw[1][i] >= 0) v = *reinterpret_cast<const bf16x8*>(ph + (long)cw[1][i] * H + c);
    *reinterpret_cast<bf16x8*>(hs + i * ldh + c) = v;
  }
  __syncthreads();
  const int u0 = blockIdx.x * 16;
  const long row0 = (long)q * H + u0;
  f32x4_ d_ih[NT], d_hh[NT];
  rows16_dot_tiles<NT>(static_cast<const bf16*>(a.w_ih) + row0 * nin, nin, nin, xs, ldx, lane, d_ih);
  rows16_dot_tiles<NT>(static_cast<const bf16*>(a.w_hh) + row0 * H, H, H, hs, ldh, lane, d_hh);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int i = 16 * t + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 4 * (lane >> 4) + r;   // unit inside the workgroup
      const float pre = rnd<bf16>(d_ih[t][r] + a.bias[row0 + j]);
      gs[(i * 4 + q) * 16 + j] = rnd<bf16>(pre + d_hh[t][r]);
    }
  }
  __syncthreads();
  for (int e = tid; e < nb * 16; e += BT) {
    const int i = e / 16, j = e % 16;
    const float* g4 = gs + i * 64;
    cell_store<bf16>(a, cw, i, r0 + i, u0 + j, g4[j], g4[16 + j], g4[32 + j], g4[48 + j]);
  }
}

// one workgroup per row: logp[row_dst[i]] = log_softmax(logits[i, :V])   (row_dst NULL: row i; a row outside the cache is dropped)
__global__ __launch_bounds__(BT) void rnnlm_logp_kernel(int V, const float* __restrict__ logits, long ldl, float* __restrict__ logp,
                                                       long ldo, int out_rows, const int* __restrict__ row_dst) {
  __shared__ float red[16];
  const int i = blockIdx.x, tid = threadIdx.x;
  const int o = row_dst ? row_dst[i] : i;
  const float* x = logits + (long)i * ldl;
  float mx = -INFINITY;
  for (int v = tid; v < V; v += BT) mx = fmaxf(mx, x[v]);
  mx = block_max(mx, red);
  float se = 0.f;
  for (int v = tid; v < V; v += BT) se += expf(x[v] - mx);
  se = block_sum(se, red);
  if (o < 0 || o >= out_rows) return;
  const float lse = mx + logf(se);
  float* y = logp + (long)o * ldo;
  for (int v = tid; v < V; v += BT) y[v] = x[v] - lse;
}

constexpr size_t LDS_MAX = 150 * 1024;
inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }
inline size_t mfma_lds(int nt, int nin, int H) { return (size_t)16 * nt * (nin + 8 + H + 8) * 2 + (size_t)16 * nt * 64 * sizeof(float); }
inline size_t valu_lds(int nbr, int nin, int H) { return ((size_t)nbr * (nin + H) + (size_t)nbr * 4 * UN) * sizeof(float); }
inline bool mfma_ok(int dtype, int nin, int H) { return dtype == EMO_BF16 && H % 32 == 0 && nin % 32 == 0; }
// does one layer (input width nin) fit a kernel form?
inline bool layer_ok(int dtype, int nb, int nin, int H) {
  const int vec = dtype == EMO_BF16 ? 8 : 4;
  if (nin < vec || H < UN || nin % vec || H % vec || H % UN) return false;
  if (mfma_ok(dtype, nin, H)) return mfma_lds(nb > 16 ? 2 : 1, nin, H) <= LDS_MAX;
  return valu_lds(nb > 16 ? 32 : 16, nin, H) <= LDS_MAX;
}

template <typename K>
int set_lds(K kernel, size_t bytes, size_t* granted) {
  if (bytes > 64 * 1024 && bytes > *granted) {
    EMO_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess,
              "rnnlm_step: hipFuncSetAttribute(%zu) failed", bytes);
    *granted = bytes;
  }
  return 0;
}

// ROWS: a.nb rows in tiles of 16 (a.nb <= 16: one tile) or 32 on blockIdx.y
template <bool ROWS>
int launch_layer(int dtype, const LmLayerArgs& a, hipStream_t s) {
  const int two = a.nb > 16;
  const unsigned tiles = ROWS ? (a.nb + (two ? 32 : 16) - 1) / (two ? 32 : 16) : 1;
  if (mfma_ok(dtype, a.nin, a.H)) {
    const size_t sm = mfma_lds(two ? 2 : 1, a.nin, a.H);
    static size_t g1 = 0, g2 = 0;
    if (two) {
      if (set_lds(rnnlm_layer_mfma_kernel<2, ROWS>, sm, &g2)) return 1;
      rnnlm_layer_mfma_kernel<2, ROWS><<<dim3(a.H / 16, tiles), BT, sm, s>>>(a);
    } else {
      if (set_lds(rnnlm_layer_mfma_kernel<1, ROWS>, sm, &g1)) return 1;
      rnnlm_layer_mfma_kernel<1, ROWS><<<dim3(a.H / 16, tiles), BT, sm, s>>>(a);
    }
    EMO_LAUNCH_CHECK();
    return 0;
  }
  const size_t sm = valu_lds(two ? 32 : 16, a.nin, a.H);
  EMO_DISPATCH(dtype, {
    static size_t g1 = 0, g2 = 0;
    if (two) {
      if (set_lds(rnnlm_layer_kernel<T, 32, ROWS>, sm, &g2)) return 1;
      rnnlm_layer_kernel<T, 32, ROWS><<<dim3(a.H / UN, tiles), BT, sm, s>>>(a);
    } else {
      if (set_lds(rnnlm_layer_kernel<T, 16, ROWS>, sm, &g1)) return 1;
      rnnlm_layer_kernel<T, 16, ROWS><<<dim3(a.H / UN, tiles), BT, sm, s>>>(a);
    }
  });
  EMO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int emoasr_rnnlm_step_supported(int dtype, int nb, int L, int E, int H) {
  if (!(dtype == EMO_F32 || dtype == EMO_BF16 || dtype == EMO_F32X3)) return 0;
  if (nb < 1 || nb > NBMAX || L < 1) return 0;
  return layer_ok(dtype, nb, E, H) && (L == 1 || layer_ok(dtype, nb, H, H)) ? 1 : 0;
}

extern "C" long emoasr_rnnlm_step_ws_bytes(int dtype, int H, int V) {
  const size_t es = dtype == EMO_BF16 ? 2 : 4;
  return (long)(align256((size_t)NBMAX * H * es) + align256((size_t)NBMAX * V * sizeof(float)));
}

extern "C" int emoasr_rnnlm_step(int dtype, int nb, int L, int E, int H, int V, int slots, const int* ids, const void* emb,
                                 const void* const* w_ih, const void* const* w_hh, const float* const* bias, void* ph, float* pc,
                                 const int* src, const int* dst, const void* w_out, const float* b_out, float* logp, long ldlogp,
                                 int logp_rows, const int* row_dst, void* ws, long ws_bytes, void* stream) {
  EMO_CHECK(emoasr_rnnlm_step_supported(dtype, nb, L, E, H), "rnnlm_step: nb=%d L=%d E=%d H=%d outside the kernel's shape plan", nb,
            L, E, H);
  EMO_CHECK(V >= 1 && slots >= 1 && ldlogp >= V && logp_rows >= 1, "rnnlm_step: V=%d slots=%d ldlogp=%ld logp_rows=%d", V, slots,
            ldlogp, logp_rows);
  EMO_CHECK(ws && ws_bytes >= emoasr_rnnlm_step_ws_bytes(dtype, H, V), "rnnlm_step: workspace of %ld bytes is too small", ws_bytes);
  const size_t es = dtype == EMO_BF16 ? 2 : 4;
  char* hrow = static_cast<char*>(ws);
  float* logits = reinterpret_cast<float*>(hrow + align256((size_t)NBMAX * H * es));
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < L; ++l) {
    LmLayerArgs a;
    a.nb = nb; a.H = H; a.slots = slots;
    if (l == 0) { a.nin = E; a.xrows = V; a.xtab = emb; a.ldx = E; a.xidx = ids; }
    else { a.nin = H; a.xrows = slots; a.xtab = static_cast<char*>(ph) + (size_t)(l - 1) * slots * H * es; a.ldx = H; a.xidx = dst; }
    a.w_ih = w_ih[l]; a.w_hh = w_hh[l]; a.bias = bias[l];
    a.ph = static_cast<char*>(ph) + (size_t)l * slots * H * es;
    a.pc = pc + (size_t)l * slots * H;
    a.src = src; a.dst = dst;
    a.hrow = l == L - 1 ? hrow : nullptr;
    a.parent = nullptr; a.src_base = a.dst_base = 0;
    if (launch_layer<false>(dtype, a, s)) return 1;
  }
  emoasr_epilogue_t ep = {};
  ep.bias = b_out; ep.alpha = 1.f; ep.res_scale = 1.f; ep.out_f32 = 1;
  if (emoasr_gemm_nt(dtype, nb, V, H, hrow, H, w_out, H, logits, V, &ep, stream)) return 1;
  rnnlm_logp_kernel<<<nb, BT, 0, s>>>(V, logits, V, logp, ldlogp, logp_rows, row_dst);
  EMO_LAUNCH_CHECK();
  return 0;
}

// ---- the step for R rows of the batched joint search ---------------------------------------------------------
constexpr int ROWS_MAX = 65535 * 16;   // tiles on blockIdx.y

extern "C" int emoasr_rnnlm_step_rows_supported(int dtype, int L, int E, int H) { return emoasr_rnnlm_step_supported(dtype, NBMAX, L, E, H); }

extern "C" long emoasr_rnnlm_step_rows_ws_bytes(int dtype, int R, int H) {
  const size_t es = dtype == EMO_BF16 ? 2 : 4;
  return R >= 1 && H >= 1 ? (long)align256((size_t)R * H * es) : 0;
}

extern "C" int emoasr_rnnlm_step_rows(int dtype, const emoasr_rnnlm_rows_t* rl, const int* ids, const int* parent, void* stream) {
  EMO_CHECK(rl && ids && parent, "rnnlm_step_rows: missing arguments");
  const int L = rl->L, E = rl->E, H = rl->H, V = rl->V, R = rl->R, slots = rl->slots;
  EMO_CHECK(emoasr_rnnlm_step_rows_supported(dtype, L, E, H), "rnnlm_step_rows: L=%d E=%d H=%d outside the kernel's shape plan", L, E, H);
  EMO_CHECK(R >= 1 && R <= ROWS_MAX && V >= 1 && rl->ldl >= V, "rnnlm_step_rows: R=%d V=%d ldl=%ld", R, V, rl->ldl);
  EMO_CHECK(rl->emb && rl->w_ih && rl->w_hh && rl->bias && rl->w_out && rl->ph && rl->pc && rl->logits, "rnnlm_step_rows: missing operands");
  // both slot ranges inside the pools, and apart: another workgroup may still be staging a source slot
  const long sb = rl->src_base, db = rl->dst_base;
  EMO_CHECK(sb >= 0 && db >= 0 && sb + R <= slots && db + R <= slots && (sb + R <= db || db + R <= sb),
            "rnnlm_step_rows: source slots %ld.. and destination slots %ld.. of %d rows in pools of %d slots", sb, db, R, slots);
  EMO_CHECK(rl->ws && rl->ws_bytes >= emoasr_rnnlm_step_rows_ws_bytes(dtype, R, H), "rnnlm_step_rows: workspace of %ld bytes is too small",
            rl->ws_bytes);
  const size_t es = dtype == EMO_BF16 ? 2 : 4;
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < L; ++l) {
    LmLayerArgs a;
    a.nb = R; a.H = H; a.slots = slots;
    if (l == 0) { a.nin = E; a.xrows = V; a.xtab = rl->emb; a.ldx = E; a.xidx = ids; }
    else { a.nin = H; a.xrows = slots; a.xtab = static_cast<char*>(rl->ph) + (size_t)(l - 1) * slots * H * es; a.ldx = H; a.xidx = nullptr; }
    a.w_ih = rl->w_ih[l]; a.w_hh = rl->w_hh[l]; a.bias = rl->bias[l];
    a.ph = static_cast<char*>(rl->ph) + (size_t)l * slots * H * es;
    a.pc = rl->pc + (size_t)l * slots * H;
    a.src = a.dst = nullptr;
    a.parent = parent; a.src_base = rl->src_base; a.dst_base = rl->dst_base;
    a.hrow = l == L - 1 ? rl->ws : nullptr;
    if (launch_layer<true>(dtype, a, s)) return 1;
  }
  emoasr_epilogue_t ep = {};
  ep.bias = rl->b_out; ep.alpha = 1.f; ep.res_scale = 1.f; ep.out_f32 = 1;
  return emoasr_gemm_nt(dtype, R, V, H, rl->ws, H, rl->w_out, H, rl->logits, rl->ldl, &ep, stream);
}
