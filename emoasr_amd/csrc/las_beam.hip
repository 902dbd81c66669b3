// Kernels of the BATCHED LAS beam search (engine/las.py:las_beam_search_batch): S searches of width W occupy
// rows s * W .. s * W + W - 1 of every per-hypothesis array, as in csrc/decode_batch.hip, and step in lockstep.
//   * emoasr_las_attend_group: one decoder position of the location-aware attention (csrc/las.hip: las_score_kernel / las_ctx_kernel
//     with drop_p = 0, the same arithmetic in the same order) for all rows, against the searches' STACKED key projections and
//     encoder frames -- stored once per utterance, a tile fetched once for the rows of a search.  A row convolves the previous
//     weights of its PARENT row (the int32 global row emoasr_beam_update_batch leaves in n_parent): the gather of the largest
//     state array happens inside the kernel.
//   * emoasr_las_state_gather: parent row -> child row for the small state arrays of a step, through a pointer table, one launch.
//   * emoasr_las_attend_cells: emoasr_las_attend_group for the fusion grid -- a search is an (utterance,
//     lm_weight) pair, search s runs over the frames of utterance sutt[s], stored once per UTTERANCE.  The same kernels, compiled
//     with the CELLS flag: a row gets the bits the group form gives it over replicated frames.
// All read the update kernel's state array: a row at or past its search's n_alive, and every row of a finished search, is
// skipped -- nothing of it is read, nothing is written for it.  Every index that comes from device memory (offsets, parents, the
// live count) is range-checked before it addresses anything.
#include <cfloat>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int LAS_C = EMOASR_LAS_CONV_CHANNELS, LAS_K = EMOASR_LAS_CONV_WIDTH, LAS_HALO = (LAS_K - 1) / 2;
constexpr int LAS_TT = 32;                          // frames per tile
constexpr int LAS_STRIP = LAS_TT + 2 * LAS_HALO;    // 232
constexpr int LAS_MAX_A = 512;                      // one 8-channel group per lane
constexpr int LAS_CTX_COLS = 64;
constexpr int LAS_MAXW = 32;
constexpr int LAS_RB = 8;                           // rows whose strips and location features are formed in one pass
constexpr int LAS_FPW = LAS_TT / 4;                 // frames of a tile per wave
constexpr int LAS_SLD = LAS_STRIP + 1;              // row stride of the strips in LDS: the (row, 8-frame group) windows of a wave fall in different banks
constexpr int LAS_CH = 256;                         // frames per chunk of soft-max weights in the context pass (one per thread and row)

template <typename T> __device__ __forceinline__ float exp_t(float x) {
  if constexpr (sizeof(T) == 4) return expf(x); else return __expf(x);
}

// the live rows of search s and its frames; false: the search is skipped (finished, nothing alive, or offsets out of range).
// CELLS: the frames are those of utterance sutt[s] of U (moff has U + 1 entries); a sutt[s] outside 0 .. U - 1 skips the search
template <bool CELLS>
__device__ __forceinline__ bool las_search(const emoasr_beam_state_t* state, const int* moff, const int* sutt, int U, int s, int W,
                                           int Tmax, int rows, int& na, long& r0, int& Ts) {
  const emoasr_beam_state_t st = state[s];
  if (st.done) return false;
  na = min(st.n_alive, W);
  if (na < 1) return false;
  int u = s;
  if constexpr (CELLS) {
    u = sutt[s];
    if (u < 0 || u >= U) return false;
  }
  r0 = moff[u];
  Ts = moff[u + 1] - moff[u];
  return r0 >= 0 && Ts >= 1 && Ts <= Tmax && r0 + Ts <= (long)rows;
}

__device__ __forceinline__ int las_parent(const int* parent, int R, int W, int w) {
  const int p = parent[R + w];
  return (p >= R && p < R + W) ? p : R;
}

template <typename T, bool CELLS>
__global__ __launch_bounds__(256) void las_group_score_kernel(const emoasr_las_attend_group_t a, const int* sutt, int U) {
  __shared__ float s_filt[LAS_C * LAS_K];
  __shared__ float s_strip[LAS_RB][LAS_SLD];
  __shared__ float s_feat[LAS_RB][LAS_TT * LAS_C];
  __shared__ int s_par[LAS_MAXW];
  const int s = blockIdx.y, t0 = blockIdx.x * LAS_TT, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int na, Ts;
  long r0;
  if (!las_search<CELLS>(a.state, a.moff, sutt, U, s, a.W, a.Tmax, a.rows, na, r0, Ts)) return;   // (block-uniform)
  if (t0 >= Ts) return;
  const int R = s * a.W;
  for (int j = tid; j < LAS_C * LAS_K; j += 256) s_filt[j] = a.filt[j];
  if (tid < na) s_par[tid] = las_parent(a.parent, R, a.W, tid);
  const int a0 = lane * 8;
  const bool act = a0 < a.A;
  // the lane's 8 channels of the wave's 8 frames of the tile, once for all rows; W_conv, b_conv and w_score likewise
  float pkr[LAS_FPW][8], wc[8][LAS_C], ws[8], bc[8];
  const T* pk = static_cast<const T*>(a.pk) + r0 * a.A;
#pragma unroll
  for (int i = 0; i < LAS_FPW; ++i) {
    const int t = t0 + wave + 4 * i;
    if (act && t < Ts) {
      load8<T>(pk + (long)t * a.A + a0, pkr[i]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) pkr[i][e] = 0.f;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bc[e] = act ? a.b_conv[a0 + e] : 0.f;
    ws[e] = act ? a.w_score[a0 + e] : 0.f;
#pragma unroll
    for (int c = 0; c < LAS_C; ++c) wc[e][c] = act ? a.w_conv[(a0 + e) * LAS_C + c] : 0.f;
  }
  for (int w0 = 0; w0 < na; w0 += LAS_RB) {
    const int nr = min(LAS_RB, na - w0);
    __syncthreads();   // (the previous pass has read s_feat; the first pass: s_filt and s_par are written)
    // the strips aw_src[parent][t0 - 100 .. t0 + 32 + 100), zero outside the search's frames
    for (int x = tid; x < nr * LAS_STRIP; x += 256) {
      const int r = x / LAS_STRIP, j = x - r * LAS_STRIP;
      const int t = t0 - LAS_HALO + j;
      s_strip[r][j] = (t >= 0 && t < Ts) ? a.aw_src[(long)s_par[w0 + r] * a.Tmax + t] : 0.f;
    }
    __syncthreads();
    // location features: a task is (row, channel, 8 consecutive frames).  The 8 sums slide over the strip together: per 8 filter
    // taps 8 new strip values and 8 taps are read for 64 products, each sum still adds its taps in ascending order
    // (las_feat's order, csrc/las.hip)
    for (int x = tid; x < nr * LAS_C * (LAS_TT / 8); x += 256) {
      const int c = x % LAS_C, q = (x / LAS_C) % (LAS_TT / 8), r = x / (LAS_C * (LAS_TT / 8));
      const float* fl = s_filt + c * LAS_K;
      const float* sp = s_strip[r] + q * 8;
      float acc[8], win[16];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[j] = 0.f;
        win[j] = sp[j];
      }
      for (int kc = 0; kc + 8 <= LAS_K; kc += 8) {   // taps kc .. kc + 7 read sp[kc .. kc + 14]
#pragma unroll
        for (int j = 0; j < 8; ++j) win[8 + j] = sp[kc + 8 + j];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const float f = fl[kc + kk];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += f * win[kk + j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) win[j] = win[8 + j];
      }
      static_assert(LAS_K % 8 == 1, "one tap is left after the chunks of 8");
      {
        const float f = fl[LAS_K - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f * win[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s_feat[r][(q * 8 + j) * LAS_C + c] = acc[j];
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const long row = R + w0 + r;
      float pqb[8];
      if (act) {
        load8<T>(static_cast<const T*>(a.pq) + row * a.A + a0, pqb);
#pragma unroll
        for (int e = 0; e < 8; ++e) pqb[e] += bc[e];
      }
#pragma unroll
      for (int i = 0; i < LAS_FPW; ++i) {
        const int tt = wave + 4 * i, t = t0 + tt;
        if (t < Ts) {   // (wave-uniform)
          float part = 0.f;
          if (act) {
            float f[LAS_C];
#pragma unroll
            for (int c = 0; c < LAS_C; ++c) f[c] = s_feat[r][tt * LAS_C + c];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float x = pkr[i][e] + pqb[e];
#pragma unroll
              for (int c = 0; c < LAS_C; ++c) x += wc[e][c] * f[c];
              part += ws[e] * tanh_t<T>(x);
            }
          }
          part = wave_sum(part);
          if (lane == 0) a.scores[row * a.Tmax + t] = part;
        }
      }
    }
  }
}

// WB: W rounded up to 8 / 16 / 24 / 32 -- the (row, column) accumulators of a thread have compile-time bounds
template <typename T, int WB, bool CELLS>
__global__ __launch_bounds__(256) void las_group_ctx_kernel(const emoasr_las_attend_group_t a, const int* sutt, int U) {
  __shared__ float s_m[LAS_MAXW], s_inv[LAS_MAXW];
  __shared__ float s_w[WB][LAS_CH];
  __shared__ float s_acc[32][LAS_CTX_COLS + 1];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int na, Ts;
  long r0;
  if (!las_search<CELLS>(a.state, a.moff, sutt, U, s, a.W, a.Tmax, a.rows, na, r0, Ts)) return;   // (block-uniform)
  const int R = s * a.W;
  // the soft-max statistics of every live row: one wave per row
  for (int w = wave; w < na; w += 4) {
    const float* sc = a.scores + (long)(R + w) * a.Tmax;
    float m = -FLT_MAX;
    for (int t = lane; t < Ts; t += 64) m = fmaxf(m, sc[t]);
    m = wave_max(m);
    float sum = 0.f;
    for (int t = lane; t < Ts; t += 64) sum += exp_t<T>(sc[t] - m);
    sum = wave_sum(sum);
    if (lane == 0) {
      s_m[w] = m;
      s_inv[w] = 1.f / sum;
    }
  }
  const int dg = tid & 7, tl = tid >> 3;
  const int d0 = blockIdx.x * LAS_CTX_COLS + dg * 8;
  const T* eo = static_cast<const T*>(a.eouts) + r0 * a.D;
  float acc[WB][8];
#pragma unroll
  for (int w = 0; w < WB; ++w)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[w][e] = 0.f;
  // per chunk of 256 frames: the weights of all rows into LDS (thread j forms frame tb + j of every live row), then the frames'
  // eouts rows without a barrier between them, so that their loads overlap
  for (int tb = 0; tb < Ts; tb += LAS_CH) {
    __syncthreads();   // (the previous chunk's weights are consumed; the first chunk: the statistics are written)
    {
      const int t = tb + tid;
#pragma unroll
      for (int w = 0; w < WB; ++w) {
        float v = 0.f;
        if (w < na && t < Ts) {
          v = exp_t<T>(a.scores[(long)(R + w) * a.Tmax + t] - s_m[w]) * s_inv[w];
          if (blockIdx.x == 0) a.aw_dst[(long)(R + w) * a.Tmax + t] = v;
        }
        s_w[w][tid] = v;
      }
    }
    __syncthreads();
    const int tend = min(Ts, tb + LAS_CH);
    if (d0 < a.D) {
      for (int t = tb + tl; t < tend; t += 32) {
        float v[8];
        load8<T>(eo + (long)t * a.D + d0, v);   // one fetch for the W rows
#pragma unroll
        for (int w = 0; w < WB; ++w) {
          const float wt = s_w[w][t - tb];
          if (wt != 0.f) {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[w][e] += wt * v[e];
          }
        }
      }
    }
  }
#pragma unroll
  for (int w = 0; w < WB; ++w) {
    if (w < na) {   // (block-uniform)
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 8; ++e) s_acc[tl][dg * 8 + e] = acc[w][e];
      __syncthreads();
      if (tid < LAS_CTX_COLS) {
        float t = 0.f;
        for (int r = 0; r < 32; ++r) t += s_acc[r][tid];
        const int d = blockIdx.x * LAS_CTX_COLS + tid;
        if (d < a.D) static_cast<T*>(a.ctx)[(long)(R + w) * a.ctx_ld + d] = from_f32<T>(t);
      }
    }
  }
}

__global__ __launch_bounds__(256) void las_state_gather_kernel(const emoasr_las_state_gather_t g) {
  const int r = blockIdx.x, s = r / g.W, w = r - s * g.W;
  const emoasr_beam_state_t st = g.state[s];
  if (st.done || w >= st.n_alive) return;   // (block-uniform)
  const int p = las_parent(g.parent, s * g.W, g.W, w);
  const emoasr_las_gather_item_t it = g.item[blockIdx.y];
  const uint4* src = reinterpret_cast<const uint4*>(static_cast<const char*>(it.src) + (long)p * it.row_bytes);
  uint4* dst = reinterpret_cast<uint4*>(static_cast<char*>(it.dst) + (long)r * it.row_bytes);
  const int n16 = (int)(it.row_bytes / 16);
  for (int i = threadIdx.x; i < n16; i += 256) dst[i] = src[i];
}

}  // namespace

namespace {

// the argument checks and the two launches of emoasr_las_attend_group / _cells (`name` goes into the messages)
template <bool CELLS>
int las_attend_launch(const char* name, int dtype, const emoasr_las_attend_group_t* a, const int* sutt, int U, void* stream) {
  EMO_CHECK(a->W >= 1 && a->W <= LAS_MAXW, "%s: group size %d outside 1..32", name, a->W);
  EMO_CHECK(a->A > 0 && a->A % 8 == 0 && a->A <= LAS_MAX_A, "%s: attn_dim A=%d must be a multiple of 8, at most %d", name, a->A,
            LAS_MAX_A);
  EMO_CHECK(a->D > 0 && a->D % 8 == 0, "%s: enc_hidden_size D=%d must be a multiple of 8", name, a->D);
  EMO_CHECK(a->S >= 1 && a->S <= 65535, "%s: %d searches (1..65535)", name, a->S);
  EMO_CHECK(a->Tmax >= 1 && a->rows >= 1, "%s: Tmax=%d, rows=%d", name, a->Tmax, a->rows);
  EMO_CHECK(a->pk && a->eouts && a->moff && a->pq && a->aw_src && a->parent && a->state && a->filt && a->w_conv && a->b_conv &&
                a->w_score && a->scores && a->aw_dst && a->ctx,
            "%s: NULL operand", name);
  EMO_CHECK(a->ctx_ld >= a->D && a->ctx_ld % 8 == 0, "%s: ctx_ld=%ld", name, a->ctx_ld);
  EMO_CHECK((((size_t)a->pk | (size_t)a->eouts | (size_t)a->pq | (size_t)a->ctx) & 15) == 0,
            "%s: pk, eouts, pq and ctx must be 16-byte aligned", name);
  hipStream_t s = (hipStream_t)stream;
  const dim3 g1(cdiv(a->Tmax, LAS_TT), a->S), g2(cdiv(a->D, LAS_CTX_COLS), a->S);
  EMO_DISPATCH(dtype, (las_group_score_kernel<T, CELLS><<<g1, 256, 0, s>>>(*a, sutt, U)));
  EMO_LAUNCH_CHECK();
  const int wb = (a->W + 7) / 8;
  EMO_DISPATCH(dtype, {
    if (wb == 1) las_group_ctx_kernel<T, 8, CELLS><<<g2, 256, 0, s>>>(*a, sutt, U);
    else if (wb == 2) las_group_ctx_kernel<T, 16, CELLS><<<g2, 256, 0, s>>>(*a, sutt, U);
    else if (wb == 3) las_group_ctx_kernel<T, 24, CELLS><<<g2, 256, 0, s>>>(*a, sutt, U);
    else las_group_ctx_kernel<T, 32, CELLS><<<g2, 256, 0, s>>>(*a, sutt, U);
  });
  EMO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int emoasr_las_attend_group(int dtype, const emoasr_las_attend_group_t* a, void* stream) {
  EMO_CHECK(a, "las_attend_group: missing arguments");
  return las_attend_launch<false>("las_attend_group", dtype, a, nullptr, 0, stream);
}

extern "C" int emoasr_las_attend_cells(int dtype, const emoasr_las_attend_cells_t* c, void* stream) {
  EMO_CHECK(c && c->sutt, "las_attend_cells: missing arguments");
  EMO_CHECK(c->U >= 1 && c->U <= c->g.S, "las_attend_cells: %d utterances for %d searches (1 .. searches)", c->U, c->g.S);
  return las_attend_launch<true>("las_attend_cells", dtype, &c->g, c->sutt, c->U, stream);
}

/* host-side check of a search -> utterance map before it is uploaded: every entry inside 0 .. U - 1, the searches of one utterance
 * consecutive and the utterances in order, every utterance searched at least once */
extern "C" int emoasr_las_cells_check(int S, const int* sutt_host, int U) {
  EMO_CHECK(sutt_host && S >= 1 && U >= 1 && U <= S, "las cells: missing map, or %d utterances for %d searches", U, S);
  EMO_CHECK(sutt_host[0] == 0, "las cells: search 0 belongs to utterance %d (the map starts at utterance 0)", sutt_host[0]);
  for (int s = 1; s < S; ++s) {
    const int d = sutt_host[s] - sutt_host[s - 1];
    EMO_CHECK(d == 0 || d == 1, "las cells: search %d belongs to utterance %d after utterance %d (searches of one utterance are "
              "consecutive, utterances in order)", s, sutt_host[s], sutt_host[s - 1]);
  }
  EMO_CHECK(sutt_host[S - 1] == U - 1, "las cells: the map ends at utterance %d of %d", sutt_host[S - 1], U);
  return 0;
}

extern "C" int emoasr_las_state_gather(const emoasr_las_state_gather_t* g, void* stream) {
  EMO_CHECK(g && g->parent && g->state, "las_state_gather: missing arguments");
  EMO_CHECK(g->W >= 1 && g->W <= LAS_MAXW, "las_state_gather: group size %d outside 1..32", g->W);
  EMO_CHECK(g->S >= 1 && (long)g->S * g->W <= 0x7fffffffL, "las_state_gather: %d searches", g->S);
  EMO_CHECK(g->n >= 1 && g->n <= EMOASR_LAS_GATHER_MAX, "las_state_gather: %d arrays (1..%d)", g->n, EMOASR_LAS_GATHER_MAX);
  for (int k = 0; k < g->n; ++k) {
    const emoasr_las_gather_item_t& it = g->item[k];
    EMO_CHECK(it.src && it.dst && it.row_bytes >= 16 && it.row_bytes % 16 == 0 && (((size_t)it.src | (size_t)it.dst) & 15) == 0,
              "las_state_gather: array %d needs 16-byte aligned pointers and rows of a multiple of 16 bytes (row_bytes=%ld)", k,
              it.row_bytes);
  }
  las_state_gather_kernel<<<dim3(g->S * g->W, g->n), 256, 0, (hipStream_t)stream>>>(*g);
  EMO_LAUNCH_CHECK();
  return 0;
}
