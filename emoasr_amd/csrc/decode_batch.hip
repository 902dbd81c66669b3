// Kernels of the BATCHED joint CTC / attention beam search (modeling/beam_search_device.py:joint_beam_search_device_batch):
// S searches of width W occupy rows s * W .. s * W + W - 1 of every per-hypothesis array and step in lockstep.
//   * emoasr_attn_step_group: single-query cross-attention of the W hypotheses of a search against that search's OWN
//     projected memory [T_s, 2 dd] -- the memory is stored once per utterance (no per-beam replica), and a K / V tile is
//     fetched once for all W queries;
//   * emoasr_beam_update_batch: beam_update_kernel (csrc/decode_rt.hip) with one workgroup per search, and a one-thread
//     tail launch that advances the shared output position and writes the host's mirror.
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

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

// One workgroup per (search s, head h).  LDS: the W queries (f32), one tile of TK keys and values (f32; the key rows padded by
// one float so that the TK lanes of a score column hit TK banks), the W x TK scores / probabilities and the running (max, sum,
// rescale) of every query.  Per tile: scores (a thread owns one key j and the queries w0, w0 + 256 / TK, ...: the key element is
// read once for all of them), the online soft-max update by 8 lanes per query, then P . V into the thread's own (query, column)
// accumulators (one column, the queries w1, w1 + 256 / DK, ...: the value element is read once for all of them).  The next
// tile's 16-byte chunks are fetched into registers before the current tile is computed.  Everything a row sees is its own
// search's memory in tiles counted from that memory's first row, so a row's bits do not depend on S or on the other searches of
// the launch.
template <typename T, int DK, int TK, int WB>
__global__ __launch_bounds__(G_THREADS) void attn_step_group_kernel(int W, int H, const T* __restrict__ q, const T* __restrict__ kv,
                                                                    const int* __restrict__ moff, float scale, T* __restrict__ out) {
  // WB: the group size rounded up to 8 / 16 / 24 / 32 -- the loops over a thread's queries have compile-time bounds and no
  // branches (queries W .. WB - 1 are zero rows whose results are never written)
  constexpr int NACC = WB * DK / G_THREADS;       // (query, column) accumulators per thread
  constexpr int WSTEP = G_THREADS / DK;           // ... their queries are WSTEP apart
  constexpr int NSC = WB * TK / G_THREADS;        // (query, key) scores per thread
  constexpr int SSTEP = G_THREADS / TK;
  constexpr int VN = Chunk16<T>::N;
  constexpr int CH = DK / VN;                     // chunks of a K (or V) row
  constexpr int NCH = TK * CH / G_THREADS;        // chunks of a K (or V) tile per thread
  static_assert(NACC * G_THREADS == WB * DK && NSC * G_THREADS == WB * TK && WB % 8 == 0 && WB <= G_MAXW && NCH * G_THREADS == TK * CH && NCH >= 1, "tiling");
  __shared__ float s_q[WB][DK];
  __shared__ float s_k[TK][DK + 1];
  __shared__ float s_v[TK][DK];
  __shared__ float s_p[WB][TK];
  __shared__ float s_m[G_MAXW], s_l[G_MAXW], s_a[G_MAXW];
  const int s = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
  const int dd = H * DK;
  const long r0 = moff[s];
  const int Ts = moff[s + 1] - moff[s];
  Chunk16<T> ck[NCH], cv[NCH];
  auto fetch = [&](int t0) {   // rows t0 .. t0 + TK - 1 of the search (zero past its end)
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int x = tid + k * G_THREADS, j = x / CH, cc = x - j * CH;
      if (t0 + j < Ts) {
        const T* row = kv + (r0 + t0 + j) * 2 * dd + h * DK + cc * VN;
        ck[k] = *reinterpret_cast<const Chunk16<T>*>(row);
        cv[k] = *reinterpret_cast<const Chunk16<T>*>(row + dd);
      } else {
        ck[k].zero();
        cv[k].zero();
      }
    }
  };
  fetch(0);
  for (int i = tid; i < WB * DK; i += G_THREADS) {
    const int w = i / DK, c = i - w * DK;
    s_q[w][c] = w < W ? to_f32(q[((long)s * W + w) * dd + h * DK + c]) : 0.f;
  }
  if (tid < G_MAXW) { s_m[tid] = -INFINITY; s_l[tid] = 0.f; s_a[tid] = 0.f; }
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  const int pc = tid % DK, pw = tid / DK;    // P . V: the thread's column and first query
  const int sj = tid % TK, sw = tid / TK;    // scores: the thread's key and first query
  for (int t0 = 0; t0 < Ts; t0 += TK) {
    const int n = min(TK, Ts - t0);
    __syncthreads();                         // (the previous tile's P . V has read s_v / s_p; the first pass: s_q is written)
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int x = tid + k * G_THREADS, j = x / CH, cc = x - j * CH;
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        s_k[j][cc * VN + e] = ck[k].get(e);
        s_v[j][cc * VN + e] = cv[k].get(e);
      }
    }
    if (t0 + TK < Ts) fetch(t0 + TK);        // in flight while this tile is computed
    __syncthreads();
    {
      // per (query, key): four interleaved partial sums (shorter chains: less rounding), the scale once at the end
      float d[NSC][4];
#pragma unroll
      for (int k = 0; k < NSC; ++k) d[k][0] = d[k][1] = d[k][2] = d[k][3] = 0.f;
      for (int c = 0; c < DK; c += 4) {
        const float k0 = s_k[sj][c], k1 = s_k[sj][c + 1], k2 = s_k[sj][c + 2], k3 = s_k[sj][c + 3];
#pragma unroll
        for (int k = 0; k < NSC; ++k) {
          const int w = sw + k * SSTEP;
          d[k][0] = fmaf(s_q[w][c], k0, d[k][0]);
          d[k][1] = fmaf(s_q[w][c + 1], k1, d[k][1]);
          d[k][2] = fmaf(s_q[w][c + 2], k2, d[k][2]);
          d[k][3] = fmaf(s_q[w][c + 3], k3, d[k][3]);
        }
      }
#pragma unroll
      for (int k = 0; k < NSC; ++k) {
        const int w = sw + k * SSTEP;
        s_p[w][sj] = sj < n ? ((d[k][0] + d[k][1]) + (d[k][2] + d[k][3])) * scale : -INFINITY;
      }
    }
    __syncthreads();
    {  // 8 lanes per query (the 8 lanes are neighbours inside one wave)
      const int w = tid >> 3, sub = tid & 7;
      if (w < W) {
        float mx = -INFINITY;
        for (int j = sub; j < TK; j += 8) mx = fmaxf(mx, s_p[w][j]);
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        mx = fmaxf(mx, __shfl_xor(mx, 4));
        const float m_old = s_m[w];
        const float m_new = fmaxf(m_old, mx);   // finite: every tile holds at least one valid key
        float sum = 0.f;
        for (int j = sub; j < TK; j += 8) {
          const float p = expf(s_p[w][j] - m_new);   // (masked: exp(-inf) = 0)
          s_p[w][j] = p;
          sum += p;
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        if (sub == 0) {
          const float a = expf(m_old - m_new);       // (first tile: exp(-inf) = 0)
          s_a[w] = a;
          s_l[w] = s_l[w] * a + sum;
          s_m[w] = m_new;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      acc[i] *= s_a[pw + i * WSTEP];
    }
    for (int j = 0; j < n; ++j) {            // (keys in ascending order into every accumulator)
      const float v = s_v[j][pc];
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        acc[i] = fmaf(s_p[pw + i * WSTEP][j], v, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int w = pw + i * WSTEP;
    if (w < W) out[((long)s * W + w) * dd + h * DK + pc] = from_f32<T>(acc[i] / s_l[w]);
  }
}

template <typename T>
int launch_group(int S, int W, int H, int dk, const void* q, const void* kv, const int* moff, float scale, void* out, hipStream_t s) {
  dim3 grid(S, H);
#define EMO_GROUP_LAUNCH(DK, TK, WB) \
  attn_step_group_kernel<T, DK, TK, WB><<<grid, G_THREADS, 0, s>>>(W, H, (const T*)q, (const T*)kv, moff, scale, (T*)out)
#define EMO_GROUP_CASE(DK, TK)                 \
  case DK:                                     \
    if (W <= 8) EMO_GROUP_LAUNCH(DK, TK, 8);   \
    else if (W <= 16) EMO_GROUP_LAUNCH(DK, TK, 16); \
    else if (W <= 24) EMO_GROUP_LAUNCH(DK, TK, 24); \
    else EMO_GROUP_LAUNCH(DK, TK, 32);         \
    break;
  switch (dk) {
    EMO_GROUP_CASE(32, 64)
    EMO_GROUP_CASE(64, 64)
    EMO_GROUP_CASE(128, 32)
    default:
      emo_set_error("attn_step_group: head width %d (supported: 32, 64, 128)", dk);
      return 1;
  }
#undef EMO_GROUP_CASE
#undef EMO_GROUP_LAUNCH
  return 0;
}

}  // namespace

extern "C" int emoasr_attn_step_group(int dtype, int S, int W, int dd, int H, const void* q, const void* kv, const int* moff,
                                      void* out, void* stream) {
  EMO_CHECK(q && kv && moff && out, "attn_step_group: missing arguments");
  EMO_CHECK(S >= 1 && W >= 1 && W <= G_MAXW, "attn_step_group: %d searches, group size %d outside 1..32", S, W);
  EMO_CHECK(H >= 1 && dd % H == 0, "attn_step_group: dd=%d H=%d", dd, H);
  EMO_CHECK(((size_t)kv & 15) == 0, "attn_step_group: the memory must be 16-byte aligned");
  const float scale = 1.f / sqrtf((float)(dd / H));
  EMO_DISPATCH(dtype, if (launch_group<T>(S, W, H, dd / H, q, kv, moff, scale, out, (hipStream_t)stream)) return 1);
  EMO_LAUNCH_CHECK();
  return 0;
}

/* host-side check of the row offsets of a launch (the callers hold them on the host before the upload) */
extern "C" int emoasr_group_offsets_check(int S, const int* moff_host) {
  EMO_CHECK(moff_host && S >= 1, "group offsets: missing");
  EMO_CHECK(moff_host[0] >= 0, "group offsets: first offset %d", moff_host[0]);
  for (int s = 0; s < S; ++s)
    EMO_CHECK(moff_host[s + 1] - moff_host[s] >= 1, "group offsets: search %d has %d rows (offsets must rise, T_s >= 1)", s,
              moff_host[s + 1] - moff_host[s]);
  return 0;
}

// ---- beam bookkeeping, one workgroup per search ------------------------------------------------------------------------
namespace {

// beam_update_kernel (csrc/decode_rt.hip) for search s = blockIdx.x: the same arithmetic in the same order on rows
// s * bw .. s * bw + bw - 1.  n_parent is the GLOBAL row of the parent (emoasr_beam_cache_gather and the CTC scorer index
// all nb rows); n_pcand, the history and res_parent stay local to the search.  The position is the shared word *u.pos: the
// workgroups only read it, beam_batch_tail_kernel advances it after all of them.
__global__ __launch_bounds__(256) void beam_update_batch_kernel(emoasr_beam_update_batch_t b) {
  __shared__ float sc[32][32];
  __shared__ int sel_j[32][32];
  __shared__ double cscore[1024];
  __shared__ int c_m[1024], c_j[1024];
  __shared__ int sorted_e[32];
  const emoasr_beam_update_t& u = b.u;
  const int s = blockIdx.x;
  emoasr_beam_state_t* st = u.state + s;
  const int pos = *b.pos;
  if (st->done || pos >= b.max_pos) return;   // (max_pos: the rows of the history and of the caches)
  const int tid = threadIdx.x;
  const int bw = u.bw, cw = u.cw, na = st->n_alive;
  const int R = s * bw;                 // first global row of the search
  const float* vals = u.vals + (long)R * cw;
  const int* cands = u.cands + (long)R * cw;
  const float* psi = u.psi ? u.psi + (long)R * cw : nullptr;
  const float* lm_at = u.lm_at ? u.lm_at + (long)R * cw : nullptr;
  double* score = u.score + R;
  float* score_ctc = u.score_ctc + R;
  const float f1 = u.one_minus_lam, fl = u.lam, fm = u.mu;
  for (int i = tid; i < na * cw; i += 256) {
    const int m = i / cw, j = i - m * cw;
    float v;
    if (psi) {
      v = f1 * vals[m * cw + j] + fl * (psi[m * cw + j] - score_ctc[m]);
      if (lm_at) v = v + fm * lm_at[m * cw + j];
    } else {
      v = vals[m * cw + j];
    }
    sc[m][j] = v;
  }
  __syncthreads();
  const int keep = min(bw, cw);
  for (int i = tid; i < na * cw; i += 256) {
    const int m = i / cw, j = i - m * cw;
    const float v = sc[m][j];
    int r = 0;
    for (int k = 0; k < cw; ++k) r += (sc[m][k] > v) || (sc[m][k] == v && k < j);
    if (r < keep) sel_j[m][r] = j;
  }
  __syncthreads();
  const int nc = na * keep;
  for (int e = tid; e < nc; e += 256) {
    const int m = e / keep, r = e - m * keep, j = sel_j[m][r];
    c_m[e] = m; c_j[e] = j;
    cscore[e] = score[m] + (double)sc[m][j];
  }
  __syncthreads();
  for (int e = tid; e < nc; e += 256) {
    const double v = cscore[e];
    int r = 0;
    for (int k = 0; k < nc; ++k) r += (cscore[k] > v) || (cscore[k] == v && k < e);
    if (r < bw) sorted_e[r] = e;
  }
  __syncthreads();
  if (tid != 0) return;
  int a = 0, nres = st->n_results;
  const int nsel = min(bw, nc);
  int* hp = u.hist_parent + ((long)pos * b.S + s) * bw;
  int* ht = u.hist_token + ((long)pos * b.S + s) * bw;
  int *n_ids = u.n_ids + R, *n_parent = u.n_parent + R, *n_pcand = u.n_pcand + R;
  for (int r = 0; r < nsel; ++r) {
    const int e = sorted_e[r], m = c_m[e], j = c_j[e];
    const int tok = cands[m * cw + j];
    if (tok == u.eos) {
      if (pos < 1) continue;  // empty hypothesis
      u.res_score[R + nres] = cscore[e] + u.len_weight * (double)(pos + 2);
      u.res_step[R + nres] = pos;
      u.res_parent[R + nres] = m;
      ++nres;
      if (nres >= bw) break;
    } else {
      n_ids[a] = tok; n_parent[a] = R + m; n_pcand[a] = j;
      score[a] = cscore[e];
      score_ctc[a] = psi ? psi[m * cw + j] : 0.f;
      hp[a] = m; ht[a] = tok;
      ++a;
    }
  }
  for (int k = a; k < bw; ++k) {  // unused slots: copies of the search's slot 0
    n_ids[k] = a > 0 ? n_ids[0] : u.eos;
    n_parent[k] = a > 0 ? n_parent[0] : R;
    n_pcand[k] = a > 0 ? n_pcand[0] : 0;
    score[k] = 0.0; score_ctc[k] = 0.f;
    hp[k] = -1; ht[k] = -1;
  }
  for (int k = 0; k < bw; ++k) {
    u.n_last[R + k] = n_ids[k];
    u.n_outlen[R + k] = pos + 1;
    u.n_klens[R + k] = pos + 2;
  }
  st->n_alive = a;
  st->n_results = nres;
  st->done = (nres >= bw || a == 0) ? 1 : 0;
  st->pos = pos + 1;
}

// After the S workgroups of a step (stream order): advance the shared position once and tell the host.  ctl = {all searches
// finished}.  A step replayed after the end finds ctl[0] set and changes nothing.
__global__ void beam_batch_tail_kernel(emoasr_beam_update_batch_t b) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (b.ctl[0] || *b.pos >= b.max_pos) return;
  int nd = 0;
  for (int s = 0; s < b.S; ++s) nd += b.u.state[s].done ? 1 : 0;
  const int pos = *b.pos + 1;
  *b.pos = pos;
  if (nd == b.S) b.ctl[0] = 1;
  if (b.u.host_mirror) {   // payload first, the position last
    volatile int* hm = b.u.host_mirror;
    hm[1] = nd;
    __threadfence_system();
    hm[0] = pos;
    __threadfence_system();
  }
}

}  // namespace

extern "C" int emoasr_beam_update_batch(const emoasr_beam_update_batch_t* b, void* stream) {
  EMO_CHECK(b && b->pos && b->ctl && b->u.state && b->u.vals && b->u.cands && b->u.score && b->u.n_ids, "beam_update_batch: missing arguments");
  EMO_CHECK(b->S >= 1 && b->max_pos >= 1, "beam_update_batch: %d searches, %d positions", b->S, b->max_pos);
  EMO_CHECK(b->u.bw >= 1 && b->u.bw <= 32 && b->u.cw >= 1 && b->u.cw <= 32, "beam_update_batch: beam %d / candidates %d outside 1..32",
            b->u.bw, b->u.cw);
  beam_update_batch_kernel<<<b->S, 256, 0, (hipStream_t)stream>>>(*b);
  beam_batch_tail_kernel<<<1, 64, 0, (hipStream_t)stream>>>(*b);
  EMO_LAUNCH_CHECK();
  return 0;
}
