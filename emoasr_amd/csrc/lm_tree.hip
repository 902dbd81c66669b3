// Transformer-LM shallow fusion inside the batched transducer beam search, over a PREFIX TREE (engine.rnnt_beam_search_batch with a
// Transformer LM under decoder.rnnt_tlm_fusion = "device").  Hypotheses of the transducer search grow at
// different rates and their states live in recycled slots, so the dense per-beam K / V caches of the joint search (csrc/decode_rt.hip)
// do not carry over: a dense cache per slot would be slots x Lmax x layers x d x 2 values per search.  Here every token a hypothesis
// appends is one NODE whose K / V rows are written once and never copied, a slot holds the list of node ids of its prefix, and the
// self-attention of a row reads K / V gathered through that list:
//
//   emoasr_lm_tree_advance   per round: a fresh node per live row (compact, counted by one wave per search: no atomics), the list of
//                            the source slot copied to the destination slot and extended by the node, (node, position) per row
//   emoasr_lm_tree_attn      single-query attention of row i against the keys / values at the nodes of lanc[dst[i]], the new key /
//                            value written at the row's node first; the gathered twin of attn_step_kernel (csrc/rowlin.hip)
//   emoasr_lm_tree_step      the launch chain of emoasr_bert_lm_step (csrc/decode_rt.hip) for R rows: per-row positions, the kernel
//                            above in place of the cache append + dense attention, raw logits in the compute dtype
//
// The fused CTC search (csrc/ctc_beam_lm.hip) drives the same tree under decoder.ctc_tlm_fusion = "device" (DESIGN.md section 32): its
// pool rows are the slots, its record list (one record per new prefix) the rows of a step:
//
//   emoasr_lm_tree_advance_rec    advance from the record list and its count as they lie on the device: one wave per record, a node
//                                 per record by atomicAdd on the search's counter, the control words lab / dst for the two kernels above
//   emoasr_lm_tree_attn_rows / emoasr_lm_tree_step_rows    the two kernels above over the first R rows (they are these with R = S W)
//   emoasr_log_softmax_rows_to    the step's raw logits, normalised over the LM's whole vocabulary by the body of emoasr_log_softmax
//                                 (csrc/log_softmax_body.h), scattered into the f32 pool rows the next frame reads
//
// The batched LAS search (engine/las.py) drives it under decoder.las_tlm_fusion = "device" (DESIGN.md section 33): the search is
// label-synchronous, a row of a step is its parent's prefix plus one token, and the slots are two halves of S W rows:
//
//   emoasr_lm_tree_advance_beam   advance from the lockstep book (ids, parent, state): one wave per search, nodes by ballot, the
//                                 control words lab / dst for the step; emoasr_log_softmax_rows_to then fills the f32 rows the score
//                                 kernel reads
//
// Bounds: every slot number, length, label and node id that arrives through device memory is checked or clamped before it is used as
// an index; a row that fails a check writes nothing.
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

// One wave per search.  Lane w < W owns row s W + w.
__global__ __launch_bounds__(64) void lm_tree_advance_kernel(const emoasr_lm_tree_t t, const long long* __restrict__ src,
                                                             const long long* __restrict__ dst,
                                                             const long long* __restrict__ active) {
  const int s = blockIdx.x, lane = threadIdx.x, W = t.W, Lcap = t.Lcap;
  const long r = (long)s * W + lane;
  long long sl = -1, dl = -1;
  int p = -1;
  bool live = false;
  if (lane < W) {
    sl = src[r]; dl = dst[r];
    live = active[r] != 0 && sl >= 0 && sl < t.nslots && dl >= 0 && dl < t.nslots;
    if (live) { p = t.llen[sl]; live = p >= 0; }
  }
  const bool over = live && p >= Lcap;              // the prefix would exceed Lcap
  const bool want = live && !over;
  const unsigned long long wants = __ballot(want);
  const int rank = __popcll(wants & ((1ull << lane) - 1ull));
  const int base = min(max(t.nnodes[s], 0), t.node_cap);
  const bool full = want && base + rank >= t.node_cap;
  const bool ok = want && !full;
  const int node = ok ? s * t.node_cap + base + rank : -1;
  const int bits = (__ballot(over) ? EMOASR_LM_TREE_OVERLEN : 0) | (__ballot(full) ? EMOASR_LM_TREE_POOL_FULL : 0);
  const int taken = __popcll(__ballot(ok));
  if (lane < W) { t.row_node[r] = node; t.row_pos[r] = ok ? p : 0; }
  // the lists: the wave copies row after row (lanc[src][:p] -> lanc[dst], then the node).  No live row's source slot is a
  // destination slot of this launch -- the book kernel's mark and sweep hands out as destinations only slots no live hypothesis
  // reads, the guarantee emoasr_rnnt_beam_lstm_rows relies on for the LSTM states -- so the copies of different rows (and of
  // different waves) do not overlap and need no order.
  for (int w = 0; w < W; ++w) {
    const int nd = __shfl(node, w, 64);
    if (nd < 0) continue;                           // (uniform over the wave)
    const int ss = __shfl((int)sl, w, 64), ds = __shfl((int)dl, w, 64), pw = __shfl(p, w, 64);
    const long so = (long)ss * Lcap, dn = (long)ds * Lcap;
    for (int i = lane; i < pw; i += 64) t.lanc[dn + i] = t.lanc[so + i];
    if (lane == 0) { t.lanc[dn + pw] = nd; t.llen[ds] = pw + 1; }
  }
  if (lane == 0) {
    t.nnodes[s] = base + taken;
    if (bits) t.status[s] |= bits;                  // (one writer per word: this wave)
  }
}

// The advance step under the RECORD LIST of the fused CTC search (csrc/ctc_beam_lm.hip): one wave per record,
// lanes striding the list copy.  The records of one search lie anywhere in the list, so a node is taken with one atomicAdd on the
// search's counter (which names the node, nothing else) and a bit is raised with atomicOr.  A share that is used up is put back by
// the wave that overdrew it: the counter never ends above node_cap, and no wave that reads it at or above node_cap takes a node.
__global__ __launch_bounds__(256) void lm_tree_advance_rec_kernel(const emoasr_lm_tree_t t, const int* __restrict__ rec, int rec_cap,
                                                                  const int* __restrict__ rec_count,
                                                                  const double* __restrict__ lm_weight,
                                                                  long long* __restrict__ lab, long long* __restrict__ dstw) {
  const int lane = threadIdx.x & 63, Lcap = t.Lcap;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rec_cap) return;                         // (uniform over the wave)
  const int n = min(max(rec_count[0], 0), rec_cap);
  const int per = t.nslots / t.S;                   // slots of one search's share
  int node = -1, p = 0, sl = -1, dl = -1;
  long long token = 0;
  if (r < n) {
    const int s = rec[r];
    token = rec[3 * (long)rec_cap + r];
    sl = rec[4 * (long)rec_cap + r];
    dl = rec[5 * (long)rec_cap + r];
    const bool in_share = s >= 0 && s < t.S && dl >= s * per && dl < (s + 1) * per && (sl < 0 || (sl >= s * per && sl < (s + 1) * per));
    if (in_share && !(lm_weight && !(lm_weight[s] > 0.0))) {      // (a search that fuses nothing takes no node)
      p = sl < 0 ? 0 : t.llen[sl];
      if (p < 0) {
        p = 0;                                      // a slot that holds no prefix: no effect
      } else if (p >= Lcap) {
        if (lane == 0) atomicOr(&t.status[s], EMOASR_LM_TREE_OVERLEN);
      } else {
        int got = -1;
        if (lane == 0) {
          const int old = atomicAdd(&t.nnodes[s], 1);
          if (old >= 0 && old < t.node_cap) got = s * t.node_cap + old;
          else { atomicSub(&t.nnodes[s], 1); atomicOr(&t.status[s], EMOASR_LM_TREE_POOL_FULL); }
        }
        node = __shfl(got, 0, 64);
      }
    }
  }
  if (node >= 0) {
    // no record's source slot is a destination slot of this launch (the frame kernel frees the row of a prefix that left the
    // beam only at the start of the next frame), so the copies of different waves do not overlap and need no order
    const long so = (long)sl * Lcap, dn = (long)dl * Lcap;
    for (int i = lane; i < p; i += 64) t.lanc[dn + i] = t.lanc[so + i];
    if (lane == 0) { t.lanc[dn + p] = node; t.llen[dl] = p + 1; }
  }
  if (lane == 0) {
    t.row_node[r] = node;
    t.row_pos[r] = node >= 0 ? p : 0;
    lab[r] = node >= 0 ? token : 0;
    dstw[r] = node >= 0 ? dl : -1;
  }
}

// The advance step under the LOCKSTEP BOOK of the batched LAS search (emoasr_beam_update_batch's ids / parent / state; DESIGN.md
// section 33): one wave per search, lane w < W owns row s W + w, nodes by ballot as in lm_tree_advance_kernel.  The slots are two
// halves of S W: row r reads slot src_base + parent' (its parent's row of the previous step) and writes slot dst_base + r.  Which
// rows are live is csrc/las_beam.hip's rule: the search is not done, w < n_alive, a parent outside the search's rows reads row 0.
__global__ __launch_bounds__(64) void lm_tree_advance_beam_kernel(const emoasr_lm_tree_t t, const int* __restrict__ ids,
                                                                  const int* __restrict__ parent,
                                                                  const emoasr_beam_state_t* __restrict__ state, int src_base,
                                                                  int dst_base, long long* __restrict__ lab,
                                                                  long long* __restrict__ dstw) {
  const int s = blockIdx.x, lane = threadIdx.x, W = t.W, Lcap = t.Lcap, R = s * W;
  const emoasr_beam_state_t st = state[s];
  const int na = st.done ? 0 : min(max(st.n_alive, 0), W);
  int sl = -1, dl = -1, p = -1;
  bool live = lane < na;                            // (nothing of a skipped row is read)
  if (live) {
    const int pr = parent[R + lane];
    sl = src_base + ((pr >= R && pr < R + W) ? pr : R);       // (the host checked both halves against nslots)
    dl = dst_base + R + lane;
    p = t.llen[sl];
    live = p >= 0;
  }
  const bool over = live && p >= Lcap;              // the prefix would exceed Lcap
  const bool want = live && !over;
  const unsigned long long wants = __ballot(want);
  const int rank = __popcll(wants & ((1ull << lane) - 1ull));
  const int base = min(max(t.nnodes[s], 0), t.node_cap);
  const bool full = want && base + rank >= t.node_cap;
  const bool ok = want && !full;
  const int node = ok ? s * t.node_cap + base + rank : -1;
  const int bits = (__ballot(over) ? EMOASR_LM_TREE_OVERLEN : 0) | (__ballot(full) ? EMOASR_LM_TREE_POOL_FULL : 0);
  const int taken = __popcll(__ballot(ok));
  if (lane < W) {
    t.row_node[R + lane] = node;
    t.row_pos[R + lane] = ok ? p : 0;
    lab[R + lane] = ok ? (long long)ids[R + lane] : 0;
    dstw[R + lane] = ok ? (long long)dl : -1;
  }
  // the lists, row after row: sources lie in one half of the slots, destinations in the other, so no copy reads what another writes
  for (int w = 0; w < W; ++w) {
    const int nd = __shfl(node, w, 64);
    if (nd < 0) continue;                           // (uniform over the wave)
    const int ss = __shfl(sl, w, 64), ds = __shfl(dl, w, 64), pw = __shfl(p, w, 64);
    const long so = (long)ss * Lcap, dn = (long)ds * Lcap;
    for (int i = lane; i < pw; i += 64) t.lanc[dn + i] = t.lanc[so + i];
    if (lane == 0) { t.lanc[dn + pw] = nd; t.llen[ds] = pw + 1; }
  }
  if (lane == 0) {
    t.nnodes[s] = base + taken;
    if (bits) t.status[s] |= bits;                  // (one writer per word: this wave)
  }
}

// pool[row_dst[r]][:V] = log_softmax(x[r, :V_lm])[:V] for the rows r < n that row_ok admits (NULL: all): the body of
// log_softmax_kernel (csrc/decoder.hip), so a row is bit-equal to emoasr_log_softmax's.  A row whose destination lies outside the
// pool is dropped.
template <typename T>
__global__ __launch_bounds__(256) void log_softmax_rows_to_kernel(int V, int Vout, const T* __restrict__ x, long ldx,
                                                                  const int* __restrict__ row_dst, const int* __restrict__ row_ok,
                                                                  float* __restrict__ out, long ldo, int out_rows) {
  __shared__ float red[16];
  const long m = blockIdx.x;
  const int o = row_dst[m];
  if (o < 0 || o >= out_rows || (row_ok && row_ok[m] < 0)) return;      // (uniform over the workgroup)
  const T* row = x + m * ldx;
#include "log_softmax_body.h"
  for (int v = threadIdx.x; v < Vout; v += 256) out[o * ldo + v] = to_f32(row[v]) - lse;
}

struct TreeAttnArgs {
  int R, d, dk, nslots, Lcap; long nodes;
  const void* qkv; void* kpool; void* vpool;        // pools of ONE layer: [nodes][d]
  const int* llen; const int* lanc; const int* row_node; const long long* dst;
  float scale; void* out;
};

// One wave per (row, head), the shape of attn_step_kernel: the node list staged once in LDS, 16-byte key loads, scores in LDS.  The
// new key / value take part from LDS (they are this wave's own stores: no read-after-write through memory).
template <typename T>
__global__ __launch_bounds__(64) void lm_tree_attn_kernel(const TreeAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = reinterpret_cast<float*>(smem);                 // [Lcap] scores / probabilities
  int* anc = reinterpret_cast<int*>(smem) + a.Lcap;           // [Lcap] node ids
  __shared__ float qs[128], ks[128], vs[128];
  const int r = blockIdx.x, h = blockIdx.y, lane = threadIdx.x, d = a.d, dk = a.dk;
  const int node = a.row_node[r];
  const long long slot = a.dst[r];
  if (node < 0 || node >= a.nodes || slot < 0 || slot >= a.nslots) return;      // (uniform over the wave)
  const int n = a.llen[slot];                                 // keys: the prefix with the new token
  if (n < 1 || n > a.Lcap) return;
  const T* row = static_cast<const T*>(a.qkv) + (long)r * 3 * d + h * dk;
  T* kp = static_cast<T*>(a.kpool) + h * dk;
  T* vp = static_cast<T*>(a.vpool) + h * dk;
  const int* list = a.lanc + (long)slot * a.Lcap;
  const int last = (int)a.nodes - 1;
  for (int t = lane; t < n - 1; t += 64) anc[t] = min(max(list[t], 0), last);
  for (int c = lane; c < dk; c += 64) {
    const T kn = row[d + c], vn = row[2 * d + c];
    qs[c] = to_f32(row[c]); ks[c] = to_f32(kn); vs[c] = to_f32(vn);
    kp[(long)node * d + c] = kn;
    vp[(long)node * d + c] = vn;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int t = lane; t < n; t += 64) {
    float s = 0.f;
    if (t < n - 1) {
      const T* kr = kp + (long)anc[t] * d;
      for (int c = 0; c < dk; c += 8) {
        float kv[8];
        load8<T>(kr + c, kv);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += qs[c + e] * kv[e];
      }
    } else {
      for (int c = 0; c < dk; ++c) s += qs[c] * ks[c];
    }
    s *= a.scale;
    sc[t] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float p = expf(sc[t] - mx);
    sc[t] = p;
    sum += p;
  }
  sum = wave_sum(sum);
  __syncthreads();
  const float inv = 1.f / sum;
  T* out = static_cast<T*>(a.out) + (long)r * d + h * dk;
  for (int c = lane; c < dk; c += 64) {
    float o = 0.f;
    for (int t = 0; t < n - 1; ++t) o += sc[t] * to_f32(vp[(long)anc[t] * d + c]);
    o += sc[n - 1] * vs[c];
    out[c] = from_f32<T>(o * inv);
  }
}

// x[i] = word_emb[clamp(lab[i])] + pe[row_pos[i]] for a row with a node, a zero row otherwise
template <typename T>
__global__ __launch_bounds__(256) void lm_tree_embed_kernel(int R, int d, int n_emb, int Lcap, const long long* __restrict__ lab,
                                                            const int* __restrict__ row_node, const int* __restrict__ row_pos,
                                                            const T* __restrict__ table, const float* __restrict__ pe,
                                                            T* __restrict__ out) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < (long)R * d; i += gridDim.x * 256L) {
    const int m = (int)(i / d), c = (int)(i - (long)m * d);
    float v = 0.f;
    if (row_node[m] >= 0) {
      const long id = (long)min(max(lab[m], 0LL), (long long)n_emb - 1);
      const int p = min(max(row_pos[m], 0), Lcap - 1);
      v = to_f32(table[id * d + c]) + pe[(long)p * d + c];
    }
    out[i] = from_f32<T>(v);
  }
}

struct Bump {  // carve 256-byte aligned pieces out of the caller's scratch
  char* p; size_t left; bool ok = true;
  void* take(size_t n) {
    n = (n + 255) / 256 * 256;
    if (n > left) { ok = false; return nullptr; }
    void* r = p; p += n; left -= n; return r;
  }
};

int linear(int dtype, int M, int N, int K, const void* x, const emoasr_lin_t& l, void* y, int act, const void* residual,
           void* stream) {
  emoasr_epilogue_t e{};
  e.alpha = 1.f; e.res_scale = 1.f;
  e.bias = l.b; e.act = act; e.residual = residual; e.ldr = N;
  return emoasr_gemm_nt(dtype, M, N, K, x, K, l.w, K, y, N, &e, stream);
}

int tree_ok(const emoasr_lm_tree_t* t, const char* who) {
  EMO_CHECK(t && t->llen && t->lanc && t->nnodes && t->row_node && t->row_pos && t->status, "%s: missing tree state", who);
  EMO_CHECK(t->S >= 1 && t->W >= 1 && t->W <= 64 && t->nslots >= 1 && t->Lcap >= 1 && t->node_cap >= 1 &&
            (long)t->S * t->node_cap <= 0x7fffffffL && (long)t->nslots * t->Lcap <= 0x7fffffffL,
            "%s: S=%d W=%d nslots=%d Lcap=%d node_cap=%d unsupported", who, t->S, t->W, t->nslots, t->Lcap, t->node_cap);
  return 0;
}

int tree_attn(int dtype, const emoasr_lm_tree_t* t, int R, int d, int H, const void* qkv, void* kpool, void* vpool,
              const long long* dst, void* out, void* stream) {
  if (R == 0) return 0;
  EMO_CHECK(H >= 1 && d % H == 0 && (d / H) % 8 == 0 && d / H <= 128, "lm_tree_attn: d=%d H=%d unsupported (heads of 8 .. 128 in multiples of 8)", d, H);
  const size_t lds = (size_t)t->Lcap * 8;
  EMO_CHECK(lds + 1536 <= 64 * 1024, "lm_tree_attn: Lcap=%d needs %zu bytes of LDS (64 KB at most)", t->Lcap, lds + 1536);
  TreeAttnArgs a{R, d, d / H, t->nslots, t->Lcap, (long)t->S * t->node_cap, qkv, kpool, vpool, t->llen, t->lanc,
                 t->row_node, dst, 1.f / sqrtf((float)(d / H)), out};
  dim3 grid(a.R, H);
  EMO_DISPATCH(dtype, (lm_tree_attn_kernel<T><<<grid, 64, lds, (hipStream_t)stream>>>(a)));
  EMO_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int emoasr_lm_tree_advance(const emoasr_lm_tree_t* t, const long long* src, const long long* dst,
                                      const long long* active, void* stream) {
  if (tree_ok(t, "lm_tree_advance")) return 1;
  EMO_CHECK(src && dst && active, "lm_tree_advance: missing control words");
  lm_tree_advance_kernel<<<t->S, 64, 0, (hipStream_t)stream>>>(*t, src, dst, active);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_lm_tree_advance_rec(const emoasr_lm_tree_t* t, const int* rec, int rec_cap, const int* rec_count,
                                          const double* lm_weight, long long* lab, long long* dst, void* stream) {
  if (tree_ok(t, "lm_tree_advance_rec")) return 1;
  EMO_CHECK(rec && rec_count && lab && dst && rec_cap >= 1, "lm_tree_advance_rec: missing records or control words (rec_cap=%d)", rec_cap);
  EMO_CHECK(t->nslots % t->S == 0, "lm_tree_advance_rec: %d slots do not divide into %d searches' shares", t->nslots, t->S);
  lm_tree_advance_rec_kernel<<<cdiv(rec_cap, 4), 256, 0, (hipStream_t)stream>>>(*t, rec, rec_cap, rec_count, lm_weight, lab, dst);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_lm_tree_advance_beam(const emoasr_lm_tree_t* t, const int* ids, const int* parent,
                                           const emoasr_beam_state_t* state, int src_base, int dst_base, long long* lab,
                                           long long* dst, void* stream) {
  if (tree_ok(t, "lm_tree_advance_beam")) return 1;
  EMO_CHECK(ids && parent && state && lab && dst, "lm_tree_advance_beam: missing book or control words");
  const long nb = (long)t->S * t->W;
  EMO_CHECK(src_base >= 0 && dst_base >= 0 && src_base + nb <= t->nslots && dst_base + nb <= t->nslots &&
            (src_base + nb <= dst_base || dst_base + nb <= src_base),
            "lm_tree_advance_beam: halves at %d and %d of %ld rows do not lie apart inside %d slots", src_base, dst_base, nb, t->nslots);
  lm_tree_advance_beam_kernel<<<t->S, 64, 0, (hipStream_t)stream>>>(*t, ids, parent, state, src_base, dst_base, lab, dst);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_log_softmax_rows_to(int dtype, int n, int V_lm, int V, const void* x, long ldx, const int* row_dst,
                                          const int* row_ok, float* out, long ld_lm, int out_rows, void* stream) {
  if (n == 0) return 0;
  EMO_CHECK(n > 0 && V >= 1 && V_lm >= V && ldx >= V_lm && ld_lm >= V && out_rows >= 1 && x && row_dst && out,
            "log_softmax_rows_to: n=%d V_lm=%d V=%d ldx=%ld ld_lm=%ld out_rows=%d", n, V_lm, V, ldx, ld_lm, out_rows);
  EMO_DISPATCH(dtype, (log_softmax_rows_to_kernel<T><<<n, 256, 0, (hipStream_t)stream>>>(V_lm, V, (const T*)x, ldx, row_dst, row_ok,
                                                                                        out, ld_lm, out_rows)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_lm_tree_attn_rows(int dtype, const emoasr_lm_tree_t* t, int R, int d, int H, const void* qkv, void* kpool,
                                        void* vpool, const long long* dst, void* out, void* stream) {
  if (tree_ok(t, "lm_tree_attn")) return 1;
  EMO_CHECK(R >= 0 && qkv && kpool && vpool && dst && out, "lm_tree_attn: missing arguments (R=%d)", R);
  return tree_attn(dtype, t, R, d, H, qkv, kpool, vpool, dst, out, stream);
}

extern "C" int emoasr_lm_tree_attn(int dtype, const emoasr_lm_tree_t* t, int d, int H, const void* qkv, void* kpool, void* vpool,
                                   const long long* dst, void* out, void* stream) {
  if (tree_ok(t, "lm_tree_attn")) return 1;
  return emoasr_lm_tree_attn_rows(dtype, t, t->S * t->W, d, H, qkv, kpool, vpool, dst, out, stream);
}

extern "C" size_t emoasr_lm_tree_step_ws_bytes(int dtype, int R, int d, int F) {
  const size_t esz = dtype == EMO_BF16 ? 2 : 4;
  // x, y, o, t1, t2 (d each), qkv (3d), the feed-forward's inner rows (F) + alignment slack
  return (size_t)R * esz * ((size_t)5 * d + 3 * d + F) + 8 * 256;
}

// R rows: the first R of the control words, of (row_node, row_pos) and of the logits; the cost follows R, not the capacity
extern "C" int emoasr_lm_tree_step_rows(int dtype, int nl, const emoasr_bert_layer_t* layers, const emoasr_lm_tree_t* t,
                                        const emoasr_lm_tree_step_t* io, int R, void* stream) {
  if (tree_ok(t, "lm_tree_step")) return 1;
  EMO_CHECK(layers && io && io->ws && io->logits && io->kpool && io->vpool && io->lab && io->dst && io->word_emb && io->pe,
            "lm_tree_step: missing arguments");
  EMO_CHECK(R >= 0, "lm_tree_step: R=%d", R);
  if (R == 0) return 0;
  const int d = io->d, H = io->H, F = io->F, V = io->V;
  EMO_CHECK(nl >= 1 && d >= 1 && H >= 1 && d % H == 0 && F >= 1 && V >= 1 && io->n_emb >= 1, "lm_tree_step: bad dims nl=%d d=%d H=%d F=%d V=%d", nl, d, H, F, V);
  const size_t esz = dtype == EMO_BF16 ? 2 : 4;
  hipStream_t s = (hipStream_t)stream;
  Bump ws{(char*)io->ws, io->ws_bytes};
  void* x = ws.take((size_t)R * d * esz);
  void* y = ws.take((size_t)R * d * esz);
  void* o = ws.take((size_t)R * d * esz);
  void* qkv = ws.take((size_t)R * 3 * d * esz);
  void* act = ws.take((size_t)R * F * esz);
  void* t1 = ws.take((size_t)R * d * esz);
  void* t2 = ws.take((size_t)R * d * esz);
  EMO_CHECK(ws.ok, "lm_tree_step: scratch too small (%zu bytes given)", io->ws_bytes);
  EMO_DISPATCH(dtype, (lm_tree_embed_kernel<T><<<cdiv((long)R * d, 256), 256, 0, s>>>(R, d, io->n_emb, t->Lcap, io->lab, t->row_node,
                                                                                       t->row_pos, (const T*)io->word_emb, io->pe,
                                                                                       (T*)y)));
  EMO_LAUNCH_CHECK();
  const size_t layer_bytes = (size_t)t->S * t->node_cap * d * esz;
  if (emoasr_layernorm_fwd(dtype, R, d, y, io->ln_emb.g, io->ln_emb.b, 1e-12f, x, nullptr, nullptr, stream)) return 1;
  for (int li = 0; li < nl; ++li) {
    const emoasr_bert_layer_t& Ly = layers[li];
    char* kp = (char*)io->kpool + li * layer_bytes;
    char* vp = (char*)io->vpool + li * layer_bytes;
    if (linear(dtype, R, 3 * d, d, x, Ly.qkv, qkv, EMOASR_ACT_NONE, nullptr, stream)) return 1;
    if (tree_attn(dtype, t, R, d, H, qkv, kp, vp, io->dst, o, stream)) return 1;
    if (linear(dtype, R, d, d, o, Ly.attn_out, y, EMOASR_ACT_NONE, x, stream)) return 1;
    if (emoasr_layernorm_fwd(dtype, R, d, y, Ly.ln_attn.g, Ly.ln_attn.b, 1e-12f, x, nullptr, nullptr, stream)) return 1;
    if (linear(dtype, R, F, d, x, Ly.inter, act, 3 /* GELU */, nullptr, stream)) return 1;
    if (linear(dtype, R, d, F, act, Ly.out, y, EMOASR_ACT_NONE, x, stream)) return 1;
    if (emoasr_layernorm_fwd(dtype, R, d, y, Ly.ln_out.g, Ly.ln_out.b, 1e-12f, x, nullptr, nullptr, stream)) return 1;
  }
  if (linear(dtype, R, d, d, x, io->transform, t1, 3, nullptr, stream)) return 1;
  if (emoasr_layernorm_fwd(dtype, R, d, t1, io->ln_transform.g, io->ln_transform.b, 1e-12f, t2, nullptr, nullptr, stream)) return 1;
  emoasr_lin_t tied{io->word_emb, io->out_bias};
  return linear(dtype, R, V, d, t2, tied, io->logits, EMOASR_ACT_NONE, nullptr, stream);
}

extern "C" int emoasr_lm_tree_step(int dtype, int nl, const emoasr_bert_layer_t* layers, const emoasr_lm_tree_t* t,
                                   const emoasr_lm_tree_step_t* io, void* stream) {
  if (tree_ok(t, "lm_tree_step")) return 1;
  return emoasr_lm_tree_step_rows(dtype, nl, layers, t, io, t->S * t->W, stream);
}
