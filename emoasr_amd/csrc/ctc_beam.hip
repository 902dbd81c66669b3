// Batched CTC prefix beam search on the device, no LM: the N-best producer of `test_asr.py --nbest --beam_width N` on a CTC model
// (CTCDecoder._beam_search and _merge_ctc_paths, asr/modeling/decoders/ctc.py:262-344, 372-397).  Results equal the host search of
// csrc/ctc_beam_host.hip: the same hypotheses in the same order, the same sequence of double operations per value.
//
//   emoasr_ctc_beam_batch  one 256-thread workgroup per utterance walks that utterance's frames in order; nothing leaves the
//                          device until the search is over.  A frame is
//     1. candidates   live prefix i gives candidate i (k + 1) + j: j = 0 the stay (blank or a repeat of the last label), j = 1..k
//                     the extension by the frame's j-th best label (a blank among them is no candidate).  That index IS the
//                     first-seen order of the host loop.  One thread per candidate, <= 5 each; the table (p_b, p_nb, asr, length
//                     bonus: 4 doubles x 1 056) lives in LDS.
//     2. merge        live prefixes are distinct label sequences, so two candidates denote the same sequence only when one is the
//                     stay of live q and the other the extension (p, v) with q = p + (v): at most two ever fold.  Every prefix has
//                     a canonical node id (below), so that test is q.parent == p.id && q.last == v, found by the extension's
//                     thread in a loop over the <= 32 live prefixes.  The fold is lse2 per value, first operand the candidate
//                     seen first, which also keeps its length bonus and its position; the other one is struck.
//     3. select       W rounds of a workgroup arg-max over (total descending, position ascending): what std::stable_sort leaves
//                     in front.  Totals stay in registers; a round is a wave butterfly, one LDS word pair per wave and one
//                     barrier (the pairs are double-buffered).  Rank counting would read 1 056 x 1 056 totals per frame.
//     4. identity     a survivor that is an extension without a live twin gets its id from a per-utterance trie: an open-addressed
//                     table in the workspace keyed by (parent id, label), the id being the slot it lands in (+ 1; the root (<eos>)
//                     is 0).  A prefix that dropped out and is formed again finds its old slot, so a child that outlived it still
//                     matches.  <= W compare-and-swap probes per frame, <= frames x W + 1 nodes, load <= 1/2.
//                          The token sequences are rebuilt once, at the end, by walking the keys back to the root.
//
// Nothing is contracted: the library is built with -ffp-contract=off, the length bonus is one multiply, the total two adds.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int BEAM_MAX_W = EMOASR_CTC_BEAM_MAX_WIDTH;
#ifndef EMO_CTC_BEAM_THREADS   // A/B builds only (python -m emoasr_amd.build --variant beam64 -DEMO_CTC_BEAM_THREADS=64): 64, 128 or 256
#define EMO_CTC_BEAM_THREADS 256
#endif
constexpr int BEAM_THREADS = EMO_CTC_BEAM_THREADS;
static_assert(BEAM_THREADS == 64 || BEAM_THREADS == 128 || BEAM_THREADS == 256, "whole waves, a power of two");
constexpr int BEAM_MAX_CAND = BEAM_MAX_W * (BEAM_MAX_W + 1);                         // 1 056
constexpr int BEAM_PER_THREAD = (BEAM_MAX_CAND + BEAM_THREADS - 1) / BEAM_THREADS;   // 5
constexpr long BEAM_WS_BYTES_PER_NODE = 32;   // 4 slots of 8 bytes per possible node: a power of two of slots with load <= 1/2 fits
constexpr long BEAM_MAX_NODES = 1l << 28;      // node ids and slot counts stay well inside 32 bits
constexpr double NEG = -1e10;                 // LOG_0 of decoders/ctc.py:23

enum { BEAM_BAD_LABEL = 1, BEAM_BAD_OFFSETS = 2, BEAM_TOO_LONG = 4, BEAM_WS_SHORT = 8 };
enum { CAND_NEW = -1, CAND_NONE = -2 };       // c_id: an extension whose node id is not known yet / no candidate (blank, folded away)

__device__ __forceinline__ double lse2(double a, double b) {
  const double m = a > b ? a : b;
  return m + log(exp(a - m) + exp(b - m));
}

struct Live {
  double p_b, p_nb, len_bonus, total;
  int id, parent, last, n_plain, len, pad;    // last = -1: the root, which has no label to repeat
};

typedef unsigned long long u64;

__device__ __forceinline__ u64 trie_key(int parent, int v) { return ((u64)(unsigned)parent << 32) | (unsigned)(v + 1); }

// slot + 1 of (parent, v), inserted when absent; -1 when the table is full (it never is: load <= 1/2).  Keys tried in one frame
// are distinct, so the compare-and-swap alone orders them; keys of earlier frames are behind a barrier.
__device__ int trie_find_or_add(u64* tab, unsigned mask, int parent, int v) {
  const u64 key = trie_key(parent, v);
  unsigned h = (unsigned)parent * 0x9E3779B1u ^ (unsigned)(v + 1) * 0x85EBCA77u;
  h ^= h >> 15;
  for (unsigned n = 0; n <= mask; ++n) {
    const unsigned s = (h + n) & mask;
    const u64 old = atomicCAS(tab + s, (u64)0, key);
    if (old == 0 || old == key) return (int)s + 1;
  }
  return -1;
}

__device__ __forceinline__ bool beats(double t, int p, double bt, int bp) {   // (total descending, position ascending)
  return p != INT_MAX && (bp == INT_MAX || t > bt || (t == bt && p < bp));
}

__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_batch_kernel(
    int V, int W, int k, const float* __restrict__ logp, long ld, const int* __restrict__ row_off, const int* __restrict__ top,
    int blank, int eos, double len_weight, int max_frames, int* __restrict__ out_tok, int* __restrict__ out_len,
    double* __restrict__ out_score, int* __restrict__ out_n, unsigned char* __restrict__ ws, long ws_bytes,
    int* __restrict__ status) {
  __shared__ double c_pb[BEAM_MAX_CAND], c_pnb[BEAM_MAX_CAND], c_asr[BEAM_MAX_CAND], c_bonus[BEAM_MAX_CAND];
  __shared__ int c_id[BEAM_MAX_CAND];
  __shared__ Live live[2][BEAM_MAX_W];
  __shared__ double wred_t[2][BEAM_THREADS / 64];
  __shared__ int wred_p[2][BEAM_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long r0 = row_off[b], r1 = row_off[b + 1];
  const long frames = r1 - r0;
  // this utterance's share of the workspace: 4 slots per node it can make, from 32 (W row_off[b] + b) bytes on
  const long cap = (long)W * frames + 1;
  const long ws_lo = BEAM_WS_BYTES_PER_NODE * ((long)W * r0 + b), ws_hi = BEAM_WS_BYTES_PER_NODE * ((long)W * r1 + b + 1);
  int err = 0;
  if (r0 < 0 || frames < 0) err = BEAM_BAD_OFFSETS;
  else if (frames > max_frames || cap > BEAM_MAX_NODES) err = BEAM_TOO_LONG;
  else if (ws_hi > ws_bytes) err = BEAM_WS_SHORT;
  if (err) {                                   // (uniform over the workgroup)
    if (tid == 0) { atomicOr(status, err); out_n[b] = -1; }
    return;
  }
  u64* tab = (u64*)(ws + ws_lo);
  unsigned slots = 2;
  while ((long)slots < 2 * cap) slots <<= 1;   // <= 4 cap - 2
  const unsigned mask = slots - 1;
  for (unsigned s = tid; s < slots; s += BEAM_THREADS) __hip_atomic_store(tab + s, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) live[0][0] = Live{0.0, NEG, 0.0, 0.0, 0, -1, -1, 0, 1, 0};   // (<eos>): hypotheses start with the LM's BOS
  __threadfence();
  __syncthreads();

  const int kk = k + 1;
  int n_live = 1, cur = 0;
  for (long t = 0; t < frames; ++t) {
    const float* row = logp + (r0 + t) * ld;
    const int* tp = top + (r0 + t) * (long)k;
    const Live* L = live[cur];
    Live* N = live[cur ^ 1];
    const int nc = n_live * kk;
    const double lp_blank = (double)row[blank];
    int match[BEAM_PER_THREAD];
    int bad = 0;
    // 1. candidates
#pragma unroll
    for (int m = 0; m < BEAM_PER_THREAD; ++m) {
      const int c = tid + m * BEAM_THREADS;
      match[m] = -1;
      if (c >= nc) continue;
      const int i = c / kk, j = c - i * kk;
      const Live p = L[i];
      const bool has_last = p.last >= 0;
      if (j == 0) {   // stay on the same prefix: blank, or a repeat of its last label
        const double stay_b = lse2(p.p_b + lp_blank, p.p_nb + lp_blank);
        const double stay_nb = has_last ? p.p_nb + (double)row[p.last] : NEG;
        c_pb[c] = stay_b; c_pnb[c] = stay_nb; c_asr[c] = lse2(stay_b, stay_nb); c_bonus[c] = p.len_bonus; c_id[c] = p.id;
        continue;
      }
      const int v = tp[j - 1];
      if (v < 0 || v >= V) { bad = 1; c_id[c] = CAND_NONE; continue; }
      if (v == blank) { c_id[c] = CAND_NONE; continue; }
      const double lp_v = (double)row[v];
      const double ext_nb = (has_last && v == p.last) ? p.p_b + lp_v : lse2(p.p_b + lp_v, p.p_nb + lp_v);
      c_pb[c] = NEG; c_pnb[c] = ext_nb; c_asr[c] = lse2(NEG, ext_nb);
      c_bonus[c] = __dmul_rn(len_weight, (double)(p.n_plain + 1));   // the length bonus counts the PARENT's labels (ctc.py:308)
      c_id[c] = CAND_NEW;
      for (int q = 0; q < n_live; ++q)
        if (L[q].parent == p.id && L[q].last == v) match[m] = q;
    }
    if (__syncthreads_or(bad)) {
      if (tid == 0) { atomicOr(status, BEAM_BAD_LABEL); out_n[b] = -1; }
      return;
    }
    // 2. merge: the extension's thread folds the pair into whichever of the two was seen first
#pragma unroll
    for (int m = 0; m < BEAM_PER_THREAD; ++m) {
      const int c = tid + m * BEAM_THREADS, q = match[m];
      if (q < 0) continue;
      const int s = q * kk;
      if (s < c) {
        c_pb[s] = lse2(c_pb[s], c_pb[c]); c_pnb[s] = lse2(c_pnb[s], c_pnb[c]); c_asr[s] = lse2(c_asr[s], c_asr[c]);
        c_id[c] = CAND_NONE;
      } else {
        c_pb[c] = lse2(c_pb[c], c_pb[s]); c_pnb[c] = lse2(c_pnb[c], c_pnb[s]); c_asr[c] = lse2(c_asr[c], c_asr[s]);
        c_id[c] = L[q].id;
        c_id[s] = CAND_NONE;
      }
    }
    __syncthreads();
    // 3. select the W largest totals, ties to the lower position
    double tot[BEAM_PER_THREAD];
    unsigned alive = 0;
#pragma unroll
    for (int m = 0; m < BEAM_PER_THREAD; ++m) {
      const int c = tid + m * BEAM_THREADS;
      tot[m] = 0.0;
      if (c < nc && c_id[c] != CAND_NONE) {
        tot[m] = __dadd_rn(__dadd_rn(c_asr[c], 0.0), c_bonus[c]);   // asr + lm + len_bonus with lm = 0.0
        alive |= 1u << m;
      }
    }
    int n_new = 0;
    for (int r = 0; r < W; ++r) {
      double bt = 0.0;
      int bp = INT_MAX;
#pragma unroll
      for (int m = 0; m < BEAM_PER_THREAD; ++m)
        if (((alive >> m) & 1u) && (bp == INT_MAX || tot[m] > bt)) { bt = tot[m]; bp = tid + m * BEAM_THREADS; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ot = __shfl_xor(bt, o, 64);
        const int op = __shfl_xor(bp, o, 64);
        if (beats(ot, op, bt, bp)) { bt = ot; bp = op; }
      }
      if (lane == 0) { wred_t[r & 1][wave] = bt; wred_p[r & 1][wave] = bp; }
      __syncthreads();
      bt = wred_t[r & 1][0]; bp = wred_p[r & 1][0];
#pragma unroll
      for (int w = 1; w < BEAM_THREADS / 64; ++w)
        if (beats(wred_t[r & 1][w], wred_p[r & 1][w], bt, bp)) { bt = wred_t[r & 1][w]; bp = wred_p[r & 1][w]; }
      if (bp == INT_MAX) break;                // (uniform: every thread read the same four pairs)
      if ((bp & (BEAM_THREADS - 1)) == tid) {
        alive &= ~(1u << (bp / BEAM_THREADS));
        const int i = bp / kk, j = bp - i * kk;
        Live nw = L[i];
        nw.p_b = c_pb[bp]; nw.p_nb = c_pnb[bp]; nw.len_bonus = c_bonus[bp]; nw.total = bt;
        if (j > 0) {
          const int v = tp[j - 1];
          nw.parent = L[i].id; nw.last = v; nw.len = L[i].len + 1;
          nw.n_plain = L[i].n_plain + (v == eos ? 0 : 1);   // an appended <eos> is not a plain label
          nw.id = c_id[bp];
        }
        N[r] = nw;
      }
      ++n_new;
    }
    __syncthreads();
    // 4. node ids of the survivors that are new (or formed again): <= W probes, all in the first wave
    int full = 0;
    if (tid < n_new && N[tid].id == CAND_NEW) {
      const int id = trie_find_or_add(tab, mask, N[tid].parent, N[tid].last);
      N[tid].id = id;
      full = id < 0;
    }
    if (__syncthreads_or(full)) {
      if (tid == 0) { atomicOr(status, BEAM_WS_SHORT); out_n[b] = -1; }
      return;
    }
    n_live = n_new;
    cur ^= 1;
  }

  // the live prefixes are in selection order, best first; their labels come from walking the keys back to the root
  if (tid == 0) out_n[b] = n_live;
  if (tid < n_live) {
    const Live p = live[cur][tid];
    const long o = (long)b * W + tid;
    out_len[o] = p.len;
    out_score[o] = p.total;
    int* tok = out_tok + o * ((long)max_frames + 1);
    int id = p.id;
    for (int pos = p.len - 1; pos >= 1 && id >= 1 && (unsigned)(id - 1) <= mask; --pos) {
      const u64 key = __hip_atomic_load(tab + (id - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tok[pos] = (int)(unsigned)(key & 0xFFFFFFFFu) - 1;
      id = (int)(key >> 32);
    }
    tok[0] = eos;
  }
}

}  // namespace

extern "C" long emoasr_ctc_beam_batch_ws_bytes(int B, int total_rows, int W) {
  if (B < 0 || total_rows < 0 || W < 1 || W > BEAM_MAX_W) return -1;
  return BEAM_WS_BYTES_PER_NODE * ((long)W * total_rows + B);
}

extern "C" int emoasr_ctc_beam_batch(int B, int V, int W, int k, const float* logp, long ld, const int* row_off, const int* top,
                                     int blank, int eos, double len_weight, int max_frames, int* out_tok, int* out_len,
                                     double* out_score, int* out_n, void* ws, long ws_bytes, int* status, void* stream) {
  if (B == 0) return 0;
  EMO_CHECK(W >= 1 && W <= BEAM_MAX_W, "ctc_beam_batch: beam width %d is outside 1..%d", W, BEAM_MAX_W);
  EMO_CHECK(B > 0 && V >= 1 && k >= 1 && k <= W && k <= V && ld >= V, "ctc_beam_batch: B=%d V=%d W=%d k=%d ld=%ld", B, V, W, k, ld);
  EMO_CHECK(blank >= 0 && blank < V && eos >= 0 && eos < V, "ctc_beam_batch: blank %d / eos %d outside the %d labels", blank, eos,
            V);
  EMO_CHECK(max_frames >= 0 && ws_bytes >= 0, "ctc_beam_batch: max_frames=%d ws_bytes=%ld", max_frames, ws_bytes);
  EMO_CHECK(row_off && out_tok && out_len && out_score && out_n && ws && status && (max_frames == 0 || (logp && top)),
            "ctc_beam_batch: null argument");
  ctc_beam_batch_kernel<<<B, BEAM_THREADS, 0, (hipStream_t)stream>>>(V, W, k, logp, ld, row_off, top, blank, eos, len_weight,
                                                                     max_frames, out_tok, out_len, out_score, out_n,
                                                                     (unsigned char*)ws, ws_bytes, status);
  EMO_LAUNCH_CHECK();
  return 0;
}
