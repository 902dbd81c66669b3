// Device code shared by the two CTC prefix beam searches: the whole-utterance search without an LM (csrc/ctc_beam.hip) and the
// frame-per-launch search with LM shallow fusion (csrc/ctc_beam_lm.hip).  Everything that decides a hypothesis or a score bit is
// here, once: a fused search with lm_weight = 0 equals the plain one because both run this code, not because two copies agree.
//
// One 256-thread workgroup advances one search by one frame (beam_frame_step):
//     0. LM scan      (LM only) thread i < live walks prefix i's k candidates in top order: lm_run = p.lm, then per label that is
//                     not the blank lm_run = lm_run + lm_weight * (double)lm_logp[slot_i][label] (one multiply, one add, in that
//                     order: the reference's running `score_lm +=`, ctc.py:309-310).  Extension j carries the running value, the
//                     stay p.lm.  k adds per live prefix, none per candidate.  lm_weight <= 0: nothing is read or added.
//     1. candidates   live prefix i gives candidate i (k + 1) + j: j = 0 the stay (blank or a repeat of the last label), j = 1..k
//                     the extension by the frame's j-th best label (a blank among them is no candidate).  That index IS the
//                     first-seen order of the host loop.  One thread per candidate, <= 5 each; the table (p_b, p_nb, asr, length
//                     bonus, with an LM its term: 4 or 5 doubles x 1 056) lives in LDS.
//     2. merge        live prefixes are distinct label sequences, so two candidates denote the same sequence only when one is the
//                     stay of live q and the other the extension (p, v) with q = p + (v): at most two ever fold.  Every prefix has
//                     a canonical node id (below), so that test is q.parent == p.id && q.last == v, found by the extension's
//                     thread in a loop over the <= 32 live prefixes.  The fold is lse2 per value, first operand the candidate
//                     seen first, which also keeps its LM term, its length bonus and its position; the other one is struck.
//     3. select       W rounds of a workgroup arg-max over (total descending, position ascending): what std::stable_sort leaves
//                     in front.  Totals stay in registers; a round is a wave butterfly, one LDS word pair per wave and one
//                     barrier (the pairs are double-buffered).  Rank counting would read 1 056 x 1 056 totals per frame.
// and then gives the survivors their identity (beam_new_ids):
//     4. identity     a survivor that is an extension without a live twin gets its id from a per-search trie: an open-addressed
//                     table in the workspace keyed by (parent id, label), the id being the slot it lands in (+ 1; the root (<eos>)
//                     is 0).  A prefix that dropped out and is formed again finds its old slot, so a child that outlived it still
//                     matches.  <= W compare-and-swap probes per frame, <= frames x W + 1 nodes, load <= 1/2.
//                          The token sequences are rebuilt once, at the end, by walking the keys back to the root (beam_back_walk).
//
// Nothing is contracted: the library is built with -ffp-contract=off, the length bonus is one multiply, the total two adds.
#pragma once
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int BEAM_MAX_W = EMOASR_CTC_BEAM_MAX_WIDTH;
constexpr int BEAM_THREADS = 256;             // (64 and 128 were measured and lost at both beam widths: DESIGN.md section 18)
constexpr int BEAM_MAX_CAND = BEAM_MAX_W * (BEAM_MAX_W + 1);                         // 1 056
constexpr int BEAM_PER_THREAD = (BEAM_MAX_CAND + BEAM_THREADS - 1) / BEAM_THREADS;   // 5
constexpr long BEAM_WS_BYTES_PER_NODE = 32;   // 4 slots of 8 bytes per possible node: a power of two of slots with load <= 1/2 fits
constexpr long BEAM_MAX_NODES = 1l << 28;     // node ids and slot counts stay well inside 32 bits
constexpr double NEG = -1e10;                 // LOG_0 of decoders/ctc.py:23

enum { BEAM_BAD_LABEL = 1, BEAM_BAD_OFFSETS = 2, BEAM_TOO_LONG = 4, BEAM_WS_SHORT = 8, BEAM_BAD_UTT = 16, BEAM_NO_SLOT = 32 };
enum { CAND_NEW = -1, CAND_NONE = -2 };       // id: an extension whose node id is not known yet / no candidate (blank, folded away)

__device__ __forceinline__ double lse2(double a, double b) {
  const double m = a > b ? a : b;
  return m + log(exp(a - m) + exp(b - m));
}

struct Live {
  double p_b, p_nb, lm, len_bonus, total;     // lm, slot: 0.0 and unused without an LM
  int id, parent, last, n_plain, len, slot;   // last = -1: the root, which has no label to repeat; slot: its row of the LM pool
};
static_assert(sizeof(Live) == 64, "the live set is copied as 16 words per prefix");

// (<eos>): hypotheses start with the LM's BOS
__device__ __forceinline__ Live live_root(int slot) { return Live{0.0, NEG, 0.0, 0.0, 0.0, 0, -1, -1, 0, 1, slot}; }

typedef unsigned long long u64;

// slots of the trie of a search that can make `cap` nodes: a power of two, <= 4 cap - 2
__device__ __forceinline__ unsigned trie_slots(long cap) {
  unsigned slots = 2;
  while ((long)slots < 2 * cap) slots <<= 1;
  return slots;
}

__device__ __forceinline__ void trie_clear(u64* tab, unsigned slots) {
  for (unsigned s = threadIdx.x; s < slots; s += BEAM_THREADS) __hip_atomic_store(tab + s, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

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

// Steps 0-3 of one frame for the whole workgroup: the live set L[0 .. n_live) and the frame's log-probabilities `row` and top-k
// labels `tp` -> the survivors N[0 .. n_new), best first, complete (behind a barrier) on return.  -> n_new, or -1 when a top-k
// label is outside the V labels (uniform over the workgroup; the caller writes its own refusal).  A survivor that needs a node id
// has id == CAND_NEW, and with an LM slot == -1 unless it folded with its live twin, whose row it keeps.
// lm_logp, ld_lm: the LM pool (read when LM and lm_weight > 0 only).  L and N are the caller's, in LDS; the candidate table and
// the per-wave arg-max pairs are this function's own LDS, one array each and not one struct: the compiler then knows that a
// store to one column cannot change another.
template <bool LM>
__device__ __forceinline__ int beam_frame_step(const Live* L, Live* N, int n_live, const float* __restrict__ row,
                                               const int* __restrict__ tp, int V, int W, int k, int blank, int eos, double lm_weight,
                                               double len_weight, const float* __restrict__ lm_logp, long ld_lm) {
  __shared__ double c_pb[BEAM_MAX_CAND], c_pnb[BEAM_MAX_CAND], c_asr[BEAM_MAX_CAND], c_bonus[BEAM_MAX_CAND];
  __shared__ double c_lm[LM ? BEAM_MAX_CAND : 1];   // (never touched, and so never allocated, without an LM)
  __shared__ int c_id[BEAM_MAX_CAND];
  __shared__ double wred_t[2][BEAM_THREADS / 64];
  __shared__ int wred_p[2][BEAM_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = k + 1;
  const int nc = n_live * kk;
  const double lp_blank = (double)row[blank];
  int match[BEAM_PER_THREAD];
  int bad = 0;
  // 0. the running LM sum along each live prefix's candidates, in top order
  if constexpr (LM) {
    if (tid < n_live) {
      const Live p = L[tid];
      double lm_run = p.lm;
      c_lm[tid * kk] = p.lm;
      const bool use_lm = lm_weight > 0.0;
      const float* lrow = lm_logp + (long)p.slot * ld_lm;
      for (int j = 1; j <= k; ++j) {
        const int v = tp[j - 1];
        if (use_lm && v >= 0 && v < V && v != blank) lm_run = __dadd_rn(lm_run, __dmul_rn(lm_weight, (double)lrow[v]));
        c_lm[tid * kk + j] = lm_run;
      }
    }
  }
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
  if (__syncthreads_or(bad)) return -1;
  // 2. merge: the extension's thread folds the pair into whichever of the two was seen first (which keeps its LM term and bonus)
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
      double lm = 0.0;
      if constexpr (LM) lm = c_lm[c];
      tot[m] = __dadd_rn(__dadd_rn(c_asr[c], lm), c_bonus[c]);   // (asr + lm) + len_bonus
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
      if constexpr (LM) nw.lm = c_lm[bp];
      if (j > 0) {
        const int v = tp[j - 1];
        nw.parent = L[i].id; nw.last = v; nw.len = L[i].len + 1;
        nw.n_plain = L[i].n_plain + (v == eos ? 0 : 1);   // an appended <eos> is not a plain label
        nw.id = c_id[bp];
        if constexpr (LM) {
          nw.slot = -1;
          if (nw.id != CAND_NEW)                          // folded with its live twin: that prefix keeps its row
            for (int q = 0; q < n_live; ++q)
              if (L[q].id == nw.id) nw.slot = L[q].slot;
        }
      }
      N[r] = nw;
    }
    ++n_new;
  }
  __syncthreads();
  return n_new;
}

// 4. node ids of the survivors that are new (or formed again): <= W probes, all in the first wave.  -> whether this thread's
// survivor was one; *full: its probe found the table full (the caller votes and refuses).
__device__ __forceinline__ bool beam_new_ids(Live* N, int n_new, u64* tab, unsigned mask, int* full) {
  const int tid = threadIdx.x;
  const bool is_new = tid < n_new && N[tid].id == CAND_NEW;
  *full = 0;
  if (is_new) {
    const int id = trie_find_or_add(tab, mask, N[tid].parent, N[tid].last);
    N[tid].id = id;
    *full = id < 0;
  }
  return is_new;
}

// tok[0 .. len) of the prefix with node id `id`: <eos>, then its labels from walking the trie keys back to the root
__device__ __forceinline__ void beam_back_walk(const u64* tab, unsigned mask, int id, int len, int eos, int* __restrict__ tok) {
  for (int pos = len - 1; pos >= 1 && id >= 1 && (unsigned)(id - 1) <= mask; --pos) {
    const u64 key = __hip_atomic_load(tab + (id - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tok[pos] = (int)(unsigned)(key & 0xFFFFFFFFu) - 1;
    id = (int)(key >> 32);
  }
  tok[0] = eos;
}

}  // namespace
