// Batched CTC prefix beam search WITH LM shallow fusion on the device, one frame per launch (CTCDecoder._beam_search with lm /
// lm_weight, asr/modeling/decoders/ctc.py:203-344).  A *search* is one (utterance, (lm_weight, len_weight)) pair: S searches run
// over B utterances, several of them may name the same utterance (the cells of a fusion grid) and then share its logp / top rows,
// which are only read.  Results equal the host search of csrc/ctc_beam_host.hip fed the same f32 LM rows: the same hypotheses in
// the same order, the same sequence of double operations per value.
//
//   emoasr_ctc_beam_lm_init    every search becomes the root (<eos>) holding slot 0 of its share of the LM pool; its trie is cleared;
//                              one record per search asks for the root's LM row (src = -1: from the zero state).
//   emoasr_ctc_beam_lm_frame   one 256-thread workgroup per search advances it by frame t (a search whose utterance is shorter
//                              returns at once).  Steps 1-4 are those of csrc/ctc_beam.hip (candidates at position i (k + 1) + j,
//                              the fold of a stay with its extension twin into the one seen first, W rounds of arg-max with ties to
//                              the lower position, node ids from the (parent id, label) trie) plus
//     0. LM scan      thread i < live walks prefix i's k candidates in top order: lm_run = p.lm, then per label that is not the
//                     blank lm_run = lm_run + lm_weight * (double)lm_logp[slot_i][label] (one multiply, one add, in that order:
//                     the reference's running `score_lm +=`, ctc.py:309-310).  Extension j carries the running value, the stay
//                     p.lm; a fold keeps the LM term of the candidate seen first.  k adds per live prefix, none per candidate.
//                     lm_weight <= 0: nothing is read or added, the term stays 0.0 and the search is that of ctc_beam.hip.
//     5. slots        a survivor that is an extension without a live twin is a NEW prefix: it takes a row of the LM pool from the
//                     search's free list and emits a record (search, node, parent node, label, parent's row, its row); the caller
//                     runs the LM over the records before the next launch.  The row of a prefix that left the beam is freed at the
//                     start of the NEXT frame: this frame's records may still name it as a parent.  Held at once: <= W live after
//                     the previous frame + <= W taken now = 2 W rows.  An empty free list retires the search (status bit 5).
//   emoasr_ctc_beam_lm_finish  token sequences by walking the trie keys back to the root, as ctc_beam.hip ends.
//
// State between launches lives in the workspace: per search a block (live set, free list, dying list) and a trie share sized for
// max_frames.  Stores are plain stores plus the trie's compare-and-swap and the atomic adds of the record count / status word.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int BEAM_MAX_W = EMOASR_CTC_BEAM_MAX_WIDTH;
constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_CAND = BEAM_MAX_W * (BEAM_MAX_W + 1);                         // 1 056
constexpr int BEAM_PER_THREAD = (BEAM_MAX_CAND + BEAM_THREADS - 1) / BEAM_THREADS;   // 5
constexpr long BEAM_WS_BYTES_PER_NODE = 32;   // 4 trie slots of 8 bytes per possible node
constexpr long BEAM_MAX_NODES = 1l << 28;
constexpr int BEAM_MAX_SLOTS = 2 * BEAM_MAX_W + 2;   // rows of the LM pool one search ever uses
constexpr int BEAM_FREE_CAP = 72;                    // >= BEAM_MAX_SLOTS, keeps the head a multiple of 8 bytes
constexpr double NEG = -1e10;                 // LOG_0 of decoders/ctc.py:23

enum { BEAM_BAD_LABEL = 1, BEAM_BAD_OFFSETS = 2, BEAM_TOO_LONG = 4, BEAM_WS_SHORT = 8, BEAM_BAD_UTT = 16, BEAM_NO_SLOT = 32 };
enum { CAND_NEW = -1, CAND_NONE = -2 };

__device__ __forceinline__ double lse2(double a, double b) {
  const double m = a > b ? a : b;
  return m + log(exp(a - m) + exp(b - m));
}

struct Live {
  double p_b, p_nb, lm, len_bonus, total;
  int id, parent, last, n_plain, len, slot;   // last = -1: the root; slot: this prefix's row of the LM pool
};
static_assert(sizeof(Live) == 64, "the live set is copied as 16 words per prefix");

struct Head {
  int n_live, n_free, n_dying, dead;
  unsigned mask;                              // trie slots - 1
  int pad[3];
  int free_[BEAM_FREE_CAP];                   // rows not held, taken from the end
  int dying[BEAM_MAX_W];                      // rows of the prefixes that left the beam at the previous frame
};
constexpr long STATE_BYTES = BEAM_MAX_W * (long)sizeof(Live) + (long)sizeof(Head);
static_assert(sizeof(Head) % 8 == 0 && STATE_BYTES % 8 == 0, "trie shares stay 8-byte aligned");
constexpr int HEAD_WORDS = sizeof(Head) / 4;

typedef unsigned long long u64;

__device__ __forceinline__ long trie_share(int W, int max_frames) { return BEAM_WS_BYTES_PER_NODE * ((long)W * max_frames + 1); }

__device__ __forceinline__ u64 trie_key(int parent, int v) { return ((u64)(unsigned)parent << 32) | (unsigned)(v + 1); }

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

// what a search's utterance and its share of the workspace allow -> 0 or the status bit (uniform over the workgroup)
__device__ __forceinline__ int check_search(int s, int S, int B, int W, int max_frames, const int* row_off, const int* utt,
                                            long ws_bytes, long* r0_out, long* frames_out) {
  const int u = utt[s];
  if (u < 0 || u >= B) return BEAM_BAD_UTT;
  const long r0 = row_off[u], frames = (long)row_off[u + 1] - r0;
  if (r0 < 0 || frames < 0) return BEAM_BAD_OFFSETS;
  if (frames > max_frames || (long)W * frames + 1 > BEAM_MAX_NODES) return BEAM_TOO_LONG;
  if ((long)S * STATE_BYTES + (long)(s + 1) * trie_share(W, max_frames) > ws_bytes) return BEAM_WS_SHORT;
  *r0_out = r0;
  *frames_out = frames;
  return 0;
}

__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_lm_init_kernel(
    int S, int B, int W, const int* __restrict__ row_off, const int* __restrict__ utt, int eos, int max_frames, int slots,
    unsigned char* __restrict__ ws, long ws_bytes, int* __restrict__ rec, int rec_cap, int* __restrict__ rec_count,
    int* __restrict__ status) {
  const int s = blockIdx.x, tid = threadIdx.x;
  Live* gl = (Live*)(ws + (long)s * STATE_BYTES);
  Head* gh = (Head*)(gl + BEAM_MAX_W);
  long r0 = 0, frames = 0;
  const int err = check_search(s, S, B, W, max_frames, row_off, utt, ws_bytes, &r0, &frames);
  if (err) {
    if (tid == 0) { atomicOr(status, err); gh->dead = 1; gh->n_live = 0; gh->n_free = 0; gh->n_dying = 0; gh->mask = 0; }
    return;
  }
  u64* tab = (u64*)(ws + (long)S * STATE_BYTES + (long)s * trie_share(W, max_frames));
  const long cap = (long)W * frames + 1;
  unsigned tslots = 2;
  while ((long)tslots < 2 * cap) tslots <<= 1;   // <= 4 cap - 2
  for (unsigned i = tid; i < tslots; i += BEAM_THREADS) __hip_atomic_store(tab + i, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int nslot = slots < BEAM_MAX_SLOTS ? slots : BEAM_MAX_SLOTS;
  const int base = s * slots;
  for (int i = tid; i < nslot - 1; i += BEAM_THREADS) gh->free_[i] = base + nslot - 1 - i;   // (taken from the end: 1, 2, ...)
  if (tid == 0) {
    gl[0] = Live{0.0, NEG, 0.0, 0.0, 0.0, 0, -1, -1, 0, 1, base};   // (<eos>): hypotheses start with the LM's BOS
    gh->n_live = 1; gh->n_free = nslot - 1; gh->n_dying = 0; gh->dead = 0; gh->mask = tslots - 1;
    const int r = atomicAdd(rec_count, 1);
    if (r < rec_cap) {
      rec[r] = s; rec[rec_cap + r] = 0; rec[2 * (long)rec_cap + r] = -1; rec[3 * (long)rec_cap + r] = eos;
      rec[4 * (long)rec_cap + r] = -1; rec[5 * (long)rec_cap + r] = base;
    }
  }
}

__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_lm_frame_kernel(
    int S, int B, int V, int W, int k, int t, const float* __restrict__ logp, long ld, const int* __restrict__ row_off,
    const int* __restrict__ top, const int* __restrict__ utt, const double* __restrict__ lm_weight,
    const double* __restrict__ len_weight, int blank, int eos, int max_frames, const float* __restrict__ lm_logp, long ld_lm,
    unsigned char* __restrict__ ws, long ws_bytes, int* __restrict__ rec, int rec_cap, int* __restrict__ rec_count,
    int* __restrict__ status) {
  __shared__ double c_pb[BEAM_MAX_CAND], c_pnb[BEAM_MAX_CAND], c_asr[BEAM_MAX_CAND], c_bonus[BEAM_MAX_CAND], c_lm[BEAM_MAX_CAND];
  __shared__ int c_id[BEAM_MAX_CAND];
  __shared__ Live live[2][BEAM_MAX_W];
  __shared__ Head h;
  __shared__ double wred_t[2][BEAM_THREADS / 64];
  __shared__ int wred_p[2][BEAM_THREADS / 64];
  __shared__ int verdict;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Live* gl = (Live*)(ws + (long)s * STATE_BYTES);
  Head* gh = (Head*)(gl + BEAM_MAX_W);
  if (gh->dead) return;
  long r0 = 0, frames = 0;
  int err = check_search(s, S, B, W, max_frames, row_off, utt, ws_bytes, &r0, &frames);
  if (err) {
    if (tid == 0) { atomicOr(status, err); gh->dead = 1; }
    return;
  }
  if (t >= frames) return;
  u64* tab = (u64*)(ws + (long)S * STATE_BYTES + (long)s * trie_share(W, max_frames));
  // the state block -> LDS
  for (int i = tid; i < HEAD_WORDS; i += BEAM_THREADS) ((int*)&h)[i] = ((const int*)gh)[i];
  for (int i = tid; i < BEAM_MAX_W * 16; i += BEAM_THREADS) ((int*)live[0])[i] = ((const int*)gl)[i];
  if (tid == 0) verdict = 0;
  __syncthreads();
  const int n_live = h.n_live < W ? h.n_live : W;
  const unsigned mask = h.mask;
  if (n_live < 1 || h.n_free < 0 || h.n_dying < 0 || h.n_dying > BEAM_MAX_W || h.n_free + h.n_dying > BEAM_MAX_SLOTS ||
      (long)(mask + 1) * 8 > trie_share(W, max_frames)) {   // (a block that init never wrote)
    if (tid == 0) { atomicOr(status, BEAM_WS_SHORT); gh->dead = 1; }
    return;
  }
  const double lmw = lm_weight[s], lenw = len_weight[s];
  const float* row = logp + (r0 + t) * ld;
  const int* tp = top + (r0 + t) * (long)k;
  const Live* L = live[0];
  Live* N = live[1];
  const int kk = k + 1;
  const int nc = n_live * kk;
  const double lp_blank = (double)row[blank];
  int match[BEAM_PER_THREAD];
  int bad = 0;
  // 0. the running LM sum along each live prefix's candidates, in top order
  if (tid < n_live) {
    const Live p = L[tid];
    double lm_run = p.lm;
    c_lm[tid * kk] = p.lm;
    const bool use_lm = lmw > 0.0;
    const float* lrow = lm_logp + (long)p.slot * ld_lm;
    for (int j = 1; j <= k; ++j) {
      const int v = tp[j - 1];
      if (use_lm && v >= 0 && v < V && v != blank) lm_run = __dadd_rn(lm_run, __dmul_rn(lmw, (double)lrow[v]));
      c_lm[tid * kk + j] = lm_run;
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
    c_bonus[c] = __dmul_rn(lenw, (double)(p.n_plain + 1));   // the length bonus counts the PARENT's labels (ctc.py:308)
    c_id[c] = CAND_NEW;
    for (int q = 0; q < n_live; ++q)
      if (L[q].parent == p.id && L[q].last == v) match[m] = q;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) { atomicOr(status, BEAM_BAD_LABEL); gh->dead = 1; }
    return;
  }
  // 2. merge: the extension's thread folds the pair into whichever of the two was seen first (which keeps its LM term and bonus)
#pragma unroll
  for (int m = 0; m < BEAM_PER_THREAD; ++m) {
    const int c = tid + m * BEAM_THREADS, q = match[m];
    if (q < 0) continue;
    const int z = q * kk;
    if (z < c) {
      c_pb[z] = lse2(c_pb[z], c_pb[c]); c_pnb[z] = lse2(c_pnb[z], c_pnb[c]); c_asr[z] = lse2(c_asr[z], c_asr[c]);
      c_id[c] = CAND_NONE;
    } else {
      c_pb[c] = lse2(c_pb[c], c_pb[z]); c_pnb[c] = lse2(c_pnb[c], c_pnb[z]); c_asr[c] = lse2(c_asr[c], c_asr[z]);
      c_id[c] = L[q].id;
      c_id[z] = CAND_NONE;
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
      tot[m] = __dadd_rn(__dadd_rn(c_asr[c], c_lm[c]), c_bonus[c]);   // (asr + lm) + len_bonus
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
      nw.p_b = c_pb[bp]; nw.p_nb = c_pnb[bp]; nw.lm = c_lm[bp]; nw.len_bonus = c_bonus[bp]; nw.total = bt;
      if (j > 0) {
        const int v = tp[j - 1];
        nw.parent = L[i].id; nw.last = v; nw.len = L[i].len + 1;
        nw.n_plain = L[i].n_plain + (v == eos ? 0 : 1);   // an appended <eos> is not a plain label
        nw.id = c_id[bp];
        nw.slot = -1;
        if (nw.id != CAND_NEW)                            // folded with its live twin: that prefix keeps its row
          for (int q = 0; q < n_live; ++q)
            if (L[q].id == nw.id) nw.slot = L[q].slot;
      }
      N[r] = nw;
    }
    ++n_new;
  }
  // 4. the rows that died one frame ago return to the free list; node ids of the survivors that are new (or formed again)
  if (tid < h.n_dying) h.free_[h.n_free + tid] = h.dying[tid];
  __syncthreads();
  const bool is_new = tid < n_new && N[tid].id == CAND_NEW;
  int full = 0;
  if (is_new) {
    const int id = trie_find_or_add(tab, mask, N[tid].parent, N[tid].last);
    N[tid].id = id;
    full = id < 0;
  }
  // 5. rows of the LM pool and records for the new prefixes (all in the first wave: W <= 32)
  if (wave == 0) {
    const int nf = h.n_free + h.n_dying;
    const u64 bal = __ballot(is_new);
    const int n_rec = __popcll(bal), rank = __popcll(bal & ((1ull << lane) - 1ull));
    int base = 0, v = 0;
    if (lane == 0) {
      if (n_rec > nf) v = BEAM_NO_SLOT;
      else if (n_rec > 0) {
        base = atomicAdd(rec_count, n_rec);
        if (base < 0 || base + n_rec > rec_cap) v = BEAM_WS_SHORT;
      }
      verdict = v;
    }
    base = __shfl(base, 0, 64);
    v = __shfl(v, 0, 64);
    if (is_new && v == 0) {
      int parent_slot = -1;
      for (int q = 0; q < n_live; ++q)
        if (L[q].id == N[tid].parent) parent_slot = L[q].slot;
      const int slot = h.free_[nf - 1 - rank];
      N[tid].slot = slot;
      const long r = base + rank;
      rec[r] = s; rec[rec_cap + r] = N[tid].id; rec[2 * (long)rec_cap + r] = N[tid].parent; rec[3 * (long)rec_cap + r] = N[tid].last;
      rec[4 * (long)rec_cap + r] = parent_slot; rec[5 * (long)rec_cap + r] = slot;
    }
    if (lane == 0) h.n_free = nf - n_rec;
  }
  if (__syncthreads_or(full)) {
    if (tid == 0) { atomicOr(status, BEAM_WS_SHORT); gh->dead = 1; }
    return;
  }
  if (verdict) {
    if (tid == 0) { atomicOr(status, verdict); gh->dead = 1; }
    return;
  }
  // the rows of the prefixes that leave the beam now wait one frame: this frame's records may name them as parents
  if (wave == 0) {
    bool dies = false;
    if (tid < n_live) {
      dies = true;
      for (int r = 0; r < n_new; ++r)
        if (N[r].id == L[tid].id) dies = false;
    }
    const u64 bal = __ballot(dies);
    if (dies) h.dying[__popcll(bal & ((1ull << lane) - 1ull))] = L[tid].slot;
    if (lane == 0) { h.n_dying = __popcll(bal); h.n_live = n_new; }
  }
  __syncthreads();
  for (int i = tid; i < HEAD_WORDS; i += BEAM_THREADS) ((int*)gh)[i] = ((const int*)&h)[i];
  for (int i = tid; i < n_new * 16; i += BEAM_THREADS) ((int*)gl)[i] = ((const int*)live[1])[i];
}

__global__ __launch_bounds__(64) void ctc_beam_lm_finish_kernel(
    int S, int W, int max_frames, int eos, int* __restrict__ out_tok, int* __restrict__ out_len, double* __restrict__ out_score,
    int* __restrict__ out_n, const unsigned char* __restrict__ ws, long ws_bytes) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const Live* gl = (const Live*)(ws + (long)s * STATE_BYTES);
  const Head* gh = (const Head*)(gl + BEAM_MAX_W);
  const unsigned mask = gh->mask;
  const int n_live = gh->n_live;
  const bool ok = !gh->dead && n_live >= 1 && n_live <= W && (long)(mask + 1) * 8 <= trie_share(W, max_frames) &&
                  (long)S * STATE_BYTES + (long)(s + 1) * trie_share(W, max_frames) <= ws_bytes;
  if (tid == 0) out_n[s] = ok ? n_live : -1;
  if (!ok || tid >= n_live) return;
  const u64* tab = (const u64*)(ws + (long)S * STATE_BYTES + (long)s * trie_share(W, max_frames));
  const Live p = gl[tid];
  const long o = (long)s * W + tid;
  const int len = p.len < 1 ? 1 : (p.len > max_frames + 1 ? max_frames + 1 : p.len);
  out_len[o] = len;
  out_score[o] = p.total;
  int* tok = out_tok + o * ((long)max_frames + 1);
  int id = p.id;
  for (int pos = len - 1; pos >= 1 && id >= 1 && (unsigned)(id - 1) <= mask; --pos) {
    const u64 key = __hip_atomic_load(tab + (id - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tok[pos] = (int)(unsigned)(key & 0xFFFFFFFFu) - 1;
    id = (int)(key >> 32);
  }
  tok[0] = eos;
}

long ws_need(int S, int max_frames, int W) { return (long)S * (STATE_BYTES + BEAM_WS_BYTES_PER_NODE * ((long)W * max_frames + 1)); }

}  // namespace

extern "C" long emoasr_ctc_beam_lm_ws_bytes(int S, int max_frames, int W) {
  if (S < 0 || max_frames < 0 || W < 1 || W > BEAM_MAX_W) return -1;
  return ws_need(S, max_frames, W);
}

extern "C" long emoasr_ctc_beam_lm_slots(int W) { return W < 1 || W > BEAM_MAX_W ? -1 : 2 * W + 2; }

extern "C" int emoasr_ctc_beam_lm_init(int S, int B, int W, const int* row_off, const int* utt, int eos, int max_frames, int slots,
                                       void* ws, long ws_bytes, int* rec, int rec_cap, int* rec_count, int* status, void* stream) {
  if (S == 0) return 0;
  EMO_CHECK(W >= 1 && W <= BEAM_MAX_W, "ctc_beam_lm_init: beam width %d is outside 1..%d", W, BEAM_MAX_W);
  EMO_CHECK(S > 0 && B > 0 && max_frames >= 0 && slots >= 1 && (long)S * slots <= INT_MAX, "ctc_beam_lm_init: S=%d B=%d max_frames=%d slots=%d",
            S, B, max_frames, slots);
  EMO_CHECK(row_off && utt && ws && rec && rec_count && status, "ctc_beam_lm_init: null argument");
  EMO_CHECK(rec_cap >= S && ws_bytes >= (long)S * STATE_BYTES, "ctc_beam_lm_init: rec_cap=%d ws_bytes=%ld for %d searches", rec_cap,
            ws_bytes, S);
  if (hipMemsetAsync(rec_count, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) { emo_set_error("ctc_beam_lm_init: memset failed"); return 2; }
  ctc_beam_lm_init_kernel<<<S, BEAM_THREADS, 0, (hipStream_t)stream>>>(S, B, W, row_off, utt, eos, max_frames, slots,
                                                                        (unsigned char*)ws, ws_bytes, rec, rec_cap, rec_count, status);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_beam_lm_frame(int S, int B, int V, int W, int k, int t, const float* logp, long ld, const int* row_off,
                                        const int* top, const int* utt, const double* lm_weight, const double* len_weight, int blank,
                                        int eos, int max_frames, const float* lm_logp, long ld_lm, void* ws, long ws_bytes, int* rec,
                                        int rec_cap, int* rec_count, int* status, void* stream) {
  if (S == 0) return 0;
  EMO_CHECK(W >= 1 && W <= BEAM_MAX_W, "ctc_beam_lm_frame: beam width %d is outside 1..%d", W, BEAM_MAX_W);
  EMO_CHECK(S > 0 && B > 0 && V >= 1 && k >= 1 && k <= W && k <= V && ld >= V && ld_lm >= V && t >= 0 && t < max_frames,
            "ctc_beam_lm_frame: S=%d B=%d V=%d W=%d k=%d ld=%ld ld_lm=%ld t=%d max_frames=%d", S, B, V, W, k, ld, ld_lm, t, max_frames);
  EMO_CHECK(blank >= 0 && blank < V && eos >= 0 && eos < V, "ctc_beam_lm_frame: blank %d / eos %d outside the %d labels", blank, eos, V);
  EMO_CHECK(logp && row_off && top && utt && lm_weight && len_weight && lm_logp && ws && rec && rec_count && status,
            "ctc_beam_lm_frame: null argument");
  EMO_CHECK(rec_cap >= 1 && ws_bytes >= (long)S * STATE_BYTES, "ctc_beam_lm_frame: rec_cap=%d ws_bytes=%ld for %d searches", rec_cap,
            ws_bytes, S);
  if (hipMemsetAsync(rec_count, 0, sizeof(int), (hipStream_t)stream) != hipSuccess) { emo_set_error("ctc_beam_lm_frame: memset failed"); return 2; }
  ctc_beam_lm_frame_kernel<<<S, BEAM_THREADS, 0, (hipStream_t)stream>>>(S, B, V, W, k, t, logp, ld, row_off, top, utt, lm_weight,
                                                                         len_weight, blank, eos, max_frames, lm_logp, ld_lm,
                                                                         (unsigned char*)ws, ws_bytes, rec, rec_cap, rec_count, status);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_ctc_beam_lm_finish(int S, int W, int max_frames, int eos, int* out_tok, int* out_len, double* out_score,
                                         int* out_n, const void* ws, long ws_bytes, void* stream) {
  if (S == 0) return 0;
  EMO_CHECK(W >= 1 && W <= BEAM_MAX_W, "ctc_beam_lm_finish: beam width %d is outside 1..%d", W, BEAM_MAX_W);
  EMO_CHECK(S > 0 && max_frames >= 0 && out_tok && out_len && out_score && out_n && ws && ws_bytes >= (long)S * STATE_BYTES,
            "ctc_beam_lm_finish: S=%d max_frames=%d ws_bytes=%ld", S, max_frames, ws_bytes);
  ctc_beam_lm_finish_kernel<<<S, 64, 0, (hipStream_t)stream>>>(S, W, max_frames, eos, out_tok, out_len, out_score, out_n,
                                                                (const unsigned char*)ws, ws_bytes);
  EMO_LAUNCH_CHECK();
  return 0;
}
