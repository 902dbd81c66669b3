// The bookkeeping of the transducer's alignment-length-synchronous beam search on the device (asr/modeling/decoders/
// rnn_transducer.py:264-321, 348-359; engine._rnnt_beam_search_graph does the same on the host): after the pick kernel of every
// expansion round, one wave per search reads the round's records, appends the blank extensions to the frame list, forms the grown
// candidates, orders them (stable, by double score), merges equal label sequences by log-add, cuts to the beam, and writes the
// NEXT round's control words -- so a frame of num_expands rounds is a linear chain of launches with no host round trip, and S
// searches of W rows each share every launch (csrc/rnnt_beam.hip: emoasr_rnnt_beam_lstm_rows / _joint_rows).
//
//   emoasr_rnnt_beam_start    every search: beams = [(<sos>), score 0, slot 0], frame 0, round 0; the trie cleared; the control
//                             words of round 0.  A search without frames is finished at once.
//   emoasr_rnnt_beam_book     one round's bookkeeping (below) + the next round's control words.  A finished search returns at
//                             once: its rows stay inactive, its beams stay what they were.
//   emoasr_rnnt_beam_finish   out_tok / out_len / out_score / out_n, best first (the layout of emoasr_ctc_beam_batch).
//
// A hypothesis is (score, node id, length, last label, slot): the slot holds the LSTM state from BEFORE its last label (a blank
// extension keeps it, :290-294), the node id is the canonical id of its label sequence in the search's trie (csrc/ctc_beam_step.h:
// a prefix that drops out and is formed again finds its old id).  Only survivors of a cut get ids: <= W per round that grows.
//
// One round, for a search at (frame t, round v) with n live rows:
//     1. frame list  += (live_i, score_i + blank_i, slot_i)
//     2. v < E - 1:  candidates c = i W + k: (live_i + label_ik, score_i + val_ik, dst_i).  The live label sequences are distinct
//                    and a row's k labels are distinct, so no two candidates are the same sequence: the merge of the host loop
//                    never folds here, and the cut is W rounds of arg-max over (score descending, position ascending) -- what a
//                    stable sort leaves in front.  The W survivors get their ids from the trie.
//     3. v == E - 1: the frame list (<= E W entries, all with ids) is ranked the same way; one lane walks it in that order and
//                    folds every entry into the first one with its id (lse2, first operand the running sum: the host's
//                    np.logaddexp(seen, score) sequence), keeping the first W distinct ones: the next frame's beams, which are
//                    the live rows of its round 0.
//     4. slots:      mark every slot of the search's region that {live, frame list, beams} reference, hand the lowest free ones
//                    to the live rows as destinations.  (E + 1) W slots always suffice: before round v the frame list references
//                    <= v W slots and the live rows <= W, v <= E - 1, and W destinations are needed.  A destination is therefore
//                    never a source of the same launch (csrc/rnnt_beam.hip: other workgroups may still be staging that slot).
//     5. control words [5][R] (int64; row s W + i): last label, source slot, destination slot, active flag, row of frame t in the
//                    stacked e matrix (row_off[s] + t).  Slots are global: s (E + 1) W + the slot inside the region.
//
// Plain C++ throughout; every double operation is written once and nothing is contracted (-ffp-contract=off).
#include "ctc_beam_step.h"

namespace {

constexpr int BK_W = EMOASR_RNNT_BEAM_MAX_WIDTH;        // 16
constexpr int BK_E = EMOASR_RNNT_BEAM_MAX_EXPANDS;      // 15
constexpr int BK_FRAME = BK_W * BK_E;                   // entries of a frame list
constexpr int BK_SLOTS = BK_W * (BK_E + 1);             // 256 slots of a region: four 64-bit words of marks
constexpr int BK_THREADS = 64;
constexpr int BK_PER_THREAD = (BK_W * BK_W + BK_THREADS - 1) / BK_THREADS;   // 4 (>= BK_FRAME / 64 as well)
static_assert(BK_FRAME <= BK_PER_THREAD * BK_THREADS, "a lane ranks at most BK_PER_THREAD entries of the frame list");

struct Hyp {
  double score;
  int id, len, last, slot;   // slot: inside the search's region
  int dst, pad;              // live rows: the destination slot of the round that is (or was just) run
};
static_assert(sizeof(Hyp) == 32, "the workspace layout counts 32 bytes per hypothesis");

struct BookState {
  int t, v, n_beam, n_live, n_frame, done, err, pad;
  Hyp beam[BK_W], live[BK_W], frame[BK_FRAME];
};
static_assert(sizeof(BookState) == EMOASR_RNNT_BEAM_STATE_BYTES, "emoasr_hip.h states the size of a search's fixed state");

struct BookArgs {
  int S, W, E, V, eos;
  const int* row_off;          // [S + 1]: frames before search s in the stacked e matrix
  const float* rec; long ldr;  // [S W][ldr]: blank, W values, W ids relative to column 1
  long long* ctl;              // [5][S W]
  unsigned char* ws; long ws_bytes;
  int* status;
};

__device__ __forceinline__ long nodes_of(long frames, int W, int E) { return (long)W * frames * (E - 1) + 1; }

// the search's state and trie inside the workspace; -> 0 or the refusal
__device__ __forceinline__ int book_places(const BookArgs& a, int s, BookState** st, u64** tab, unsigned* mask) {
  const long r0 = a.row_off[s], r1 = a.row_off[s + 1];
  if (r0 < 0 || r1 < r0) return BEAM_BAD_OFFSETS;
  const long cap = nodes_of(r1 - r0, a.W, a.E);
  if (cap > BEAM_MAX_NODES) return BEAM_TOO_LONG;
  const long base = (long)a.S * (long)sizeof(BookState);
  const long lo = base + BEAM_WS_BYTES_PER_NODE * ((long)a.W * (a.E - 1) * r0 + s);
  const long hi = base + BEAM_WS_BYTES_PER_NODE * ((long)a.W * (a.E - 1) * r1 + s + 1);
  if ((long)(s + 1) * (long)sizeof(BookState) > a.ws_bytes) return BEAM_WS_SHORT;   // not even the state fits
  *st = reinterpret_cast<BookState*>(a.ws) + s;
  if (hi > a.ws_bytes) return BEAM_WS_SHORT;
  *tab = reinterpret_cast<u64*>(a.ws + lo);
  *mask = trie_slots(cap) - 1;
  return 0;
}

// steps 4 and 5 for a search whose live rows are final (behind a barrier); lane 0 hands out the slots
__device__ __forceinline__ void book_next_round(const BookArgs& a, int s, BookState* st, int lane) {
  __shared__ int s_dst[BK_W];
  const int W = a.W, ns = (a.E + 1) * W;
  const int n_live = st->done ? 0 : st->n_live;
  if (lane == 0) {
    u64 used[BK_SLOTS / 64] = {0, 0, 0, 0};
    auto mark = [&](int slot) { used[(slot >> 6) & (BK_SLOTS / 64 - 1)] |= (u64)1 << (slot & 63); };
    for (int i = 0; i < st->n_live; ++i) mark(st->live[i].slot);
    for (int i = 0; i < st->n_frame; ++i) mark(st->frame[i].slot);
    for (int i = 0; i < st->n_beam; ++i) mark(st->beam[i].slot);
    int next = 0, lost = 0;
    for (int i = 0; i < n_live; ++i) {
      while (next < ns && ((used[next >> 6] >> (next & 63)) & 1)) ++next;
      if (next >= ns) { lost = 1; next = ns - 1; }   // (never: the count above; kept inside the region whatever happens)
      s_dst[i] = next++;
    }
    if (lost) { st->err |= BEAM_NO_SLOT; st->done = 1; atomicOr(a.status, BEAM_NO_SLOT); }
  }
  __threadfence_block();
  __syncthreads();
  const bool dead = st->done != 0;
  const long R = (long)a.S * W, base = (long)s * ns;
  if (lane < W) {
    const long r = (long)s * W + lane;
    const bool on = !dead && lane < n_live;
    if (on) st->live[lane].dst = s_dst[lane];
    a.ctl[0 * R + r] = on ? st->live[lane].last : 0;
    a.ctl[1 * R + r] = base + (on ? st->live[lane].slot : 0);
    a.ctl[2 * R + r] = base + (on ? s_dst[lane] : 0);
    a.ctl[3 * R + r] = on ? 1 : 0;
    a.ctl[4 * R + r] = on ? (long long)a.row_off[s] + st->t : 0;
  }
}

__device__ __forceinline__ void book_refuse(const BookArgs& a, int s, BookState* st, int err, int lane) {
  if (lane == 0) {
    atomicOr(a.status, err);
    if (st) { st->err |= err; st->done = 1; }
  }
  const long R = (long)a.S * a.W;
  if (lane < a.W) {
    const long r = (long)s * a.W + lane;
    a.ctl[0 * R + r] = 0; a.ctl[1 * R + r] = (long)s * (a.E + 1) * a.W; a.ctl[2 * R + r] = (long)s * (a.E + 1) * a.W;
    a.ctl[3 * R + r] = 0; a.ctl[4 * R + r] = 0;
  }
}

__global__ __launch_bounds__(BEAM_THREADS) void rnnt_beam_start_kernel(const BookArgs a) {
  const int s = blockIdx.x, tid = threadIdx.x;
  BookState* st = nullptr; u64* tab = nullptr; unsigned mask = 0;
  const int err = book_places(a, s, &st, &tab, &mask);   // (uniform over the workgroup)
  if (err) { book_refuse(a, s, st, err, tid); return; }
  trie_clear(tab, mask + 1);
  if (tid == 0) {
    st->t = 0; st->v = 0; st->n_beam = 1; st->n_live = 1; st->n_frame = 0; st->err = 0; st->pad = 0;
    st->done = a.row_off[s + 1] == a.row_off[s];
    const Hyp root{0.0, 0, 1, a.eos, 0, 0, 0};
    st->beam[0] = root; st->live[0] = root;
  }
  __threadfence();
  __syncthreads();
  book_next_round(a, s, st, tid);
}

// the arg-max of (score descending, position ascending) over the wave; INT_MAX: nothing left
__device__ __forceinline__ void wave_best(double& bt, int& bp) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ot = __shfl_xor(bt, o, 64);
    const int op = __shfl_xor(bp, o, 64);
    if (beats(ot, op, bt, bp)) { bt = ot; bp = op; }
  }
}

__global__ __launch_bounds__(BK_THREADS) void rnnt_beam_book_kernel(const BookArgs a) {
  __shared__ Hyp L[BK_W];                 // the live rows of the round just run
  __shared__ double f_in[BK_FRAME];       // the frame list's scores as appended ...
  __shared__ double f_score[BK_FRAME];    // ... and ranked
  __shared__ int f_src[BK_FRAME];
  const int s = blockIdx.x, lane = threadIdx.x, W = a.W, E = a.E;
  BookState* st = nullptr; u64* tab = nullptr; unsigned mask = 0;
  const int perr = book_places(a, s, &st, &tab, &mask);
  if (perr) { book_refuse(a, s, st, perr, lane); return; }
  if (st->done) return;                   // finished or refused: rows inactive since, beams final
  const int n_live = st->n_live, v = st->v, t = st->t, n_frame0 = st->n_frame;
  const long frames = a.row_off[s + 1] - a.row_off[s];
  if (lane < n_live) L[lane] = st->live[lane];
  __syncthreads();
  const float* rec = a.rec + (long)s * W * a.ldr;
  // 1. the blank extensions
  if (lane < n_live) {
    Hyp f = L[lane];
    f.score = L[lane].score + (double)rec[lane * a.ldr];
    st->frame[n_frame0 + lane] = f;
  }
  const int n_frame = n_frame0 + n_live;
  const bool last = v == E - 1;
  if (!last) {
    // 2. grown candidates, W rounds of arg-max
    const int nc = n_live * W;
    double sc[BK_PER_THREAD];
    unsigned alive = 0;
    int bad = 0;
#pragma unroll
    for (int m = 0; m < BK_PER_THREAD; ++m) {
      const int c = lane + m * BK_THREADS;
      sc[m] = 0.0;
      if (c < nc) {
        const int i = c / W, k = c - i * W;
        const int lab = (int)rec[i * a.ldr + 1 + W + k] + 1;
        if (lab < 1 || lab >= a.V) bad = 1;
        sc[m] = L[i].score + (double)rec[i * a.ldr + 1 + k];
        alive |= 1u << m;
      }
    }
    if (__syncthreads_or(bad)) { book_refuse(a, s, st, BEAM_BAD_LABEL, lane); return; }
    int n_new = 0;
    for (int r = 0; r < W; ++r) {
      double bt = 0.0;
      int bp = INT_MAX;
#pragma unroll
      for (int m = 0; m < BK_PER_THREAD; ++m)
        if (((alive >> m) & 1u) && (bp == INT_MAX || sc[m] > bt)) { bt = sc[m]; bp = lane + m * BK_THREADS; }
      wave_best(bt, bp);
      if (bp == INT_MAX) break;
      if ((bp & (BK_THREADS - 1)) == lane) {
        alive &= ~(1u << (bp / BK_THREADS));
        const int i = bp / W, k = bp - i * W;
        const int lab = (int)rec[i * a.ldr + 1 + W + k] + 1;
        const int id = trie_find_or_add(tab, mask, L[i].id, lab);
        st->live[r] = Hyp{bt, id, L[i].len + 1, lab, L[i].dst, 0, 0};
        if (id < 0) bad = 1;
      }
      ++n_new;
    }
    if (__syncthreads_or(bad)) { book_refuse(a, s, st, BEAM_WS_SHORT, lane); return; }
    if (lane == 0) { st->n_live = n_new; st->n_frame = n_frame; st->v = v + 1; }
  } else {
    // 3. the frame list: rank (the stable sort), then fold and cut in that order
    __threadfence_block();
    __syncthreads();
    for (int e = lane; e < n_frame; e += BK_THREADS) f_in[e] = st->frame[e].score;
    __syncthreads();
#pragma unroll
    for (int m = 0; m < BK_PER_THREAD; ++m) {
      const int e = lane + m * BK_THREADS;
      if (e >= n_frame) continue;
      const double se = f_in[e];
      int rank = 0;
      for (int j = 0; j < n_frame; ++j) rank += beats(f_in[j], j, se, e) ? 1 : 0;
      f_score[rank] = se; f_src[rank] = e;
    }
    __syncthreads();
    if (lane == 0) {
      int n_out = 0;
      for (int r = 0; r < n_frame; ++r) {
        const Hyp f = st->frame[f_src[r]];
        int hit = -1;
        for (int q = 0; q < n_out; ++q)
          if (st->beam[q].id == f.id) { hit = q; break; }
        if (hit >= 0) st->beam[hit].score = lse2(st->beam[hit].score, f_score[r]);
        else if (n_out < W) st->beam[n_out++] = f;
      }
      for (int q = 0; q < n_out; ++q) st->live[q] = st->beam[q];
      st->n_beam = n_out; st->n_live = n_out; st->n_frame = 0; st->v = 0; st->t = t + 1;
      if (t + 1 >= frames) st->done = 1;
    }
  }
  __threadfence_block();
  __syncthreads();
  book_next_round(a, s, st, lane);
}

__global__ __launch_bounds__(BK_THREADS) void rnnt_beam_finish_kernel(const BookArgs a, int Lmax, int* __restrict__ out_tok,
                                                                      int* __restrict__ out_len, double* __restrict__ out_score,
                                                                      int* __restrict__ out_n) {
  const int s = blockIdx.x, lane = threadIdx.x, W = a.W;
  BookState* st = nullptr; u64* tab = nullptr; unsigned mask = 0;
  int err = book_places(a, s, &st, &tab, &mask);
  if (!err) err = st->err;
  int n = err ? 0 : st->n_beam;
  int bad = 0;
  if (lane < n && st->beam[lane].len > Lmax + 1) bad = 1;
  if (__syncthreads_or(bad)) err = BEAM_TOO_LONG;
  if (err) {
    if (lane == 0) { atomicOr(a.status, err); out_n[s] = -1; }
    return;
  }
  if (lane == 0) out_n[s] = n;
  if (lane < n) {
    const Hyp p = st->beam[lane];
    const long o = (long)s * W + lane;
    out_len[o] = p.len;
    out_score[o] = p.score;
    beam_back_walk(tab, mask, p.id, p.len, a.eos, out_tok + o * ((long)Lmax + 1));
  }
}

int book_check(const char* who, int S, int W, int E, int V, int eos, const void* row_off, const void* ctl, const void* ws,
               long ws_bytes, const void* status) {
  EMO_CHECK(W >= 1 && W <= BK_W, "%s: beam width %d is outside 1..%d", who, W, BK_W);
  EMO_CHECK(E >= 1 && E <= BK_E, "%s: num_expands %d is outside 1..%d", who, E, BK_E);
  EMO_CHECK(S > 0 && V >= 2 && W <= V - 1 && eos >= 0 && eos < V, "%s: S=%d V=%d W=%d eos=%d", who, S, V, W, eos);
  EMO_CHECK(row_off && ctl && ws && status && ws_bytes >= 0, "%s: null argument", who);
  return 0;
}

}  // namespace

extern "C" long emoasr_rnnt_beam_ws_bytes(int S, int total_frames, int W, int num_expands) {
  if (S < 0 || total_frames < 0 || W < 1 || W > BK_W || num_expands < 1 || num_expands > BK_E) return -1;
  return (long)S * EMOASR_RNNT_BEAM_STATE_BYTES + BEAM_WS_BYTES_PER_NODE * ((long)W * total_frames * (num_expands - 1) + S);
}

extern "C" int emoasr_rnnt_beam_start(int S, int W, int num_expands, int V, int eos, const int* row_off, long long* ctl, void* ws,
                                      long ws_bytes, int* status, void* stream) {
  if (S == 0) return 0;
  if (int rc = book_check("rnnt_beam_start", S, W, num_expands, V, eos, row_off, ctl, ws, ws_bytes, status)) return rc;
  BookArgs a{S, W, num_expands, V, eos, row_off, nullptr, 0, ctl, (unsigned char*)ws, ws_bytes, status};
  rnnt_beam_start_kernel<<<S, BEAM_THREADS, 0, (hipStream_t)stream>>>(a);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_rnnt_beam_book(int S, int W, int num_expands, int V, int eos, const int* row_off, const float* rec, long ldr,
                                     long long* ctl, void* ws, long ws_bytes, int* status, void* stream) {
  if (S == 0) return 0;
  if (int rc = book_check("rnnt_beam_book", S, W, num_expands, V, eos, row_off, ctl, ws, ws_bytes, status)) return rc;
  EMO_CHECK(rec && ldr >= 1 + 2 * W, "rnnt_beam_book: a record holds 1 + 2 W = %d floats, ldr = %ld", 1 + 2 * W, ldr);
  BookArgs a{S, W, num_expands, V, eos, row_off, rec, ldr, ctl, (unsigned char*)ws, ws_bytes, status};
  rnnt_beam_book_kernel<<<S, BK_THREADS, 0, (hipStream_t)stream>>>(a);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_rnnt_beam_finish(int S, int W, int num_expands, int V, int eos, const int* row_off, int Lmax, int* out_tok,
                                       int* out_len, double* out_score, int* out_n, void* ws, long ws_bytes, int* status,
                                       void* stream) {
  if (S == 0) return 0;
  if (int rc = book_check("rnnt_beam_finish", S, W, num_expands, V, eos, row_off, out_tok, ws, ws_bytes, status)) return rc;
  EMO_CHECK(Lmax >= 0 && out_len && out_score && out_n, "rnnt_beam_finish: Lmax=%d or a null output", Lmax);
  BookArgs a{S, W, num_expands, V, eos, row_off, nullptr, 0, nullptr, (unsigned char*)ws, ws_bytes, status};
  rnnt_beam_finish_kernel<<<S, BK_THREADS, 0, (hipStream_t)stream>>>(a, Lmax, out_tok, out_len, out_score, out_n);
  EMO_LAUNCH_CHECK();
  return 0;
}
