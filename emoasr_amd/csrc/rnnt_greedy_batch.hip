// The bookkeeping of the transducer's time-synchronous greedy search (asr/modeling/decoders/rnn_transducer.py:194-240) for S
// utterances in LOCKSTEP, on the device (engine.rnnt_greedy_batch).
//
// One step of the search is a chain of launches that the engine captures once and replays:
//
//   emoasr_rnnt_beam_lstm_rows  x layers   S rows: the searches that emitted a label in the step before consume it
//   emoasr_rnnt_beam_joint_rows            S K rows: up to K consecutive frames of every live search against its current state
//   emoasr_gemm_nt                         the output layer over the S K rows
//   emoasr_rnnt_greedy_batch_book          this file: arg-max of every active row, the reference's rule, the next step's words
//
// While the arg-max is blank the prediction network does not move, so the K frames t .. t + K - 1 of a search can be scored against
// the SAME decoder state (the window of engine._rnnt_greedy_chain).  The first non-blank row k of the window is the reference's next
// emission: k blanks and the token go to the alignment, t advances by k (the search stays on the emitting frame), the rows behind k
// are discarded and one LSTM step is scheduled.  A window of blanks advances t by its active rows and schedules nothing.
//
// Control words (int64, one array): 4 S words for the LSTM rows -- label, source slot, destination slot, active -- then 3 S K words
// for the joint rows -- slot of the state to read, active, row of the stacked [sum of T, J] matrix w_enc . eouts + b.  Search s owns
// the slots 2 s and 2 s + 1 of every layer's state pool and alternates between them: emoasr_rnnt_beam_lstm_rows splits the hidden
// units over workgroups, each of which stages the whole previous h, so a step in place would let one workgroup overwrite what
// another is still reading.  An inactive row's words are all zero.
//
// A search finishes when t reaches its frame count or once its hypothesis is longer than max_len (the reference breaks AFTER the
// label that exceeds the limit: max_len + 1 labels are kept).  A finished search leaves every row of its own inactive and is not
// touched again: replaying the step after the end changes nothing.  *live counts the unfinished searches; the engine polls it.
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int GB_KMAX = EMOASR_RNNT_GREEDY_BATCH_MAX_FRAMES;

struct GreedyBatchArgs {
  int S, K, V, blank, eos, max_len;
  const int* row_off;                   // [S + 1] frames before search s in the stacked e matrix
  const void* logits; long ldl;         // [S K][ldl] of the compute dtype
  long long* ctl;                       // [4 S + 3 S K]
  int* state;                           // [S][4]: t, current slot (0 / 1), finished, unused
  int* hyp; long ldh;                   // [S][ldh], ldh >= max_len + 1
  int* align; long lda;                 // [S][lda], lda >= T_s + max_len + 1
  int* lens;                            // [S][2]: len(hyp), len(align)
  int* live;                            // [1]: searches not finished
};

__device__ __forceinline__ void lstm_words(const GreedyBatchArgs& a, int s, long long label, long long src, long long dst, long long on) {
  long long* w = a.ctl;
  w[s] = label; w[a.S + s] = src; w[2 * a.S + s] = dst; w[3 * a.S + s] = on;
}

// the joint rows s K .. s K + K - 1: frames t .. t + K - 1 of search s against the state in `slot`; rows past T are inactive
__device__ __forceinline__ void joint_words(const GreedyBatchArgs& a, int s, int i, int slot, int t, int T, bool live) {
  const long R = (long)a.S * a.K, r = (long)s * a.K + i;
  long long* w = a.ctl + 4 * (long)a.S;
  const bool on = live && t + i < T;
  w[r] = on ? slot : 0; w[R + r] = on ? 1 : 0; w[2 * R + r] = on ? (long long)a.row_off[s] + t + i : 0;
}

// one workgroup: thread <-> search (S is a few hundred at the most)
__global__ __launch_bounds__(256) void rnnt_greedy_batch_start_kernel(const GreedyBatchArgs a) {
  int n_live = 0;
  for (int s0 = 0; s0 < a.S; s0 += 256) {
    const int s = s0 + threadIdx.x;
    int on = 0;
    if (s < a.S) {
      const int T = a.row_off[s + 1] - a.row_off[s];
      on = T > 0;
      // <eos> from the zero state of slot 2 s into slot 2 s + 1; the first window reads slot 2 s + 1
      lstm_words(a, s, on ? a.eos : 0, on ? 2 * s : 0, on ? 2 * s + 1 : 0, on);
      for (int i = 0; i < a.K; ++i) joint_words(a, s, i, 2 * s + 1, 0, T, on);
      a.state[4 * s] = 0; a.state[4 * s + 1] = 1; a.state[4 * s + 2] = !on; a.state[4 * s + 3] = 0;
      a.lens[2 * s] = 0; a.lens[2 * s + 1] = 0;
    }
    n_live += __syncthreads_count(on);
  }
  if (threadIdx.x == 0) *a.live = n_live;
}

// arg-max of one row by one wave: the first maximum (emoasr_argmax_rows' order: greater wins, equal -> the lower index).  A row
// without any value that compares (all NaN, or all -inf) gives index 0, as emoasr_argmax_rows does: a blank where blank is 0.
template <typename T>
__device__ __forceinline__ int wave_argmax(const T* __restrict__ row, int V, int lane) {
  float m = -INFINITY; int mi = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float c = to_f32(row[v]);
    if (c > m || (c == m && v < mi)) { m = c; mi = v; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  return mi == 0x7fffffff ? 0 : mi;
}

// one WAVE per search (no workgroup barrier anywhere)
template <typename T>
__global__ __launch_bounds__(64) void rnnt_greedy_batch_book_kernel(const GreedyBatchArgs a) {
  const int s = blockIdx.x, lane = threadIdx.x, K = a.K;
  int* st = a.state + 4 * s;
  if (st[2]) return;                                  // finished: its rows are inactive and stay so
  const int nT = a.row_off[s + 1] - a.row_off[s];     // frames of the search
  int t = st[0], cur = st[1], nh = a.lens[2 * s], na = a.lens[2 * s + 1];
  const int n = min(K, nT - t);                       // active rows of the window (>= 1: the search is live)
  const T* rows = static_cast<const T*>(a.logits) + (long)s * K * a.ldl;
  int k = 0, tok = a.blank;
  for (; k < n; ++k) {                                // (uniform over the wave)
    tok = wave_argmax<T>(rows + (long)k * a.ldl, a.V, lane);
    if (tok != a.blank) break;
  }
  int* al = a.align + (long)s * a.lda;
  const int room = (int)min((long)nT + a.max_len + 1, a.lda) - na;   // (never short: <= nT blanks and <= max_len + 1 labels)
  const int nblank = min(k, room);
  for (int i = lane; i < nblank; i += 64) al[na + i] = a.blank;
  const bool emit = k < n && nh < a.ldh && nh <= a.max_len && k < room;
  bool done;
  if (emit) {
    if (lane == 0) { al[na + k] = tok; a.hyp[(long)s * a.ldh + nh] = tok; }
    na += k + 1; nh += 1; t += k;                     // the label is emitted AT frame t + k: the search stays on it
    done = nh > a.max_len;
  } else {
    na += nblank; t += k;
    done = t >= nT || k < n;                          // (k < n here: no room left for a label -- cannot happen, ends the search)
  }
  if (lane == 0) {
    const bool step = emit && !done;
    lstm_words(a, s, step ? tok : 0, step ? 2 * s + cur : 0, step ? 2 * s + (cur ^ 1) : 0, step);
    if (step) cur ^= 1;
    st[0] = t; st[1] = cur; st[2] = done;
    a.lens[2 * s] = nh; a.lens[2 * s + 1] = na;
    if (done) atomicSub(a.live, 1);
  }
  cur = __shfl(cur, 0, 64);
  if (lane < K) joint_words(a, s, lane, 2 * s + cur, t, nT, !done);
}

int greedy_batch_check(const char* who, int S, int K, int max_len, const void* row_off, const void* ctl, const void* state,
                       const void* lens, const void* live) {
  EMO_CHECK(S > 0 && S <= (1 << 20), "%s: S=%d", who, S);
  EMO_CHECK(K >= 1 && K <= GB_KMAX, "%s: frames per step %d is outside 1..%d", who, K, GB_KMAX);
  EMO_CHECK(max_len >= 0, "%s: max_len=%d", who, max_len);
  EMO_CHECK(row_off && ctl && state && lens && live, "%s: null argument", who);
  return 0;
}

}  // namespace

extern "C" int emoasr_rnnt_greedy_batch_start(int S, int K, int eos, int max_len, const int* row_off, long long* ctl, int* state,
                                              int* lens, int* live, void* stream) {
  if (S == 0) return 0;
  if (int rc = greedy_batch_check("rnnt_greedy_batch_start", S, K, max_len, row_off, ctl, state, lens, live)) return rc;
  EMO_CHECK(eos >= 0, "rnnt_greedy_batch_start: eos=%d", eos);
  GreedyBatchArgs a{S, K, 0, 0, eos, max_len, row_off, nullptr, 0, ctl, state, nullptr, 0, nullptr, 0, lens, live};
  rnnt_greedy_batch_start_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_rnnt_greedy_batch_book(int dtype, int S, int K, int V, int blank, int max_len, const int* row_off,
                                             const void* logits, long ldl, long long* ctl, int* state, int* hyp, long ldh, int* align,
                                             long lda, int* lens, int* live, void* stream) {
  if (S == 0) return 0;
  if (int rc = greedy_batch_check("rnnt_greedy_batch_book", S, K, max_len, row_off, ctl, state, lens, live)) return rc;
  EMO_CHECK(V >= 1 && blank >= 0 && blank < V && logits && ldl >= V, "rnnt_greedy_batch_book: V=%d blank=%d ldl=%ld", V, blank, ldl);
  EMO_CHECK(hyp && align && ldh >= (long)max_len + 1 && lda >= (long)max_len + 1, "rnnt_greedy_batch_book: ldh=%ld lda=%ld max_len=%d",
            ldh, lda, max_len);
  GreedyBatchArgs a{S, K, V, blank, 0, max_len, row_off, logits, ldl, ctl, state, hyp, ldh, align, lda, lens, live};
  EMO_DISPATCH(dtype, (rnnt_greedy_batch_book_kernel<T><<<S, 64, 0, (hipStream_t)stream>>>(a)));
  EMO_LAUNCH_CHECK();
  return 0;
}
