// Batched CTC prefix beam search WITH LM shallow fusion on the device, one frame per launch (CTCDecoder._beam_search with lm /
// lm_weight, asr/modeling/decoders/ctc.py:203-344).  A *search* is one (utterance, (lm_weight, len_weight)) pair: S searches run
// over B utterances, several of them may name the same utterance (the cells of a fusion grid) and then share its logp / top rows,
// which are only read.  Results equal the host search of csrc/ctc_beam_host.hip fed the same f32 LM rows: the same hypotheses in
// the same order, the same sequence of double operations per value.
//
//   emoasr_ctc_beam_lm_init    every search becomes the root (<eos>) holding slot 0 of its share of the LM pool; its trie is cleared;
//                              one record per search asks for the root's LM row (src = -1: from the zero state).
//   emoasr_ctc_beam_lm_frame   one 256-thread workgroup per search advances it by frame t (a search whose utterance is shorter
//                              returns at once).  Steps 0-4 are csrc/ctc_beam_step.h's, the frame body it shares with
//                              csrc/ctc_beam.hip (LM scan, candidates, merge, select, identity); with lm_weight <= 0 the LM term
//                              stays 0.0 and the search is that of ctc_beam.hip, bit for bit.  This file adds
//     5. slots        a survivor that is an extension without a live twin is a NEW prefix: it takes a row of the LM pool from the
//                     search's free list and emits a record (search, node, parent node, label, parent's row, its row); the caller
//                     runs the LM over the records before the next launch.  The row of a prefix that left the beam is freed at the
//                     start of the NEXT frame: this frame's records may still name it as a parent.  Held at once: <= W live after
//                     the previous frame + <= W taken now = 2 W rows.  An empty free list retires the search (status bit 5).
//   emoasr_ctc_beam_lm_finish  token sequences by walking the trie keys back to the root, as ctc_beam.hip ends.
//
// State between launches lives in the workspace: per search a block (live set, free list, dying list) and a trie share sized for
// max_frames.  Stores are plain stores plus the trie's compare-and-swap and the atomic adds of the record count / status word.
// This file owns that state (Head, its checks, load and store), step 5 and the init and finish kernels.
#include "ctc_beam_step.h"

namespace {

constexpr int BEAM_MAX_SLOTS = 2 * BEAM_MAX_W + 2;   // rows of the LM pool one search ever uses
constexpr int BEAM_FREE_CAP = 72;                    // >= BEAM_MAX_SLOTS, keeps the head a multiple of 8 bytes

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

__device__ __forceinline__ long trie_share(int W, int max_frames) { return BEAM_WS_BYTES_PER_NODE * ((long)W * max_frames + 1); }

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
  const unsigned tslots = trie_slots((long)W * frames + 1);
  trie_clear(tab, tslots);
  const int nslot = slots < BEAM_MAX_SLOTS ? slots : BEAM_MAX_SLOTS;
  const int base = s * slots;
  for (int i = tid; i < nslot - 1; i += BEAM_THREADS) gh->free_[i] = base + nslot - 1 - i;   // (taken from the end: 1, 2, ...)
  if (tid == 0) {
    gl[0] = live_root(base);
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
  __shared__ Live live[2][BEAM_MAX_W];
  __shared__ Head h;
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
  // the rows that died one frame ago return to the free list (step 5 reads it, behind the barriers of the frame step)
  if (tid < h.n_dying) h.free_[h.n_free + tid] = h.dying[tid];
  const Live* L = live[0];
  Live* N = live[1];
  const int n_new = beam_frame_step<true>(L, N, n_live, logp + (r0 + t) * ld, top + (r0 + t) * (long)k, V, W, k, blank, eos,
                                          lm_weight[s], len_weight[s], lm_logp, ld_lm);
  if (n_new < 0) {
    if (tid == 0) { atomicOr(status, BEAM_BAD_LABEL); gh->dead = 1; }
    return;
  }
  int full;
  const bool is_new = beam_new_ids(N, n_new, tab, mask, &full);
  // 5. rows of the LM pool and records for the new prefixes (all in the first wave: W <= 32).  free_[0 .. n_free + n_dying) is
  //    the whole free list here: the rows that waited one frame were appended above, before the frame step.
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
  beam_back_walk(tab, mask, p.id, len, eos, out_tok + o * ((long)max_frames + 1));
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
