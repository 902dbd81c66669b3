// Batched CTC prefix beam search on the device, no LM: the N-best producer of `test_asr.py --nbest --beam_width N` on a CTC model
// (CTCDecoder._beam_search and _merge_ctc_paths, asr/modeling/decoders/ctc.py:262-344, 372-397).  Results equal the host search of
// csrc/ctc_beam_host.hip: the same hypotheses in the same order, the same sequence of double operations per value.
//
//   emoasr_ctc_beam_batch  one 256-thread workgroup per utterance walks that utterance's frames in order; nothing leaves the
//                          device until the search is over.  A frame is steps 1-4 of csrc/ctc_beam_step.h (candidates, merge,
//                          select, identity) with no LM term; the two live sets in LDS swap roles from frame to frame.  The
//                          token sequences are rebuilt once, at the end, from the utterance's trie.
//
// This file owns the per-utterance share of the workspace (the trie) and its checks, the frame loop and the output.
#include "ctc_beam_step.h"

namespace {

__global__ __launch_bounds__(BEAM_THREADS) void ctc_beam_batch_kernel(
    int V, int W, int k, const float* __restrict__ logp, long ld, const int* __restrict__ row_off, const int* __restrict__ top,
    int blank, int eos, double len_weight, int max_frames, int* __restrict__ out_tok, int* __restrict__ out_len,
    double* __restrict__ out_score, int* __restrict__ out_n, unsigned char* __restrict__ ws, long ws_bytes,
    int* __restrict__ status) {
  __shared__ Live live[2][BEAM_MAX_W];
  const int b = blockIdx.x, tid = threadIdx.x;
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
  const unsigned slots = trie_slots(cap), mask = slots - 1;
  trie_clear(tab, slots);
  if (tid == 0) live[0][0] = live_root(0);
  __threadfence();
  __syncthreads();

  int n_live = 1, cur = 0;
  for (long t = 0; t < frames; ++t) {
    Live* N = live[cur ^ 1];
    const int n_new = beam_frame_step<false>(live[cur], N, n_live, logp + (r0 + t) * ld, top + (r0 + t) * (long)k, V, W, k, blank,
                                             eos, 0.0, len_weight, nullptr, 0);
    if (n_new < 0) {
      if (tid == 0) { atomicOr(status, BEAM_BAD_LABEL); out_n[b] = -1; }
      return;
    }
    int full;
    beam_new_ids(N, n_new, tab, mask, &full);
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
    beam_back_walk(tab, mask, p.id, p.len, eos, out_tok + o * ((long)max_frames + 1));
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
