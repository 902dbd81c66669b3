// Kernels of the BATCHED joint CTC / attention beam search (modeling/beam_search_device.py:joint_beam_search_device_batch):
// S searches of width W occupy rows s * W .. s * W + W - 1 of every per-hypothesis array and step in lockstep.
//   * emoasr_attn_step_group: single-query cross-attention of the W hypotheses of a search against that search's OWN
//     projected memory [T_s, 2 dd] -- the memory is stored once per utterance (no per-beam replica), and a K / V tile is
//     fetched once for all W queries;
//   * emoasr_beam_update_batch: beam_update_kernel (csrc/decode_rt.hip) with one workgroup per search, and a one-thread
//     tail launch that advances the shared output position and writes the host's mirror.
// The bodies of both are csrc/attn_group_body.h and csrc/beam_update_batch_body.h, shared with csrc/decode_grid.hip.
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"
#include "attn_group.h"
#include "beam_update_batch.h"

namespace {

// One workgroup per (search s, head h): attn_group_body on the search's rows and the search's memory.
template <typename T, int DK, int TK, int WB>
__global__ __launch_bounds__(G_THREADS) void attn_step_group_kernel(int W, int H, const T* __restrict__ q, const T* __restrict__ kv,
                                                                    const int* __restrict__ moff, float scale, T* __restrict__ out) {
#define EMO_ATTN_GROUP_OF_BLOCK                 \
  const int s = blockIdx.x, h = blockIdx.y;     \
  const long r0 = moff[s];                      \
  const int Ts = moff[s + 1] - moff[s];
#define EMO_ATTN_ROW(w) ((long)s * W + w)
#include "attn_group_body.h"
#undef EMO_ATTN_ROW
#undef EMO_ATTN_GROUP_OF_BLOCK
}

template <typename T>
int launch_group(int S, int W, int H, int dk, const void* q, const void* kv, const int* moff, float scale, void* out, hipStream_t s) {
  dim3 grid(S, H);
#define EMO_ATTN_GROUP_LAUNCH(DK, TK, WB) \
  attn_step_group_kernel<T, DK, TK, WB><<<grid, G_THREADS, 0, s>>>(W, H, (const T*)q, (const T*)kv, moff, scale, (T*)out)
  switch (dk) {
    EMO_ATTN_GROUP_CASE(32, 64, W)
    EMO_ATTN_GROUP_CASE(64, 64, W)
    EMO_ATTN_GROUP_CASE(128, 32, W)
    default:
      emo_set_error("attn_step_group: head width %d (supported: 32, 64, 128)", dk);
      return 1;
  }
#undef EMO_ATTN_GROUP_LAUNCH
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

__global__ __launch_bounds__(256) void beam_update_batch_kernel(emoasr_beam_update_batch_t b) {
#define EMO_UPDATE_MU(s) u.mu
#include "beam_update_batch_body.h"
#undef EMO_UPDATE_MU
}

__global__ void beam_batch_tail_kernel(emoasr_beam_update_batch_t b) { beam_batch_tail_body(b); }

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
