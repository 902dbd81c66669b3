// The bookkeeping of one output step of S lockstep searches, ONE copy of its arithmetic for emoasr_beam_update_batch
// (csrc/decode_batch.hip: one LM weight for the launch) and emoasr_beam_update_cells (csrc/decode_grid.hip: one per search).
#pragma once
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

// After the S workgroups of a step (stream order): advance the shared position once and tell the host.  ctl = {all searches
// finished}.  A step replayed after the end finds ctl[0] set and changes nothing.
__device__ __forceinline__ void beam_batch_tail_body(const emoasr_beam_update_batch_t& b) {
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
