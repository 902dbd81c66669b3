// Masked-LM scoring: the masked copies behind the pseudo-log-likelihood (lm/modeling/bert.py:54-86, lm/test_ppl.py:77-133).
//
//   emoasr_mlm_expand   a batch of B token sequences ys [B, N] (lengths ylens) has R = sum(ylens) masked copies: copy r belongs to
//                       the sequence b with row0[b] <= r < row0[b+1] (row0: prefix sums of ylens) and masks its position
//                       pos = r - row0[b].  The kernel writes the copies r_begin .. r_begin + r_count - 1 -- ids padded to Np, the
//                       key length, the flat row of the masked position and the token it hid -- so the [R, N] image is built
//                       where the encoder reads it and a caller can walk R in chunks that begin and end inside a sequence.
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int kWaves = 4;   // output rows per 256-thread block: one wave each

__global__ __launch_bounds__(64 * kWaves) void mlm_expand_kernel(int B, int N, int Np, const int* __restrict__ ys,
                                                                 const int* __restrict__ ylens, const int* __restrict__ row0,
                                                                 int r_begin, int r_count, int mask_id, int pad_id,
                                                                 int* __restrict__ ids, int* __restrict__ klens,
                                                                 int* __restrict__ idx, int* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));   // (one value per wave)
  if (j >= r_count) return;
  const int r = r_begin + j;
  // the last b with row0[b] <= r (sequences of length 0 share their successor's start and are stepped over); every lane walks the
  // same path
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (row0[mid] <= r) lo = mid; else hi = mid;
  }
  const int b = lo;
  const int len = min(max(ylens[b], 0), N);
  const int pos = r - row0[b];
  const bool inside = pos >= 0 && pos < len;     // (false only for a copy index past R: the row is written as padding)
  const int* __restrict__ y = ys + (long)b * N;
  int* __restrict__ out = ids + (long)j * Np;
  for (int n = lane; n < Np; n += 64) out[n] = n < len ? (n == pos ? mask_id : y[n]) : pad_id;
  if (lane == 0) {
    klens[j] = len;
    idx[j] = j * Np + (inside ? pos : 0);
    labels[j] = inside ? y[pos] : pad_id;
  }
}

}  // namespace

extern "C" int emoasr_mlm_expand(int B, int N, int Np, const int* ys, const int* ylens, const int* row0, int r_begin, int r_count,
                                 int mask_id, int pad_id, int* ids, int* klens, int* idx, int* labels, void* stream) {
  EMO_CHECK(B >= 1 && N >= 1 && Np >= N, "mlm_expand: B=%d N=%d Np=%d", B, N, Np);
  EMO_CHECK(r_begin >= 0 && r_count >= 1, "mlm_expand: r_begin=%d r_count=%d", r_begin, r_count);
  EMO_CHECK((long)r_begin + r_count <= (long)B * N, "mlm_expand: copies %d..%d of at most B * N = %ld", r_begin,
            r_begin + r_count, (long)B * N);
  EMO_CHECK((long)r_count * Np <= 0x7fffffffL, "mlm_expand: r_count * Np = %ld overflows the flat row index", (long)r_count * Np);
  EMO_CHECK(mask_id >= 0 && pad_id >= 0, "mlm_expand: mask_id=%d pad_id=%d", mask_id, pad_id);
  EMO_CHECK(ys && ylens && row0 && ids && klens && idx && labels, "mlm_expand: null argument");
  const int blocks = (r_count + kWaves - 1) / kWaves;
  mlm_expand_kernel<<<blocks, 64 * kWaves, 0, (hipStream_t)stream>>>(B, N, Np, ys, ylens, row0, r_begin, r_count, mask_id, pad_id,
                                                                     ids, klens, idx, labels);
  EMO_LAUNCH_CHECK();
  return 0;
}
