// ELECTRA (lm/modeling/electra.py:20-132): what sits between the generator and the discriminator, and the discriminator's head.
//
//   emoasr_sample_rows      one pass over a logits row: log-sum-exp, the cross-entropy row -w * (z[label] - lse) and a Gumbel-max
//                           sample argmax_v (z[v] + g(seed, row, v)) -- a draw from softmax(z) that is a pure function of
//                           (seed, row, column), ties to the lowest column.  The reference's softmax over [B, N, V] + multinomial.
//   emoasr_gumbel_noise     the same g written out for an [M, V] block (tests, statistics of the hash; not on the training path)
//   emoasr_electra_corrupt  generated = ids with the samples at the masked rows, replaced = generated != original, two counters
//   emoasr_bce_head_fwd     z = h . w_p + b_p per row, BCE-with-logits rows, optionally sigmoid(z)
//   emoasr_bce_head_bwd     dz = w (sigmoid(z) - y) g;  dh = dz w_p;  dw_p += sum_m dz h;  db_p += sum_m dz
#include "common.h"
#include "gumbel.h"
#include "../../include/emoasr_hip.h"

namespace {

// One block per row.  Every thread walks its columns once with a running maximum and a running sum of exp(x - maximum) (rescaled
// when the maximum moves: rare, so the precise expf there costs nothing), its best perturbed logit and the label's logit; the block
// then combines.  The perturbed value is the f32 sum to_f32(z) + g, so a caller can restate the argmax exactly.
template <typename T>
__global__ __launch_bounds__(256) void sample_rows_kernel(int V, const T* __restrict__ logits, long ld,
                                                          const int* __restrict__ labels, const float* __restrict__ w,
                                                          uint64_t seed, long row0, float* __restrict__ loss,
                                                          float* __restrict__ lse_out, int* __restrict__ sample) {
  __shared__ float red[16];
  __shared__ float bval[4];
  __shared__ int bcol[4];
  const long m = blockIdx.x;
  const T* row = logits + m * ld;
  const uint64_t base = (uint64_t)(row0 + m) * (uint64_t)V;
  float mx = -INFINITY, se = 0.f, best = -INFINITY;
  int col = 0x7fffffff;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float x = to_f32(row[v]);
    if (x > mx) { se = se * expf(mx - x) + 1.f; mx = x; }
    else se += __expf(x - mx);
    const float p = x + gumbel_of(seed, base + (uint64_t)v);
    if (p > best) { best = p; col = v; }     // (columns ascend within a thread: the first maximum stays)
  }
  const float bm = block_max(mx, red);
  se = block_sum(mx == -INFINITY ? 0.f : se * expf(mx - bm), red);
  const float lse = bm + logf(se);
  // argmax, ties to the lowest column
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(col, o, 64);
    if (ob > best || (ob == best && oc < col)) { best = ob; col = oc; }
  }
  if ((threadIdx.x & 63) == 0) { bval[threadIdx.x >> 6] = best; bcol[threadIdx.x >> 6] = col; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i)
      if (bval[i] > best || (bval[i] == best && bcol[i] < col)) { best = bval[i]; col = bcol[i]; }
    sample[m] = min(max(col, 0), V - 1);
    const float wm = w[m];
    loss[m] = wm == 0.f ? 0.f : -wm * (to_f32(row[labels[m]]) - lse);
    if (lse_out) lse_out[m] = lse;
  }
}

__global__ __launch_bounds__(256) void gumbel_noise_kernel(long M, int V, uint64_t seed, long row0, float* __restrict__ out,
                                                           long ldo) {
  const long n = M * V;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long m = i / V;
    const int v = (int)(i - m * V);
    out[m * ldo + v] = gumbel_of(seed, (uint64_t)(row0 + m) * (uint64_t)V + (uint64_t)v);
  }
}

// generated = ids, replaced = 0, counters = 0
__global__ __launch_bounds__(256) void corrupt_copy_kernel(int BN, const int* __restrict__ ids, int* __restrict__ generated,
                                                           float* __restrict__ replaced, int* __restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < BN) { generated[i] = ids[i]; replaced[i] = 0.f; }
  if (i < 2) counters[i] = 0;
}

// the M masked rows: the sample goes in, replaced <=> it is not the token the mask hid.  One integer atomic per block and counter.
__global__ __launch_bounds__(256) void corrupt_scatter_kernel(int BN, int M, const int* __restrict__ sel,
                                                              const int* __restrict__ labels, const int* __restrict__ samples,
                                                              int* __restrict__ generated, float* __restrict__ replaced,
                                                              int* __restrict__ counters) {
  __shared__ int cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < M) {
    const int p = sel[m];
    if (p >= 0 && p < BN) {
      const int s = samples[m];
      const bool rep = s != labels[m];
      generated[p] = s;
      replaced[p] = rep ? 1.f : 0.f;
      atomicAdd(&cnt[1], 1);
      if (rep) atomicAdd(&cnt[0], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], cnt[threadIdx.x]);
}

__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }

// one wave per row
template <typename T>
__global__ __launch_bounds__(256) void bce_head_fwd_kernel(int M, int H, const T* __restrict__ h, long ldh,
                                                           const T* __restrict__ wp, const float* __restrict__ bp,
                                                           const float* __restrict__ y, const float* __restrict__ w,
                                                           float* __restrict__ z, float* __restrict__ loss,
                                                           float* __restrict__ sig) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const T* row = h + m * ldh;
  float acc = 0.f;
  for (int c = lane; c < H; c += 64) acc += to_f32(row[c]) * to_f32(wp[c]);
  acc = wave_sum(acc);
  if (lane == 0) {
    const float zz = acc + bp[0];
    z[m] = zz;
    if (loss) loss[m] = w[m] * (fmaxf(zz, 0.f) - zz * y[m] + log1pf(expf(-fabsf(zz))));
    if (sig) sig[m] = sigmoid_f(zz);
  }
}

constexpr int kBceRows = 64;   // rows per block of the backward: one f32 atomic per column and block

template <typename T>
__global__ __launch_bounds__(256) void bce_head_bwd_kernel(int M, int H, const T* __restrict__ h, long ldh,
                                                           const T* __restrict__ wp, const float* __restrict__ z,
                                                           const float* __restrict__ y, const float* __restrict__ w,
                                                           float gscale, const float* __restrict__ gscale_dev,
                                                           T* __restrict__ dh, long lddh, float* __restrict__ dwp,
                                                           float* __restrict__ dbp) {
  __shared__ float sdz[kBceRows];
  const long r0 = (long)blockIdx.x * kBceRows;
  const int nrows = (int)min((long)kBceRows, (long)M - r0);
  const float g = gscale_dev ? gscale * gscale_dev[0] : gscale;
  for (int i = threadIdx.x; i < nrows; i += 256) sdz[i] = w[r0 + i] * (sigmoid_f(z[r0 + i]) - y[r0 + i]) * g;
  __syncthreads();
  for (int c = threadIdx.x; c < H; c += 256) {
    const float wc = to_f32(wp[c]);
    float acc = 0.f;
    for (int i = 0; i < nrows; ++i) {
      const float dz = sdz[i];
      acc += dz * to_f32(h[(r0 + i) * ldh + c]);
      dh[(r0 + i) * lddh + c] = from_f32<T>(dz * wc);
    }
    atomicAdd(&dwp[c], acc);
  }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < nrows; ++i) s += sdz[i];
    atomicAdd(dbp, s);
  }
}

inline int ew_grid(long n) { long b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }

}  // namespace

extern "C" int emoasr_sample_rows(int dtype, int M, int V, const void* logits, long ld, const int* labels, const float* w,
                                  uint64_t seed, long row0, float* loss, float* lse, int* sample, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(M > 0 && V >= 2 && ld >= V && row0 >= 0, "sample_rows: M=%d V=%d ld=%ld row0=%ld", M, V, ld, row0);
  EMO_CHECK(logits && labels && w && loss && sample, "sample_rows: null argument");
  EMO_DISPATCH(dtype, (sample_rows_kernel<T><<<M, 256, 0, (hipStream_t)stream>>>(V, (const T*)logits, ld, labels, w, seed, row0,
                                                                                  loss, lse, sample)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_gumbel_noise(int M, int V, uint64_t seed, long row0, float* out, long ldo, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(M > 0 && V >= 1 && ldo >= V && row0 >= 0 && out, "gumbel_noise: M=%d V=%d ldo=%ld row0=%ld", M, V, ldo, row0);
  gumbel_noise_kernel<<<ew_grid((long)M * V), 256, 0, (hipStream_t)stream>>>(M, V, seed, row0, out, ldo);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_electra_corrupt(int BN, int M, const int* ids, const int* sel, const int* labels, const int* samples,
                                      int* generated, float* replaced, int* counters, void* stream) {
  EMO_CHECK(BN >= 1 && M >= 0 && M <= BN, "electra_corrupt: B*N=%d M=%d", BN, M);
  EMO_CHECK(ids && generated && replaced && counters && (M == 0 || (sel && labels && samples)), "electra_corrupt: null argument");
  corrupt_copy_kernel<<<(BN + 255) / 256, 256, 0, (hipStream_t)stream>>>(BN, ids, generated, replaced, counters);
  EMO_LAUNCH_CHECK();
  if (M > 0) {
    corrupt_scatter_kernel<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(BN, M, sel, labels, samples, generated, replaced,
                                                                             counters);
    EMO_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int emoasr_bce_head_fwd(int dtype, int M, int H, const void* h, long ldh, const void* wp, const float* bp,
                                   const float* y, const float* w, float* z, float* loss, float* sig, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(M > 0 && H >= 1 && ldh >= H, "bce_head_fwd: M=%d H=%d ldh=%ld", M, H, ldh);
  EMO_CHECK(h && wp && bp && z && (!loss || (y && w)), "bce_head_fwd: null argument");
  EMO_DISPATCH(dtype, (bce_head_fwd_kernel<T><<<(M + 3) / 4, 256, 0, (hipStream_t)stream>>>(M, H, (const T*)h, ldh, (const T*)wp,
                                                                                            bp, y, w, z, loss, sig)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_bce_head_bwd(int dtype, int M, int H, const void* h, long ldh, const void* wp, const float* z,
                                   const float* y, const float* w, float gscale, const float* gscale_dev, void* dh, long lddh,
                                   float* dwp, float* dbp, void* stream) {
  if (M == 0) return 0;
  EMO_CHECK(M > 0 && H >= 1 && ldh >= H && lddh >= H, "bce_head_bwd: M=%d H=%d ldh=%ld lddh=%ld", M, H, ldh, lddh);
  EMO_CHECK(h && wp && z && y && w && dh && dwp && dbp, "bce_head_bwd: null argument");
  EMO_DISPATCH(dtype, (bce_head_bwd_kernel<T><<<(M + kBceRows - 1) / kBceRows, 256, 0, (hipStream_t)stream>>>(
                          M, H, (const T*)h, ldh, (const T*)wp, z, y, w, gscale, gscale_dev, (T*)dh, lddh, dwp, dbp)));
  EMO_LAUNCH_CHECK();
  return 0;
}
