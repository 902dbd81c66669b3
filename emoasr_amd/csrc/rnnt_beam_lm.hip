// RNN-LM shallow fusion inside the batched transducer beam search (engine.rnnt_beam_search_batch with lm=): the LM's LSTM state of a
// hypothesis lives in pools beside the prediction network's, under the SAME slot numbers, and is stepped by the SAME control words
// through emoasr_rnnt_beam_lstm_rows (csrc/rnnt_beam.hip).  What fusion adds per round is here:
//
//   emoasr_rnnt_beam_gather_rows   the LM's top-layer h of every row as an [R, H] matrix for the head product: out[r] = pool[dst[r]],
//                                  a zero row for an inactive row or a slot outside the pool (the control words of an inactive row
//                                  may hold anything)
//   emoasr_rnnt_beam_pick_lm       the fused twin of emoasr_rnnt_beam_pick: lp = log_softmax(ASR row) over V, lq = log_softmax(LM row)
//                                  over all V_lm >= V columns, f[v] = lp[v] + mu * lq[v] for v in 1 .. V - 1 (product and sum rounded
//                                  separately: the library is compiled without contraction), record { lp[blank], the k best f
//                                  (descending, ties -> lowest index), their indices relative to column 1 as floats } -- the layout
//                                  emoasr_rnnt_beam_book reads.  mu is per SEARCH (row r -> mu[r / W]); an inactive row writes nothing.
//
// One wave per row, no workgroup barrier.  The ASR row is handled exactly as in emoasr_rnnt_beam_pick (the same two forms, the same
// order of every sum), so that mu = 0 gives its record bit for bit: 0 * lq is +-0 for a finite lq and lp + (+-0) = lp.  The LM row is
// STREAMED: one pass for the maximum, one for the sum of exponentials (the ASR row's algorithm, lane l takes columns l, l + 64, ...),
// then the columns below V once more for lq; the second and third pass hit the cache (a row is <= 60 KiB).
#include <math.h>
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

// log-sum-exp of row[0 .. n) over the wave (every lane gets it)
template <typename T>
__device__ __forceinline__ float wave_row_lse(const T* __restrict__ row, int n, int lane) {
  float mx = -INFINITY;
  for (int v = lane; v < n; v += 64) mx = fmaxf(mx, to_f32(row[v]));
  mx = wave_max(mx);
  float se = 0.f;
  for (int v = lane; v < n; v += 64) se += expf(to_f32(row[v]) - mx);
  se = wave_sum(se);
  return mx + logf(se);
}

struct PickLmArgs {
  int V, V_lm, k, blank, W;
  const void* logits; long ldl;
  const void* lm_logits; long ldlm;
  const float* mu;                // [searches]
  const long long* active;        // [R] or null (every row active)
  float* out; long ldo;
};

// V > 1024: the ASR row in LDS (V floats), as rnnt_beam_pick_kernel
template <typename T>
__global__ __launch_bounds__(64) void rnnt_beam_pick_lm_kernel(const PickLmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* buf = reinterpret_cast<float*>(smem);   // [V]
  const long m = blockIdx.x;
  if (a.active && a.active[m] == 0) return;      // (uniform over the wave)
  const int lane = threadIdx.x, V = a.V, k = a.k;
  const T* row = static_cast<const T*>(a.logits) + m * a.ldl;
  const T* lrow = static_cast<const T*>(a.lm_logits) + m * a.ldlm;
  float* out = a.out + m * a.ldo;
  const float mu = a.mu[m / a.W];
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) { const float x = to_f32(row[v]); buf[v] = x; mx = fmaxf(mx, x); }
  mx = wave_max(mx);
  float se = 0.f;
  for (int v = lane; v < V; v += 64) se += expf(buf[v] - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se);
  for (int v = lane; v < V; v += 64) buf[v] -= lse;
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) out[0] = buf[a.blank];
  __builtin_amdgcn_wave_barrier();
  const float lse_lm = wave_row_lse(lrow, a.V_lm, lane);
  for (int v = lane; v < V; v += 64) {
    const float lq = to_f32(lrow[v]) - lse_lm;
    const float p = mu * lq;
    buf[v] = v >= 1 ? buf[v] + p : -INFINITY;    // the candidates are columns 1 .. V - 1
  }
  __builtin_amdgcn_wave_barrier();
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float c = buf[v];
      if (v >= 1 && (c > best || (c == best && v < bi))) { best = c; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi == 0x7fffffff) bi = 1;
    if (lane == 0) {
      out[1 + j] = best;
      out[1 + k + j] = (float)(bi - 1);
      buf[bi] = -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// V <= 1024: the ASR row and the fused values in REGISTERS (16 per lane, lane l holds columns l, l + 64, ...), as
// rnnt_beam_pick16_kernel (17.7 -> ~3 us at V = 1000: no dependent LDS round trips)
template <typename T>
__global__ __launch_bounds__(64) void rnnt_beam_pick16_lm_kernel(const PickLmArgs a) {
  const long m = blockIdx.x;
  if (a.active && a.active[m] == 0) return;      // (uniform over the wave)
  const int lane = threadIdx.x, V = a.V, k = a.k;
  const T* row = static_cast<const T*>(a.logits) + m * a.ldl;
  const T* lrow = static_cast<const T*>(a.lm_logits) + m * a.ldlm;
  float* out = a.out + m * a.ldo;
  const float mu = a.mu[m / a.W];
  float x[16];
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int v = e * 64 + lane;
    x[e] = v < V ? to_f32(row[v]) : -INFINITY;
    mx = fmaxf(mx, x[e]);
  }
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) se += (e * 64 + lane < V) ? expf(x[e] - mx) : 0.f;
  se = wave_sum(se);
  const float lse = mx + logf(se);
  const float lse_lm = wave_row_lse(lrow, a.V_lm, lane);
  float lpb = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int v = e * 64 + lane;
    x[e] -= lse;
    if (v == a.blank) lpb = x[e];
    if (v >= 1 && v < V) {
      const float lq = to_f32(lrow[v]) - lse_lm;
      const float p = mu * lq;
      x[e] = x[e] + p;
    } else {
      x[e] = -INFINITY;                          // column 0 and the columns past V are no candidates
    }
  }
  lpb = wave_max(lpb);
  if (lane == 0) out[0] = lpb;
  for (int j = 0; j < k; ++j) {
    float best = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < 16; ++e) {   // ascending columns: a strict > keeps the lowest index among equals
      if (x[e] > best) { best = x[e]; bi = e * 64 + lane; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi == 0x7fffffff) bi = 1;
    if (lane == 0) {
      out[1 + j] = best;
      out[1 + k + j] = (float)(bi - 1);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e * 64 + lane == bi) x[e] = -INFINITY;
  }
}

// out[r] = pool[dst[r]] (H values of T), a zero row for an inactive row or a slot outside the pool; one workgroup per row
template <typename T>
__global__ __launch_bounds__(256) void rnnt_beam_gather_rows_kernel(int H, const T* __restrict__ pool, long nslots,
                                                                    const long long* __restrict__ dst,
                                                                    const long long* __restrict__ active, T* __restrict__ out) {
  const long r = blockIdx.x;
  const long long d = dst[r];
  const bool on = (!active || active[r] != 0) && d >= 0 && d < nslots;
  const T* src = pool + (on ? d : 0) * (long)H;
  for (int c = threadIdx.x; c < H; c += 256) out[r * H + c] = on ? src[c] : from_f32<T>(0.f);
}

}  // namespace

extern "C" int emoasr_rnnt_beam_pick_lm(int dtype, int R, int V, int V_lm, int k, int blank, int W, const void* logits, long ldl,
                                        const void* lm_logits, long ldlm, const float* mu, const long long* active, float* out,
                                        long ldo, void* stream) {
  EMO_CHECK(R >= 1 && k >= 1 && k < V && blank >= 0 && blank < V && ldo >= 1 + 2 * k, "rnnt_beam_pick_lm: bad arguments");
  EMO_CHECK(V_lm >= V, "rnnt_beam_pick_lm: the LM's vocabulary (%d) is smaller than the model's (%d)", V_lm, V);
  EMO_CHECK(W >= 1 && logits && lm_logits && mu && out && ldl >= V && ldlm >= V_lm, "rnnt_beam_pick_lm: bad arguments");
  EMO_CHECK((size_t)V * 4 <= 60 * 1024, "rnnt_beam_pick_lm: V=%d too large for an LDS row", V);
  PickLmArgs a{V, V_lm, k, blank, W, logits, ldl, lm_logits, ldlm, mu, active, out, ldo};
  if (V <= 1024) {
    EMO_DISPATCH(dtype, (rnnt_beam_pick16_lm_kernel<T><<<R, 64, 0, (hipStream_t)stream>>>(a)));
    EMO_LAUNCH_CHECK();
    return 0;
  }
  EMO_DISPATCH(dtype, (rnnt_beam_pick_lm_kernel<T><<<R, 64, (size_t)V * 4, (hipStream_t)stream>>>(a)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_rnnt_beam_gather_rows(int dtype, int R, int H, const void* pool, long nslots, const long long* dst,
                                            const long long* active, void* out, void* stream) {
  EMO_CHECK(R >= 1 && H >= 1 && nslots >= 1 && pool && dst && out, "rnnt_beam_gather_rows: R=%d H=%d nslots=%ld", R, H, nslots);
  EMO_DISPATCH(dtype, (rnnt_beam_gather_rows_kernel<T><<<R, 256, 0, (hipStream_t)stream>>>(H, (const T*)pool, nslots, dst, active,
                                                                                          (T*)out)));
  EMO_LAUNCH_CHECK();
  return 0;
}
