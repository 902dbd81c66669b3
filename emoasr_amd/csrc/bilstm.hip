// The RNN encoder's bidirectional LSTM layer (encoder_type "rnn") with per-utterance lengths: the semantics of nn.LSTM(bidirectional
// =True, batch_first=True) over pack_padded_sequence(xs, elens, enforce_sorted=False), then pad_packed_sequence, the sum of the two
// directions and dropout (reference asr/modeling/encoders/rnn.py:41-76).
//
// bf16 layers that fit (B <= 256, H <= 512) take ONE cooperative launch for both directions instead (emoasr_bilstm_seq_*,
// csrc/lstm_coop.hip, same frame map and layouts); everything else -- f32 / f32x3, option lstm_coop = 0 -- runs this file's chain.
// The chain (engine._RNNEncMixin): the input projection of both directions is one [B*T, 8H] buffer from two
// GEMMs, and at step s = 0 .. S - 1 (S = max elens) each direction does rec = h_{s-1} . W_hh^T through the product kernels (so f32x3
// gets its split arithmetic) and then ONE cell launch for both directions that
//   - works on frame t = s (forward) or t = elens[b] - 1 - s (reverse) of row b: it gathers pre[b, t] and scatters h, c, the
//     activated gates and the h it started from (hprev, the operand of the W_hh gradient) to (b, t);
//   - treats a row with s >= elens[b] as inactive: it reads nothing of the sequence and writes zeros to frame s of that row
//     (a padded frame, s >= elens[b]), so every frame of every row is written exactly once per direction and the padded ones are
//     exact zeros -- the reverse direction never touches a negative t.
// The backward runs the steps in the opposite order with the same frame map; inactive rows write zero gate gradients, so the
// weight-gradient products run over all B * T rows, and zero their recurrent state, so a reverse row starts from dh = dc = 0.
//
// Layouts (batch-major, dir 0 forward, 1 reverse):
//   pre    [B][T][8H]   x . [W_ih_f; W_ih_r]^T + biases (row stride ldp, gates of dir d at columns 4H d ..)
//   rec    [2][B][4H]   this step's h_{s-1} . W_hh^T per direction, NULL at the first step (zero state)
//   hstate [2][B][H]    h of the previous step (in) / this step (out), compute dtype; cstate f32 [2][B][H] likewise
//   hseq / hprev [2][B][T][H], cseq f32 [2][B][T][H], gact [2][B][T][4H] (activated i | f | g | o)
// hprev[d][b][t] is the h the cell at (b, t) started from: h_{t-1} forward, h_{t+1} reverse (zero at the first frame), so the W_hh
// gradient is ONE product dg^T . hprev per direction with no shifted view that would pair rows across an utterance boundary.
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

inline int bl_grid(long n) { long b = (n + 255) / 256; return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b)); }

template <typename T>
__global__ __launch_bounds__(256) void bilstm_cell_fwd_kernel(int B, int Tn, int H, int s, const int* __restrict__ elens,
                                                              const T* __restrict__ pre, long ldp, const T* __restrict__ rec,
                                                              T* __restrict__ hstate, float* __restrict__ cstate,
                                                              T* __restrict__ hseq, T* __restrict__ hprev,
                                                              float* __restrict__ cseq, T* __restrict__ gact) {
  const long n = 2L * B * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int j = (int)(i % H);
    const long r = i / H;               // dir * B + b
    const int b = (int)(r % B), dir = (int)(r / B);
    const int len = min(elens[b], Tn);   // (the host sizes T as max elens)
    const bool active = s < len;
    const int t = !active ? s : (dir == 0 ? s : len - 1 - s);   // 0 <= t < Tn in both cases (s < Tn, len <= Tn)
    const long fr = (long)dir * B * Tn + (long)b * Tn + t;     // (dir, b, t) row of the sequence buffers
    T* ga = gact + fr * 4 * H + j;
    if (!active) {
      hseq[fr * H + j] = from_f32<T>(0.f);
      hprev[fr * H + j] = from_f32<T>(0.f);
      cseq[fr * H + j] = 0.f;
      ga[0] = ga[H] = ga[2 * H] = ga[3 * H] = from_f32<T>(0.f);
      hstate[i] = from_f32<T>(0.f);
      cstate[i] = 0.f;
      continue;
    }
    const T* p4 = pre + ((long)b * Tn + t) * ldp + (long)dir * 4 * H + j;
    float z[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) z[q] = to_f32(p4[(long)q * H]);
    if (rec) {
      const T* r4 = rec + r * 4 * H + j;
#pragma unroll
      for (int q = 0; q < 4; ++q) z[q] += to_f32(r4[(long)q * H]);
    }
    const float ig = sigmoid_t<T>(z[0]), fg = sigmoid_t<T>(z[1]), gg = tanh_t<T>(z[2]), og = sigmoid_t<T>(z[3]);
    const float cp = s > 0 ? cstate[i] : 0.f;
    const float cn = fg * cp + ig * gg;
    const T hn = from_f32<T>(og * tanh_t<T>(cn));
    hprev[fr * H + j] = s > 0 ? hstate[i] : from_f32<T>(0.f);
    hseq[fr * H + j] = hn;
    cseq[fr * H + j] = cn;
    ga[0] = from_f32<T>(ig); ga[H] = from_f32<T>(fg); ga[2 * H] = from_f32<T>(gg); ga[3 * H] = from_f32<T>(og);
    hstate[i] = hn;
    cstate[i] = cn;
  }
}

// dy [B][T][H]: gradient w.r.t. the layer's summed output (both directions receive it); dh_rec [2][B][H] = dgc_{s+1} . W_hh or NULL
// at the first backward step (then dc starts from zero)
template <typename T>
__global__ __launch_bounds__(256) void bilstm_cell_bwd_kernel(int B, int Tn, int H, int s, const int* __restrict__ elens,
                                                              const T* __restrict__ dy, const T* __restrict__ dh_rec,
                                                              float* __restrict__ dcstate, const T* __restrict__ gact,
                                                              const float* __restrict__ cseq, T* __restrict__ dg,
                                                              T* __restrict__ dgc) {
  const long n = 2L * B * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int j = (int)(i % H);
    const long r = i / H;
    const int b = (int)(r % B), dir = (int)(r / B);
    const int len = min(elens[b], Tn);   // (the host sizes T as max elens)
    const bool active = s < len;
    const int t = !active ? s : (dir == 0 ? s : len - 1 - s);
    const long fr = (long)dir * B * Tn + (long)b * Tn + t;
    T* d4 = dg + fr * 4 * H + j;
    T* c4 = dgc + r * 4 * H + j;
    if (!active) {
      d4[0] = d4[H] = d4[2 * H] = d4[3 * H] = from_f32<T>(0.f);
      c4[0] = c4[H] = c4[2 * H] = c4[3 * H] = from_f32<T>(0.f);
      dcstate[i] = 0.f;
      continue;
    }
    const T* a4 = gact + fr * 4 * H + j;
    const float ig = to_f32(a4[0]), fg = to_f32(a4[H]), gg = to_f32(a4[2 * H]), og = to_f32(a4[3 * H]);
    float dh = to_f32(dy[((long)b * Tn + t) * H + j]);
    if (dh_rec) dh += to_f32(dh_rec[i]);
    const float cu = cseq[fr * H + j];
    // the cell state this one started from: the previous frame of the direction, zero at its first frame
    const bool first = dir == 0 ? t == 0 : t == len - 1;
    const float cp = first ? 0.f : cseq[(fr + (dir == 0 ? -1 : 1)) * H + j];
    const float tc = tanh_t<T>(cu);
    const float dct = (dh_rec ? dcstate[i] : 0.f) + dh * og * (1.f - tc * tc);
    const T g0 = from_f32<T>(dct * gg * ig * (1.f - ig)), g1 = from_f32<T>(dct * cp * fg * (1.f - fg));
    const T g2 = from_f32<T>(dct * ig * (1.f - gg * gg)), g3 = from_f32<T>(dh * tc * og * (1.f - og));
    d4[0] = g0; d4[H] = g1; d4[2 * H] = g2; d4[3 * H] = g3;
    c4[0] = g0; c4[H] = g1; c4[2 * H] = g2; c4[3 * H] = g3;
    dcstate[i] = dct * fg;
  }
}

// y[b, t, :] = dropout(a + b) for t < elens[b], 0 otherwise (b may be NULL); the keep mask is scale_dropout's of the flat index
template <typename T>
__global__ __launch_bounds__(256) void bilstm_out_kernel(int B, int Tn, int H, const int* __restrict__ elens, const T* __restrict__ x0,
                                                         const T* __restrict__ x1, T* __restrict__ y, float p, uint64_t seed) {
  const long n = (long)B * Tn * H;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / H;
    const int t = (int)(r % Tn), b = (int)(r / Tn);
    float v = 0.f;
    if (t < elens[b]) {
      v = to_f32(x0[i]);
      if (x1) v += to_f32(x1[i]);
      v *= dropout_scale(seed, (uint64_t)i, p);
    }
    y[i] = from_f32<T>(v);
  }
}

}  // namespace

extern "C" int emoasr_bilstm_cell_fwd(int dtype, int B, int T_, int H, int s, const int* elens, const void* pre, long ldp,
                                      const void* rec, void* hstate, float* cstate, void* hseq, void* hprev, float* cseq,
                                      void* gact, void* stream) {
  EMO_CHECK(B >= 0 && T_ >= 1 && H >= 1 && s >= 0 && s < T_ && ldp >= 8L * H, "bilstm_cell_fwd: bad shape (B %d, T %d, H %d, s %d)",
            B, T_, H, s);
  if (B == 0) return 0;
  EMO_DISPATCH(dtype, (bilstm_cell_fwd_kernel<T><<<bl_grid(2L * B * H), 256, 0, (hipStream_t)stream>>>(
                          B, T_, H, s, elens, (const T*)pre, ldp, (const T*)rec, (T*)hstate, cstate, (T*)hseq, (T*)hprev, cseq,
                          (T*)gact)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_bilstm_cell_bwd(int dtype, int B, int T_, int H, int s, const int* elens, const void* dy, const void* dh_rec,
                                      float* dcstate, const void* gact, const float* cseq, void* dg, void* dgc, void* stream) {
  EMO_CHECK(B >= 0 && T_ >= 1 && H >= 1 && s >= 0 && s < T_, "bilstm_cell_bwd: bad shape (B %d, T %d, H %d, s %d)", B, T_, H, s);
  if (B == 0) return 0;
  EMO_DISPATCH(dtype, (bilstm_cell_bwd_kernel<T><<<bl_grid(2L * B * H), 256, 0, (hipStream_t)stream>>>(
                          B, T_, H, s, elens, (const T*)dy, (const T*)dh_rec, dcstate, (const T*)gact, cseq, (T*)dg, (T*)dgc)));
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_bilstm_out(int dtype, int B, int T_, int H, const int* elens, const void* x0, const void* x1, void* y,
                                 float drop_p, uint64_t seed, void* stream) {
  const long n = (long)B * T_ * H;
  if (n == 0) return 0;
  EMO_DISPATCH(dtype, (bilstm_out_kernel<T><<<bl_grid(n), 256, 0, (hipStream_t)stream>>>(B, T_, H, elens, (const T*)x0, (const T*)x1,
                                                                                       (T*)y, drop_p, seed)));
  EMO_LAUNCH_CHECK();
  return 0;
}
