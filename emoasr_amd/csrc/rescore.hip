// N-best rescoring and error-label alignment (asr/rescore/test_rescore_grid.py, asr/rescore/align_hyps.py): the Levenshtein
// alignment of asr/metrics.py:20-105 per (hypothesis, reference) pair, and the grid of (lm_weight, len_weight) over its counts.
//
//   emoasr_edit_align    per pair: (n_sub, n_ins, n_del, dist), the op list and the error-label row of align_hyps.  One wave per
//                        pair.  The matrix is filled in strips of 64 columns, lane l owning column 64 s + l + 1 and running l rows
//                        behind lane l - 1, so that a cell's left and diagonal neighbours arrive by one shuffle and its upper
//                        neighbour is the lane's own last value: the distances live in registers, only the last column of a strip
//                        goes through LDS to the next one.  The reference's backtrace preference (C, then I, then S, then D) is a
//                        function of the three neighbours and the match bit, so each cell leaves a 2-bit direction code -- two
//                        ballots per step, 16 bytes -- and the matrix itself is never stored.  The codes of a pair live in LDS when
//                        they fit EDIT_LDS_WORDS, else in the caller's workspace.  The backtrace (lane 0) reads codes alone and
//                        writes the ops into LDS, from where the wave copies them out and folds them into labels.
//   emoasr_rescore_grid  one thread per (grid cell, utterance): the first row with the largest
//                        (score_asr + lm_w * score_lm) + len_w * ylen, each product and sum rounded once to f64 (no fused
//                        multiply-add: the bits pandas computes), and the winners' S / I / D summed per cell with integer atomics.
#include "common.h"
#include "../../include/emoasr_hip.h"

namespace {

constexpr int EDIT_MAX_LEN = EMOASR_EDIT_MAX_LEN;
constexpr int EDIT_LDS_WORDS = EMOASR_EDIT_LDS_WORDS;   // 64-bit words of direction codes kept in LDS (32 KB)
enum { OP_C = 0, OP_I = 1, OP_S = 2, OP_D = 3 };

__device__ __forceinline__ char op_char(int c) { return c == OP_C ? 'C' : (c == OP_I ? 'I' : (c == OP_S ? 'S' : 'D')); }

// words of direction codes of an R x H pair: two per step, R + 63 steps per strip of 64 columns
__host__ __device__ inline long edit_code_words(int R, int H) { return 2l * ((H + 63) / 64) * (R + 63); }

__global__ __launch_bounds__(64) void edit_align_kernel(int P, int n_ref, const int* __restrict__ hyp,
                                                        const int* __restrict__ hyp_off, const int* __restrict__ ref,
                                                        const int* __restrict__ ref_off, const int* __restrict__ ref_idx,
                                                        int label_mode, int* __restrict__ counts, unsigned char* __restrict__ ops,
                                                        const long* __restrict__ ops_off, unsigned char* __restrict__ labels,
                                                        unsigned long long* __restrict__ ws, const long* __restrict__ ws_off,
                                                        int* __restrict__ status) {
  __shared__ unsigned long long lds_codes[EDIT_LDS_WORDS];
  __shared__ unsigned short bnd[EDIT_MAX_LEN + 1];        // d[i][64 s]: the column a strip hands to the next one
  __shared__ unsigned char opbuf[2 * EDIT_MAX_LEN];       // the ops, written from the end by the backtrace; then the labels
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= P) return;
  const int r = ref_idx ? ref_idx[p] : p;
  const int h0 = hyp_off[p], Hreal = hyp_off[p + 1] - h0;
  bool bad = r < 0 || r >= n_ref || Hreal < 0 || Hreal > EDIT_MAX_LEN;
  int r0 = 0, R = 0;
  if (!bad) {
    r0 = ref_off[r];
    R = ref_off[r + 1] - r0;
    bad = R < 0 || R > EDIT_MAX_LEN;
  }
  const int H = Hreal > 0 ? Hreal : 1;     // an empty hypothesis is one token that matches nothing
  unsigned long long* codes = lds_codes;
  if (!bad && edit_code_words(R, H) > EDIT_LDS_WORDS) {
    bad = !ws || !ws_off || ws_off[p + 1] - ws_off[p] < edit_code_words(R, H);
    if (!bad) codes = ws + ws_off[p];
  }
  if (bad) {                                // (uniform over the wave)
    if (lane == 0) {
      atomicOr(status, 1);
      for (int k = 0; k < 4; ++k) counts[4 * p + k] = -1;
    }
    return;
  }
  const int steps = R + 63, strips = (H + 63) >> 6;
  int dist = H;                             // d[R][H]; R == 0 leaves the first row's value
  for (int s = 0; s < strips; ++s) {
    const int j = s * 64 + lane + 1;        // this lane's column
    const bool col = j <= H;
    const int htok = (col && Hreal > 0) ? hyp[h0 + j - 1] : 0;
    const bool hreal = col && Hreal > 0;
    int up = j, diag = j - 1, cur = j;      // d[0][j], d[0][j-1]; cur: the lane's last value, d[i][j] after row i
    int rtok = 0, rchunk = 0, bchunk = 0;
    unsigned long long* cw = codes + 2l * s * steps;
    for (int t = 0; t < steps; ++t) {
      if ((t & 63) == 0) {                  // rows t + 1 .. t + 64 enter at lane 0 during the next 64 steps
        const int i = t + lane + 1;
        rchunk = i <= R ? ref[r0 + i - 1] : 0;
        bchunk = i <= R ? (s == 0 ? i : (int)bnd[i]) : 0;
      }
      int left = __shfl_up(cur, 1, 64);
      rtok = __shfl_up(rtok, 1, 64);
      const int rt0 = __shfl(rchunk, t & 63, 64), b0 = __shfl(bchunk, t & 63, 64);
      if (lane == 0) { left = b0; rtok = rt0; }
      const int i = t - lane + 1;
      const bool live = col && i >= 1 && i <= R;
      int code = 0;
      if (live) {
        int d;
        if (hreal && rtok == htok) { d = diag; code = OP_C; }
        else {
          const int m = min(diag, min(left, up));
          d = m + 1;
          code = left == m ? OP_I : (diag == m ? OP_S : OP_D);
        }
        diag = left;
        up = cur = d;
        if (lane == 63) bnd[i] = (unsigned short)d;
      }
      const unsigned long long b_lo = __ballot(code & 1), b_hi = __ballot(code & 2);
      if (lane == 0) { cw[2 * t] = b_lo; cw[2 * t + 1] = b_hi; }
    }
    if (s == strips - 1 && R > 0) dist = __shfl(cur, (H - 1) & 63, 64);
    __syncthreads();
  }

  // the backtrace from (R, H), ops written from the end of opbuf
  const int cap = R + H;
  int n_sub = 0, n_ins = 0, n_del = 0, start = cap;
  if (lane == 0) {
    int x = R, y = H;
    while (x | y) {
      int c;
      if (x == 0) c = OP_I;
      else if (y == 0) c = OP_D;
      else {
        const int l = (y - 1) & 63;
        const unsigned long long* w = codes + 2l * ((y - 1) >> 6) * steps + 2 * (x - 1 + l);
        c = (int)((w[0] >> l) & 1) | ((int)((w[1] >> l) & 1) << 1);
      }
      opbuf[--start] = (unsigned char)c;
      if (c == OP_C || c == OP_S) { --x; --y; n_sub += c == OP_S; }
      else if (c == OP_I) { --y; ++n_ins; }
      else { --x; ++n_del; }
    }
    counts[4 * p + 0] = n_sub;
    counts[4 * p + 1] = n_ins;
    counts[4 * p + 2] = n_del;
    counts[4 * p + 3] = dist;
  }
  start = __shfl(start, 0, 64);
  __syncthreads();
  if (ops) {
    unsigned char* o = ops + ops_off[p];
    for (int k = lane; k < cap - start; k += 64) o[k] = op_char(opbuf[start + k]);
  }
  if (!labels || label_mode == EMOASR_ALIGN_NONE || Hreal == 0) return;
  __syncthreads();
  // align_hyps.py:37-55, one label per hypothesis token, written over the ops already read (label k never lies past op k).
  // SI drops the deletions.  SID: a deletion with no label before it, or after a label that is not C, turns the next C into D;
  // after a C it is dropped (the reference's "pass D to the left" compares where it means to assign).
  if (lane == 0) {
    int n = 0, last = -1;
    bool del_flag = false;
    for (int k = start; k < cap; ++k) {
      const int c = opbuf[k];
      if (c == OP_D) {
        if (label_mode == EMOASR_ALIGN_SID && last != OP_C) del_flag = true;
      } else {
        last = (del_flag && c == OP_C) ? OP_D : c;
        del_flag = false;
        opbuf[n++] = (unsigned char)last;
      }
    }
  }
  __syncthreads();
  for (int k = lane; k < Hreal; k += 64) labels[h0 + k] = op_char(opbuf[k]);
}

__global__ __launch_bounds__(256) void rescore_grid_kernel(int U, int G2, const double* __restrict__ score_asr,
                                                           const double* __restrict__ score_lm, const int* __restrict__ ylen,
                                                           const int* __restrict__ utt_off, const int* __restrict__ counts,
                                                           const double* __restrict__ lm_w, const double* __restrict__ len_w,
                                                           int* __restrict__ best, long long* __restrict__ totals) {
  const int g = blockIdx.y, u = blockIdx.x * 256 + threadIdx.x;
  const double wl = lm_w[g / G2], wn = len_w[g % G2];
  int s = 0, i = 0, d = 0;
  if (u < U) {
    const int a = utt_off[u], b = utt_off[u + 1];
    int arg = -1;
    double top = 0.0;
    for (int k = a; k < b; ++k) {
      const double sc = __dadd_rn(__dadd_rn(score_asr[k], __dmul_rn(wl, score_lm[k])), __dmul_rn(wn, (double)ylen[k]));
      if (arg < 0 || sc > top) { top = sc; arg = k; }      // (strictly larger: the first row keeps a tie)
    }
    best[(long)g * U + u] = arg;
    if (arg >= 0) { s = counts[4 * arg]; i = counts[4 * arg + 1]; d = counts[4 * arg + 2]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    i += __shfl_xor(i, o, 64);
    d += __shfl_xor(d, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && (s | i | d)) {
    unsigned long long* t = (unsigned long long*)totals + 3l * g;
    atomicAdd(t + 0, (unsigned long long)s);
    atomicAdd(t + 1, (unsigned long long)i);
    atomicAdd(t + 2, (unsigned long long)d);
  }
}

}  // namespace

extern "C" long emoasr_edit_align_lds_words(void) { return EDIT_LDS_WORDS; }

extern "C" long emoasr_edit_align_ws_words(int ref_len, int hyp_len) {
  if (ref_len < 0 || hyp_len < 0 || ref_len > EDIT_MAX_LEN || hyp_len > EDIT_MAX_LEN) return -1;
  const long w = edit_code_words(ref_len, hyp_len > 0 ? hyp_len : 1);
  return w > EDIT_LDS_WORDS ? w : 0;
}

extern "C" int emoasr_edit_align(int P, int n_ref, int max_hyp_len, int max_ref_len, const int* hyp, const int* hyp_off,
                                 const int* ref, const int* ref_off, const int* ref_idx, int label_mode, int* counts,
                                 unsigned char* ops, const long* ops_off, unsigned char* labels, void* ws, const long* ws_off,
                                 int* status, void* stream) {
  if (P == 0) return 0;
  EMO_CHECK(P > 0 && n_ref > 0 && (ref_idx || n_ref >= P), "edit_align: P=%d n_ref=%d", P, n_ref);
  EMO_CHECK(max_hyp_len >= 0 && max_ref_len >= 0 && max_hyp_len <= EDIT_MAX_LEN && max_ref_len <= EDIT_MAX_LEN,
            "edit_align: a pair of %d x %d tokens is over the limit of %d per side", max_ref_len, max_hyp_len, EDIT_MAX_LEN);
  EMO_CHECK(label_mode == EMOASR_ALIGN_NONE || label_mode == EMOASR_ALIGN_SI || label_mode == EMOASR_ALIGN_SID,
            "edit_align: label mode %d", label_mode);
  EMO_CHECK(hyp_off && ref && ref_off && counts && status && (hyp || max_hyp_len == 0), "edit_align: null argument");
  EMO_CHECK(!ops || ops_off, "edit_align: ops without ops_off");
  EMO_CHECK(label_mode == EMOASR_ALIGN_NONE || labels, "edit_align: label mode %d without a label array", label_mode);
  EMO_CHECK((ws && ws_off) || edit_code_words(max_ref_len, max_hyp_len > 0 ? max_hyp_len : 1) <= EDIT_LDS_WORDS,
            "edit_align: a pair of %d x %d tokens needs a workspace", max_ref_len, max_hyp_len);
  edit_align_kernel<<<P, 64, 0, (hipStream_t)stream>>>(P, n_ref, hyp, hyp_off, ref, ref_off, ref_idx, label_mode, counts, ops,
                                                       ops_off, labels, (unsigned long long*)ws, ws_off, status);
  EMO_LAUNCH_CHECK();
  return 0;
}

extern "C" int emoasr_rescore_grid(int N, int U, int G1, int G2, const double* score_asr, const double* score_lm,
                                   const int* ylen, const int* utt_off, const int* counts, const double* lm_w,
                                   const double* len_w, int* best, long long* totals, void* stream) {
  EMO_CHECK(N >= 0 && U >= 1 && G1 >= 1 && G2 >= 1 && (long)G1 * G2 <= 65535, "rescore_grid: N=%d U=%d grid %d x %d", N, U, G1,
            G2);
  EMO_CHECK(utt_off && lm_w && len_w && best && totals && (N == 0 || (score_asr && score_lm && ylen && counts)),
            "rescore_grid: null argument");
  if (hipMemsetAsync(totals, 0, sizeof(long long) * 3 * G1 * G2, (hipStream_t)stream) != hipSuccess) {
    emo_set_error("rescore_grid: clearing the totals failed");
    return 2;
  }
  rescore_grid_kernel<<<dim3(cdiv(U, 256), G1 * G2), 256, 0, (hipStream_t)stream>>>(U, G2, score_asr, score_lm, ylen, utt_off,
                                                                                    counts, lm_w, len_w, best, totals);
  EMO_LAUNCH_CHECK();
  return 0;
}
