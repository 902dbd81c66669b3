/* emoasr_hip.h -- C ABI of libemoasr_hip.so, the MI355X (gfx950) device library
 * behind the emoASR-compatible Python modules in emoasr_amd/.
 *
 * The reference (emonosuke/emoASR) is pure Python on PyTorch: its "FFI" for the
 * hot path is the set of ATen / cuDNN calls made by asr/modeling/**.  Every
 * entry point below replaces one such call site (cited per function) with a
 * hand-written HIP kernel.  Signatures use plain device pointers, sizes and a
 * hipStream_t passed as void*: no torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error;
 *     emoasr_last_error() returns a message for the calling thread's last error.
 *   - dtype: EMOASR_F32 (exact mode: f32 MFMA, a bit-exact k-ordered fmaf chain), EMOASR_BF16 (bf16 MFMA,
 *     f32 accumulate) or EMOASR_F32X3 (the PARITY mode at throughput: f32 buffers, statistics and epilogues
 *     exactly as EMOASR_F32, every matrix product as three bf16 MFMAs over (hi, lo) operand pairs -- 16
 *     significand bits per operand; meets north_star's 1e-3 / bit-exact-ids tolerances, tests/test_fullsize_gpu.py).
 *     The mode is an argument of every call: the library keeps no precision state (rounds 4-5 had a
 *     process-wide option "f32_split"; it is gone).  Entry points without a matrix product treat EMOASR_F32X3
 *     as EMOASR_F32.  "T*" below means a buffer of the dtype's element type (float for both f32 codes).
 *   - statistics, losses, lattices, parameter gradients and optimizer state are
 *     always f32; lengths / labels are int32.
 *   - all pointers are device pointers unless noted; kernels are enqueued on
 *     `stream` and never synchronise the host.
 *   - activations are row-major [rows, features] ("channels-last").
 */
#ifndef EMOASR_HIP_H
#define EMOASR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { EMOASR_F32 = 0, EMOASR_BF16 = 1, EMOASR_F32X3 = 2 };
enum { EMOASR_ACT_NONE = 0, EMOASR_ACT_RELU = 1, EMOASR_ACT_SWISH = 2,
       /* emoasr_epilogue_t.dact only: the tensor behind dact_pre IS the factor to multiply by (saved by a forward epilogue whose
        * act carried EMOASR_ACT_SAVE_DACT); pass drop_p = 0 with it, the mask is part of the factor */
       EMOASR_DACT_MUL = 6 };
/* emoasr_epilogue_t.act | EMOASR_ACT_SAVE_DACT: pre_out receives act'(pre) * dropout_scale (the factor of the data gradient)
 * instead of the pre-activation: the backward of x -> dropout(act(x W^T + b)) then needs neither the activation's derivative nor
 * a second hashing of the dropout mask (transformer.py:117-118's feed-forward blocks in training). */
#define EMOASR_ACT_SAVE_DACT 0x100

const char* emoasr_last_error(void);
int emoasr_version(void);
/* Run-time options: named process-wide ints that select kernel paths and tuning values (csrc/common.h, EMO_OPTIONS, lists every
 * one with its default, its normalisation and a line of description; every default is what the training step or the decode leg
 * measured fastest).  emoasr_set_option stores the NORMALISED value (an out-of-range value becomes the option's fallback: e.g.
 * "attn_fwd_waves" 3 -> 0, "big_waves" 5 -> 8, "conv_strip" -1 -> 0 and above 65536 -> 65536); emoasr_get_option returns the stored
 * value and the default (either pointer may be null); emoasr_option_count / emoasr_option_name enumerate the names (null when the
 * index is out of range).  An unknown name is an error (emoasr_last_error: "unknown option '<name>'").
 * Options are read at launch time without synchronisation: set them while no call of the library is in flight on any thread.
 * "timers": see emoasr_timer_read. */
int emoasr_set_option(const char* name, int value);
int emoasr_get_option(const char* name, int* value, int* default_value);
int emoasr_option_count(void);
const char* emoasr_option_name(int index);
/* Device time of selected kernels that sit behind composite entry points, measured with HIP events on the launch stream
 * while emoasr_set_option("timers", 1) is in effect.  name: "attn_bwd_fused_kernel", "attn_bwd_dpos_kernel",
 * "attn_fwd_kernel", "gemm_tn_grouped_kernel".  -> number of launches recorded and their summed milliseconds
 * (synchronises on the recorded events); reset != 0 clears the record.  bench.py's roofline object reads this. */
int emoasr_timer_read(const char* name, int* calls, double* ms, int reset);
/* The same with the ALGORITHMIC work of the recorded launches (sum of 2 M N K flops / operand + result bytes as the entry point
 * was called; 0 where the library cannot know it).  Families: "gemm_nt_nn" (emoasr_gemm_nt + emoasr_gemm_nn, forward and
 * data-gradient products), "gemm_tn" (emoasr_gemm_tn + _grouped, weight gradients), "layernorm" (forward + backward),
 * "conv_module" (emoasr_conv_module_fwd_seg / _bwd_seg), and the kernels named above.  "timers" = 1 records every family, a
 * bit mask 1 << (index + 1) only the chosen ones (index = position in this list: attn_bwd_fused_kernel 0, attn_bwd_dpos3_kernel
 * 1, attn_fwd_kernel 2, gemm_tn_grouped_kernel 3, gemm_nt_nn 4, gemm_tn 5, layernorm 6, conv_module 7).  Option
 * "timer_stride" = n records every n-th launch of a family only (an event pair per launch costs device time). */
int emoasr_timer_read_ex(const char* name, int* calls, double* ms, double* flops, double* bytes, int reset);

/* GEMM epilogue, applied in this order to v = alpha*acc + bias[col]:
 *   pre_out[row,col] = v            (if pre_out)
 *   v = act(v)
 *   v *= dact'(dact_pre[row,col])   (if dact_pre; derivative of activation `dact`)
 *   v *= dropout(seed, row*N+col)   (if drop_p > 0; 0 or 1/(1-p))
 *   v = residual[row,col] + res_scale*v   (if residual)
 * pre_out / dact_pre share C's leading dimension; residual uses ldr. */
typedef struct {
  const float* bias;
  const void* residual;
  void* pre_out;
  const void* dact_pre;
  float alpha;
  float res_scale;
  int act;
  int dact;
  int ldr;
  int out_f32; /* C is float* regardless of dtype */
  float drop_p;
  uint64_t seed;
} emoasr_epilogue_t;

/* C[M,N] = epilogue(A[M,K] . B[N,K]^T).  Replaces nn.Linear / Conv1d(k=1):
 * asr/modeling/transformer.py:62-71,94,110-118; conformer.py:62,103-105,115-117;
 * encoders/conv.py:16-19; decoders/ctc.py:34,103. */
int emoasr_gemm_nt(int dtype, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                   void* C, long ldc, const emoasr_epilogue_t* ep, void* stream);
/* C[M,N] = epilogue(A[M,K] . B[K,N]) with B stored k-major (row stride ldb): the data
 * gradient dX = dY . W of the calls above, straight from the [out,in] weight. */
int emoasr_gemm_nn(int dtype, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                   void* C, long ldc, const emoasr_epilogue_t* ep, void* stream);
/* batched form: C[b,h] = alpha * A[b,h] . B[b,h]; s*_b / s*_h are the outer / inner batch strides
 * (elements).  Attention backward: dV[b,h] = Pd[b,h] . dO[b,h], dK[b,h] = dS[b,h] . Q[b,h]. */
int emoasr_gemm_nn_batched(int dtype, int M, int N, int K, const void* A, long lda, long sa_b, long sa_h,
                           const void* B, long ldb, long sb_b, long sb_h, void* C, long ldc, long sc_b,
                           long sc_h, int nb, int nh, float alpha, int accumulate, void* stream);
/* C[N1,N2] (+)= alpha * A[K,N1]^T . B[K,N2], f32 output (weight gradients; the
 * autograd backward of the calls above).  If colsum != NULL the kernel also produces
 * colsum[N1] (+)= colsum_scale * sum_k A[k,:] (the bias gradient) from the staged A tiles. */
int emoasr_gemm_tn(int dtype, int N1, int N2, int K, const void* A, long lda, const void* B, long ldb,
                   float* C, long ldc, float alpha, int accumulate, float* colsum, float colsum_scale,
                   void* stream);
/* Grouped form of emoasr_gemm_tn: n <= EMOASR_TN_GROUP_MAX independent, always-accumulating
 * products C_i += alpha_i * A_i^T . B_i (+ colsum_i) in ONE launch.  One encoder layer's backward
 * has ~10 weight gradients of 16..64 output tiles each (autograd would run them as 10 separate
 * addmm kernels); grouped they fill the chip. */
#define EMOASR_TN_GROUP_MAX 16
typedef struct emoasr_tn_problem {
  int N1, N2, K;
  const void* A; long lda;
  const void* B; long ldb;
  float* C; long ldc;
  float alpha;
  float* colsum;        /* optional bias gradient, see emoasr_gemm_tn */
  float colsum_scale;
} emoasr_tn_problem_t;
int emoasr_gemm_tn_grouped(int dtype, int n, const emoasr_tn_problem_t* probs, void* stream);
/* The launch plan emoasr_gemm_tn_grouped would use for these shapes, without launching (host only; the pointer fields of
 * probs are not read): splits[i] = split-K slices of problem i, *tile = the tile edge, *blocks = workgroups of the launch. */
int emoasr_gemm_tn_grouped_plan(int dtype, int n, const emoasr_tn_problem_t* probs, int* splits, int* tile, int* blocks);
/* out[N] (+)= scale * sum_rows X[M,N]   (bias gradients) */
int emoasr_colsum(int dtype, int M, int N, const void* X, long ldx, float* out, float scale,
                  int accumulate, void* stream);

/* ---- Conv2d subsampling front-end (asr/modeling/encoders/conv.py:5-28) ------
 * x f32 [B,T,F] -> y1 T [B,T1,F1,C] (channels-last), T1=(T-3)/2+1, F1=(F-3)/2+1
 * w1 f32 [C,9], b1 f32 [C]; ReLU fused.
 * B == 0 is an empty call on every entry of this section: nothing is launched; the weight-gradient entries (conv1_wgrad,
 * conv2_wgrad, conv2_dgrad_w1) zero their outputs when accumulate == 0 and leave them alone otherwise.  (A segment of
 * emoasr_conv2_wgrad_seg must have B > 0.) */
int emoasr_conv1_fwd(int dtype, int B, int T, int F, int C, const float* x, const float* w1,
                     const float* b1, void* y1, void* stream);
/* dw1[C,9], db1[C] (+)= from dy1 (gradient w.r.t. the pre-ReLU conv1 output);
 * scratch: emoasr_conv1_wgrad_scratch_floats(B, T, C) floats of per-block partial sums */
int emoasr_conv1_wgrad(int dtype, int B, int T, int F, int C, const float* x, const void* dy1,
                       float* dw1, float* db1, int accumulate, float* scratch, void* stream);
long emoasr_conv1_wgrad_scratch_floats(int B, int T, int C);
/* y2[(b,t2,f2), n] = epilogue(sum y1[b,2t2+kh,2f2+kw,c] * w[n,(kh,kw,c)])  (implicit GEMM) */
int emoasr_conv2_fwd(int dtype, int B, int T1, int F1, int C, const void* y1, const void* w, void* y2,
                     const emoasr_epilogue_t* ep, void* stream);
/* dw[n,(kh,kw,c)] (+)= dy2^T . im2col(y1);  dbias[n] (+)= sum dy2 (may be NULL) */
int emoasr_conv2_wgrad(int dtype, int B, int T1, int F1, int C, const void* dy2, const void* y1,
                       float* dw, float* dbias, int accumulate, void* stream);
/* The same over up to EMOASR_CONV2_WGRAD_SEGMENTS micro-batches (each with its own B and T1; F1, C shared) as ONE reduction:
 * one launch pays the split-K atomics into dw once instead of once per micro-batch.  Always accumulates.  bf16 with C a
 * multiple of 256 and option "tn_big" on runs as one launch of the 256x256-tile kernel; anything else as nseg calls of
 * emoasr_conv2_wgrad. */
#define EMOASR_CONV2_WGRAD_SEGMENTS 8
typedef struct emoasr_conv2_wgrad_seg {
  const void* dy2;   /* [B, T2, F2, C] */
  const void* y1;    /* [B, T1, F1, C] */
  int B, T1;
} emoasr_conv2_wgrad_seg_t;
int emoasr_conv2_wgrad_seg(int dtype, int nseg, const emoasr_conv2_wgrad_seg_t* segs, int F1, int C, float* dw,
                           float* dbias, void* stream);
/* dy1[b,t1,f1,c] = relu'(y1) * sum_{kh,kw} dcol[(b,t2,f2),(kh,kw,c)]  (col2im gather) */
/* Data gradient of the same convolution without an im2col buffer (four implicit GEMMs, one per parity class of
 * the output position): dy1[b,t1,f1,c] = relu'(y1[b,t1,f1,c]) * sum_{kh,kw,n} dy2[b,(t1-kh)/2,(f1-kw)/2,n]*w[n,(kh,kw,c)];
 * w = the [C, 9C] layout of emoasr_conv2_fwd.  Replaces gemm_nn (dcol) + emoasr_conv2_col2im. */
int emoasr_conv2_dgrad(int dtype, int B, int T1, int F1, int C, const void* dy2, const void* w, const void* y1,
                       void* dy1, void* stream);
int emoasr_conv2_col2im(int dtype, int B, int T1, int F1, int C, const void* dcol, const void* y1,
                        void* dy1, void* stream);
/* The same data gradient on the large-tile kernel (csrc/gemm_big.hip; bf16, C % 256 == 0): all four parity classes in ONE
 * launch.  wt = the weight laid out [c][kh][kw][n] (conv.2.weight.permute(1,2,3,0)), so that every tap's reduction over the
 * output channels n is contiguous. */
int emoasr_conv2_dgrad_kc(int dtype, int B, int T1, int F1, int C, const void* dy2, const void* wt, const void* y1,
                          void* dy1, void* stream);
/* emoasr_conv2_dgrad_kc with the first convolution's weight gradient in its epilogue: dy1 is never stored.  B, T, F: the shape
 * of conv1's input x f32 [B,T,F]; dw1[C,9], db1[C] (+)= what emoasr_conv1_wgrad computes from the dy1 above.
 * scratch: emoasr_conv2_dgrad_w1_scratch_floats(B, T, F, C) floats (per-tile partial sums). */
int emoasr_conv2_dgrad_w1(int dtype, int B, int T, int F, int C, const void* dy2, const void* wt, const void* y1,
                          const float* x, float* dw1, float* db1, int accumulate, float* scratch, void* stream);
long emoasr_conv2_dgrad_w1_scratch_floats(int B, int T, int F, int C);
/* Large-tile NT product for long, wide shapes (bf16; N % 8 == 0, K % 64 == 0): C = relu?(A . B^T + bias).  The kernel
 * behind emoasr_conv2_fwd / _dgrad_kc on a plain row-major A (nn.Linear with >= 256 outputs over >= 10^5 rows). */
int emoasr_gemm_nt_big(int dtype, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                       const float* bias, int relu, void* stream);

/* ---- LayerNorm (nn.LayerNorm call sites: conformer.py:183-187,
 * encoders/transformer.py:73, transformer.py:140-141,178-180) ------------------ */
int emoasr_layernorm_fwd(int dtype, int M, int N, const void* x, const float* gamma, const float* beta,
                         float eps, void* y, float* mean, float* rstd, void* stream);
/* dx = dres + LN'(dy); dgamma/dbeta (+)= ; dres may be NULL.  scratch: f32 workspace of
 * emoasr_layernorm_bwd_scratch_floats(N) floats (per-block partial sums; NULL if no dgamma/dbeta) */
int emoasr_layernorm_bwd(int dtype, int M, int N, const void* dy, const void* x, const float* gamma,
                         const float* mean, const float* rstd, const void* dres, void* dx,
                         float* dgamma, float* dbeta, float* scratch, void* stream);
long emoasr_layernorm_bwd_scratch_floats(int N);
/* Extended form.  dy2 (optional) = dropout(dx * scale2; drop_p2, seed2), computed from the stored dx:
 * the gradient entering the next residual branch x + scale2 * dropout(f(x)) of the backward sweep, so
 * that branch needs no separate emoasr_scale_dropout pass (same mask index: row * N + col).
 * defer_finalize != 0 leaves the dgamma / dbeta partial sums in `scratch` (which must then stay
 * untouched) for one emoasr_layernorm_bwd_finalize call that folds up to EMOASR_LN_FINALIZE_MAX
 * LayerNorms in a single launch. */
typedef struct emoasr_ln_bwd_opts {
  void* dy2;
  float scale2, drop_p2;
  uint64_t seed2;
  int defer_finalize;
} emoasr_ln_bwd_opts_t;
int emoasr_layernorm_bwd_ex(int dtype, int M, int N, const void* dy, const void* x, const float* gamma,
                            const float* mean, const float* rstd, const void* dres, void* dx,
                            float* dgamma, float* dbeta, float* scratch, const emoasr_ln_bwd_opts_t* opts,
                            void* stream);
#define EMOASR_LN_FINALIZE_MAX 64
typedef struct emoasr_ln_finalize_item {
  int M, N;              /* the M, N of the deferred emoasr_layernorm_bwd_ex call */
  const float* part;     /* its scratch */
  float *dgamma, *dbeta; /* accumulated into (either may be NULL) */
} emoasr_ln_finalize_item_t;
int emoasr_layernorm_bwd_finalize(int n, const emoasr_ln_finalize_item_t* items, void* stream);

/* ---- attention (transformer.py:48-99, conformer.py:57-95) -------------------
 * q:[B,Tq,H*DK] k,v:[B,Tk,H*DK] with row strides ldq/ldk/ldv (elements), out [B,Tq,H*DK].
 * pos: projected relative position table T [2*Tq-1, H*DK] (row r <-> rel = Tq-1-r) or NULL;
 * bias_u / bias_v f32 [H*DK] or NULL.  klens int32 [B]: keys >= klens[b] are masked
 * (NULL: none).  causal != 0 adds the lower-triangular mask (decoder self-attn).
 * scores = ((q+u).k + (q+v).pos[i-j]) * scale; softmax; dropout(drop_p); .v
 * lse f32 [B,H,Tq] is saved for backward. */
#define EMOASR_MAX_SEGMENTS 8
typedef struct {
  int B, H, DK, Tq, Tk;
  long ldq, ldk, ldv, ldo, ldp;
  const void *q, *k, *v, *pos;
  const float *bias_u, *bias_v;
  const int* klens;
  int causal;
  float scale;
  float drop_p;
  uint64_t seed;
  void* out;
  float* lse;
  /* backward only */
  const void* dout;
  float* delta; /* scratch f32 [B,H,Tq] */
  void *dq, *dk, *dv; /* T, same strides as q/k/v */
  float *dpos;        /* f32 [2*Tq-1, H*DK], accumulated */
  float *dbias_u, *dbias_v; /* f32 [H*DK], accumulated */
  /* optional backward scratch ("materialised" mode): when pdT != NULL the dq kernel stores the
   * dropped probabilities P^T and dS^T (and the un-shifted dBD band) once, and dV / dK / dpos are
   * computed by batched GEMMs over them instead of recomputing the scores three more times.
   * All three must be zero-filled by the caller before the first use for a given
   * (B, Tq, Tk, klens) and may then be reused by later calls with the same masks (the set of
   * never-written entries does not change).  Row strides ldpd >= Tq, ldbd >= 2*Tq-1, both
   * multiples of 8 elements. */
  void *pdT, *dsT;    /* T [B,H,Tk,ldpd] */
  void *dbd;          /* T [H,B,Tq,ldbd]; NULL without relative positions */
  long ldpd, ldbd;
  float* cs;          /* f32 [H, ldbd] scratch */
  /* optional: scaled scores S^T, f32 [B,H,Tk,ldst] (ldst >= Tq).  The forward stores them when
   * st != NULL; a backward given the same buffer (with the scratch above) reads them back instead
   * of recomputing (q+u).k + (q+v).pos, and computes the (q+v) part of dq as a batched GEMM over
   * the stored dBD band. */
  float* st;
  long ldst;
  /* optional, materialised backward only: Q + pos_bias_u and Q + pos_bias_v as dense T [B,Tq,H*DK]
   * tensors (written by the backward's first pass; the dK and dpos GEMMs then need no bias fix-up
   * passes), and per-(batch, query tile) partial sums of dbias_u / dbias_v, f32
   * [B * ceil(Tq/32), H, 2, DK], folded by one small reduction instead of contended atomics. */
  void *qu, *qv;
  float* dbias_part;
  /* optional: several stacked micro-batches ("segments", see emoasr_segments_t below) in ONE launch -- emoasr_attn_fwd and
   * emoasr_attn_bwd_fused only, self-attention (Tq == Tk).  nseg > 1: segment s holds utterances seg_b0[s] .. seg_b0[s+1]-1,
   * each padded to seg_T[s] frames; its rows start at row seg_row[s] of q / k / v / out / dout / dq / dk / dv (seg_row[nseg] =
   * all rows), its relative-position table at row seg_prow[s] of pos / dpos; lse and delta are [H * rows]: segment s at
   * H * seg_row[s], laid out [utterances, H, seg_T[s]].  B = all utterances, Tq = Tk = the longest segment, klens [B] in
   * order.  The dropout mask index restarts in every segment (seed + s * 0x9E3779B97F4A7C15).  nseg <= 1: one dense batch. */
  int nseg;
  int seg_b0[EMOASR_MAX_SEGMENTS + 1], seg_T[EMOASR_MAX_SEGMENTS];
  long seg_row[EMOASR_MAX_SEGMENTS + 1], seg_prow[EMOASR_MAX_SEGMENTS + 1];
  /* filled by the library (callers leave it zero): the order in which a stacked launch hands out its segments' workgroups --
   * longest segment first, so that the short ones fill the tail of the launch */
  int seg_order[EMOASR_MAX_SEGMENTS];
  /* optional (round 6, bf16 training): the attention-dropout keep mask of this launch as BITS -- uint32 [rows, H, keep_nw], one word
   * per (query row, head, 32-key tile), bit k of word w = key 32 w + k kept; rows = B * Tq (stacked: all segments' rows, in order).
   * emoasr_attn_dropmask hashes it ONCE per layer and step (dropout(p=dropout_attn_rate) of transformer.py:88); emoasr_attn_fwd and
   * both passes of emoasr_attn_bwd_fused then test a bit (2-3 instructions per element) instead of hashing the counter-based mask
   * again (13-26 per element).  NULL: the kernels hash inline / the backward fills a mask of its own. */
  const unsigned* keep_mask;
  int keep_nw;
} emoasr_attn_t;
/* words per (row, head) of a keep mask for keys 0 .. Tk-1, and the mask of the launch described by `a` (q / k / v pointers are not
 * read: B, H, Tq, Tk, klens, drop_p, seed and the segment table are) written to mask [rows, H, nw] */
long emoasr_attn_dropmask_words(int Tk);
int emoasr_attn_dropmask(int dtype, const emoasr_attn_t* a, unsigned* mask, int nw, void* stream);
int emoasr_attn_fwd(int dtype, const emoasr_attn_t* a, void* stream);
int emoasr_attn_bwd(int dtype, const emoasr_attn_t* a, void* stream);
/* The materialised mode's optional scratch as TWO areas instead of seven pointers: emoasr_attn_bwd_mat_bytes(..., which) bytes each
 * -- which = 0: the images (P^T, dS^T, dBD band; zero-filled by the caller before the first call for a given (B, Tq, Tk, klens),
 * reusable by later calls with the same masks, e.g. every layer of a backward sweep); which = 1: plain scratch (cs, Q + bias copies,
 * dbias partials; no initialisation, reusable by any call).  emoasr_attn_bwd_mat_bind fills pdT / dsT / dbd / ldpd / ldbd / cs /
 * qu / qv / dbias_part of `a` (B, H, Tq, Tk, pos, bias_u, bias_v already set) from the two base addresses.  Replaces the
 * tensor-by-tensor allocation of emoasr_amd/ops.py: AttnScratch for C callers (csrc/layer.hip: the f32 layer backward). */
size_t emoasr_attn_bwd_mat_bytes(int dtype, int B, int H, int Tq, int Tk, int rel, int which);
int emoasr_attn_bwd_mat_bind(int dtype, emoasr_attn_t* a, void* images, void* scratch);
/* Single-pass backward (bf16, no causal mask): every score tile is recomputed once; dQ, dK, dV, dbias_u/v and dpos come
 * out of four launches (prologue: delta, Q+u, Q+v, zeroed dQ accumulator; main: one workgroup per (batch, head, 128 keys)
 * sweeping the query tiles; dpos: diagonals of the stored dS; finalize: dQ f32 -> T and dbias_v).  Replaces the
 * materialised mode of emoasr_attn_bwd (P^T / dS^T / dBD images + three GEMMs): same arguments, the pdT / dsT / dbd / cs /
 * st / qu / qv / dbias_part fields are ignored.  `ws`: emoasr_attn_bwd_fused_ws_bytes(...) bytes of scratch, no
 * initialisation needed.  Reference: transformer.py:73-94, conformer.py:77-95 (their autograd backward). */
size_t emoasr_attn_bwd_fused_ws_bytes(int dtype, int B, int H, int Tq, int Tk, int rel);
/* the same for `rows` rows in all (stacked micro-batches: the segments' rows together, Tk = the longest segment) */
size_t emoasr_attn_bwd_fused_ws_bytes_rows(int dtype, long rows, int H, int Tk, int rel);
int emoasr_attn_bwd_fused(int dtype, const emoasr_attn_t* a, void* ws, size_t ws_bytes, void* stream);

/* ---- Conformer convolution module (conformer.py:98-143) ---------------------- */
/* out[M,C] = in[M,:C] * sigmoid(in[M,C:2C]) */
int emoasr_glu_fwd(int dtype, int M, int C, const void* in, void* out, void* stream);
int emoasr_glu_bwd(int dtype, int M, int C, const void* in, const void* dout, void* din, void* stream);
/* emoasr_glu_fwd over in [B,T,2C] with zeros at the frames t >= lens[b] (lens int32 [B]): inference on a padded batch whose
 * depthwise convolution must see every utterance as it sees it alone (zero padding past its own end) */
int emoasr_glu_fwd_masked(int dtype, int B, int T, int C, const void* in, const int* lens, void* out, void* stream);
/* depthwise Conv1d over time, channels-last x[B,T,C], w f32 [C,K], zero padding (K-1)/2 */
int emoasr_dwconv_fwd(int dtype, int B, int T, int C, int K, const void* x, const float* w,
                      const float* bias, void* y, void* stream);
int emoasr_dwconv_bwd_x(int dtype, int B, int T, int C, int K, const void* dy, const float* w, void* dx,
                        void* stream);
/* depthwise_conv -> batch_norm of conformer.py:129-131 with the batch statistics fused: the conv also
 * writes per-block (sum, centred sum of squares) partials of its stored output into `part`
 * (emoasr_dwconv_stats_floats(B,T,C) floats); emoasr_bn_stats_finalize merges them (Chan's parallel
 * variance) into mean / biased var [C], updates the running statistics (unbiased var, `momentum`) and
 * increments num_batches_tracked (int64 on the device; all three optional), as nn.BatchNorm1d does. */
long emoasr_dwconv_stats_floats(int B, int T, int C);
int emoasr_dwconv_fwd_stats(int dtype, int B, int T, int C, int K, const void* x, const float* w,
                            const float* bias, void* y, float* part, void* stream);
int emoasr_bn_stats_finalize(int B, int T, int C, const float* part, float* mean, float* var,
                             float* running_mean, float* running_var, float momentum,
                             long long* num_batches_tracked, void* stream);
/* scratch: emoasr_dwconv_bwd_w_scratch_floats(B,T,C,K) floats of per-block partial sums */
int emoasr_dwconv_bwd_w(int dtype, int B, int T, int C, int K, const void* dy, const void* x, float* dw,
                        float* dbias, int accumulate, float* scratch, void* stream);
long emoasr_dwconv_bwd_w_scratch_floats(int B, int T, int C, int K);
/* BatchNorm1d batch statistics over all M=B*T rows (padding included, as the reference):
 * mean[C], var[C] (biased); if running_* != NULL they are updated with `momentum`
 * (unbiased variance), exactly like nn.BatchNorm1d in training mode. */
int emoasr_bn_stats(int dtype, int M, int C, const void* y, float* mean, float* var,
                    float* running_mean, float* running_var, float momentum, void* stream);
/* z = swish(gamma*(y-mean)/sqrt(var+eps)+beta) */
int emoasr_bn_swish_fwd(int dtype, int M, int C, const void* y, const float* mean, const float* var,
                        const float* gamma, const float* beta, float eps, void* z, void* stream);
/* training-mode backward (batch statistics): dy from dz; dgamma/dbeta (+)=.  C % 8 == 0.
 * scratch: emoasr_bn_swish_bwd_scratch_floats(M, C) floats of per-block partial sums
 * (ceil(M/64) x 2 x C); needs no initialisation. */
long emoasr_bn_swish_bwd_scratch_floats(int M, int C);
int emoasr_bn_swish_bwd(int dtype, int M, int C, const void* dz, const void* y, const float* mean,
                        const float* var, const float* gamma, const float* beta, float eps, void* dy,
                        float* dgamma, float* dbeta, float* scratch, void* stream);
/* ---- fused convolution-module kernels (csrc/convfused.hip; bf16, K <= 31, C % 8 == 0): bit-identical to the separate
 * launches they replace (every intermediate is rounded to bf16 at the same point); dw / dbias of emoasr_conv_bwd_fused below
 * 1024 tiles (B * ceil(Tn / 32) < 1024) -- from there on they are folded in four slices that meet in float atomics: the same sums
 * in another order, not run-to-run deterministic.
 * emoasr_glu_dwconv_fwd: c = depthwise_conv(GLU(g)), g [B*T, 2C]; part (may be NULL) receives the per-block BatchNorm
 *   partial statistics of emoasr_dwconv_fwd_stats.  conformer.py:126-131.
 * emoasr_bn_swish_bwd_sums: passes 1-2 of emoasr_bn_swish_bwd (dgamma / dbeta accumulated; *tot_out = the [2][C] means
 *   inside `scratch`).
 * emoasr_conv_bwd_fused: given those means, ds (gradient w.r.t. the Swish output), cv (the depthwise convolution's output)
 *   and g -> dg [B*T, 2C] (BatchNorm/Swish backward, depthwise data gradient, GLU backward) and dw [C,K] / dbias [C]
 *   accumulated (the GLU output is recomputed from g).  scratch: emoasr_dwconv_bwd_w_scratch_floats() floats. */
int emoasr_glu_dwconv_fwd(int dtype, int B, int Tn, int C, int K, const void* g, const float* w, const float* bias, void* c,
                          float* part, void* stream);
int emoasr_bn_swish_bwd_sums(int dtype, int M, int C, const void* dz, const void* y, const float* mean, const float* var,
                             const float* gamma, const float* beta, float eps, float* dgamma, float* dbeta, float* scratch,
                             float** tot_out, void* stream);
int emoasr_conv_bwd_fused(int dtype, int B, int Tn, int C, int K, const void* ds, const void* cv, const float* mean,
                          const float* var, const float* gamma, const float* beta, float eps, const float* tot, const void* g,
                          const float* w, void* dg, float* dw, float* dbias, float* scratch, void* stream);

/* ---- element-wise / layout helpers ------------------------------------------ */
/* out (contiguous [d0,d1,d2,d3], dtype_out) (+)= in[strides s0..s3 (elements), dtype_in] */
int emoasr_strided_copy(int dtype_in, int dtype_out, const void* in, void* out, int d0, int d1, int d2,
                        int d3, long s0, long s1, long s2, long s3, int accumulate, void* stream);
/* y = x*scale*dropout(seed, i)  (n elements) */
int emoasr_scale_dropout(int dtype, long n, const void* x, void* y, float scale, float drop_p,
                         uint64_t seed, void* stream);
/* y[b,t,:] = (x[b,t,:]*scale + pe[t,:]) * dropout   (absolute positional encoding,
 * transformer.py:43-45); pe f32 [>=T, N] or NULL (conformer.py:49: scale only) */
int emoasr_posenc(int dtype, int B, int T, int N, const void* x, const float* pe, float scale,
                  float drop_p, uint64_t seed, void* y, void* stream);
/* dx[i] = dy[i] * act'(pre[i])  (act: EMOASR_ACT_*; pre = the saved pre-activation) */
int emoasr_act_bwd(int dtype, long n, int act, const void* dy, const void* pre, void* dx, void* stream);
/* y[i] = a[i] + b[i] */
int emoasr_add(int dtype, long n, const void* a, const void* b, void* y, void* stream);

/* dst_i [cols_i, rows_i] (compute dtype `dtype_out`, row stride ld_dst_i) = transpose of src_i [rows_i, cols_i] (f32, dense), all
 * n items in ONE launch: the transposed weight copies of emoasr_conformer_layer_t, refreshed after every optimizer step. */
typedef struct emoasr_tc_item {
  const float* src; void* dst;
  int rows, cols; long ld_dst;
} emoasr_tc_item_t;
#define EMOASR_TC_MAX 64
int emoasr_transpose_cast_batched(int dtype_out, int n, const emoasr_tc_item_t* items, void* stream);

/* ---- CTC (decoders/ctc.py:36-38,103-115,176-201; torch.nn.CTCLoss semantics) -- */
/* lse[m] = logsumexp_v logits[m,:V] */
int emoasr_row_lse(int dtype, int M, int V, const void* logits, long ld, float* lse, void* stream);
/* The CTC head in one pass (csrc/gemm_big.hip; bf16, N % 8 == 0, K % 64 == 0): C = A . B^T + bias stored AND lse[m] = log sum_n
 * exp(C[m,n]) of the row as stored -- the soft-max partials leave the product's epilogue (part: scratch [ceil(N / 64), M, 2] f32)
 * instead of a second pass over the logits (emoasr_gemm_nt + emoasr_row_lse).  decoders/ctc.py:103-113. */
int emoasr_gemm_nt_lse(int dtype, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                       const float* bias, float* part, float* lse, void* stream);
/* Forward-backward lattices.  S = 2*Lmax+1 states.  lp (scratch), alpha, beta: f32 [B,T,S];
 * nll[b] = -log p(labels_b | x_b) (+inf if infeasible).  alpha and beta both include the
 * emission at t, so occupancy(t,s) = exp(alpha+beta-lp+nll). */
int emoasr_ctc_forward(int dtype, int B, int T, int V, int Lmax, const void* logits, long ld,
                       const float* lse, const int* labels, const int* elens, const int* ylens, int blank,
                       float* lp, float* alpha, float* beta, float* nll, void* stream);
/* gscale_dev (device, 1 float, may be NULL) multiplies gscale without a host sync.
 * grad[b,t,v] = gscale * (softmax - occupancy) for t < elens[b]; 0 elsewhere and for
 * utterances with nll = inf (zero_infinity=True). */
int emoasr_ctc_grad(int dtype, int B, int T, int V, int Lmax, const void* logits, long ld,
                    const float* lse, const int* labels, const int* elens, const int* ylens, int blank,
                    const float* lp, const float* alpha, const float* beta, const float* nll,
                    float gscale, const float* gscale_dev, void* grad, long ldg, void* stream);
/* The same for the utterances of several stacked micro-batches in one set of launches (engine.ctc_train_stacked): utterance b's
 * logits / lse / gradient rows are row0[b] + t, t < tpad[b] (its micro-batch's padded length; rows t >= tpad[b] do not exist),
 * instead of b * Tn + t; the lattice tables lp / alpha / beta stay [B, Tn, S] with Tn = the longest padded length; uscale[b]
 * (optional) multiplies gscale per utterance (micro-batch weight / micro-batch size).  row0 == NULL: the dense layout. */
int emoasr_ctc_forward_rows(int dtype, int B, int Tn, int V, int Lmax, const void* logits, long ld, const float* lse,
                            const int* labels, const int* elens, const int* ylens, int blank, const long* row0, float* lp,
                            float* alpha, float* beta, float* nll, void* stream);
int emoasr_ctc_grad_rows(int dtype, int B, int Tn, int V, int Lmax, const void* logits, long ld, const float* lse,
                         const int* labels, const int* elens, const int* ylens, int blank, const float* lp, const float* alpha,
                         const float* beta, const float* nll, float gscale, const float* gscale_dev, const long* row0,
                         const int* tpad, const float* uscale, void* grad, long ldg, void* stream);
/* greedy: best[b,t] = argmax_v logits (first max wins); hyp[b,:hyplen[b]] = collapse
 * repeats then drop blank, over t < elens[b] */
int emoasr_ctc_greedy(int dtype, int B, int T, int V, const void* logits, long ld, const int* elens,
                      int blank, int* best, int* hyp, int* hyplen, void* stream);

/* ---- Transformer decoder side (decoders/transformer.py:82-146, criteria.py:5-46) ---- */
/* out[m,:] = (table[ids[m],:]*scale + pe[m % L,:]) * dropout   (embedding + PositionalEncoder) */
int emoasr_embed_fwd(int dtype, int M, int L, int d, const int* ids, const void* table, const float* pe,
                     float scale, float drop_p, uint64_t seed, void* out, void* stream);
/* dtable[ids[m],:] += dout[m,:]*scale*dropout  (f32 atomics) */
int emoasr_embed_bwd(int dtype, int M, int d, const int* ids, const void* dout, float scale, float drop_p,
                     uint64_t seed, float* dtable, void* stream);
/* LabelSmoothingLoss rows: w[m] = 0 for padded positions, else the row weight (1/B [/ylen]);
 * loss[m] = -w*sum_v q[v]*log_softmax(logits[m])[v], q = 1-eps on labels[m], eps/(V-1) elsewhere;
 * grad (may be NULL) = gscale*[gscale_dev]*w*(softmax - q) */
int emoasr_lsm_loss(int dtype, int M, int V, const void* logits, long ld, const int* labels, const float* w,
                    float lsm_prob, float* loss, float gscale, const float* gscale_dev, void* grad, long ldg,
                    void* stream);

/* ---- knowledge distillation (asr/criteria.py:49-288, decoders/ctc_aligner.py:96-221) ---- */
/* Soft-target cross-entropy rows (one kernel behind DistillLoss, CTCAlignDistillLoss, RNNTWordDistillLoss,
 * RNNTAlignDistillLoss).  Row r reads logits row lrow[r] (lrow NULL: r), the dense f32 soft target
 * soft[src[r], :V] (src NULL or src[r] < 0: no soft term) and the label-smoothed hard target of class hard[r]
 * (hard NULL or < 0: none):  loss[r] = -(w_soft[r]*sum_v q_s[v] log p[v] + w_hard[r]*sum_v q_h[v] log p[v]);
 * grad (may be NULL; rows indexed like logits) = gscale*[gscale_dev]*(w_soft*(p*sum(q_s) - q_s) + w_hard*(p - q_h)) */
int emoasr_soft_ce(int dtype, int R, int V, const void* logits, long ld, const int* lrow, const float* soft, long lds,
                   const int* src, const int* hard, const float* w_soft, const float* w_hard, float lsm_prob,
                   float* loss, float gscale, const float* gscale_dev, void* grad, long ldg, void* stream);
/* CTCForcedAligner.__call__ (ctc_aligner.py:139-221) on the lattices of emoasr_ctc_forward (same lp/alpha/beta
 * [B,Tn,2*Lmax+1]): aligns[b,t] (int32 [B,Tn]) = token of the best state among those reachable from frame t-1's
 * choice, 0 for t >= elens[b]. */
int emoasr_ctc_best_path(int B, int Tn, int Lmax, const float* lp, const float* alpha, const float* beta,
                         const int* labels, const int* elens, const int* ylens, int blank, int* aligns, void* stream);
/* CTCAlignDistillLoss._frame_to_label_mapping (criteria.py:170-215): label_map[b,t] = index of the label that
 * frame t is assigned to, or -1; position 0 "all", 1 "left", 2 "mid", 3 "right"; count[b] = frames mapped. */
int emoasr_ctc_label_map(int B, int Tn, const int* aligns, const int* xlens, int blank, int position, int* label_map,
                         int* count, void* stream);

/* RNNTForcedAligner.__call__ (decoders/rnnt_aligner.py:158-198) on the lattices of emoasr_rnnt_forward (alpha, beta
 * f32 [B,Tn,U]): aligns (int32 [B,U-1]) = frame at which each label is emitted along the greedy alpha+beta walk;
 * labels not reached before the last frame keep 0. */
int emoasr_rnnt_best_path(int B, int Tn, int U, const float* alpha, const float* beta, const int* elens,
                          const int* ylens, int* aligns, void* stream);

/* ---- joint CTC/attention beam search (decoders/transformer.py:161-294, ctc_score.py:13-85) ---- */
/* out[m,v] = log_softmax(x[m,:V])[v] + mu*add[m,v]   (add may be NULL; f32 out) */
int emoasr_log_softmax(int dtype, int M, int V, const void* x, long ldx, const float* add, long lda, float mu,
                       float* out, long ldo, void* stream);
/* k largest per row, descending, ties to the lowest index; aux (optional) is gathered at the same
 * indices into aux_out */
int emoasr_topk(int M, int V, int k, const float* x, long ldx, const float* aux, long ldaux, float* vals,
                int* idx, float* aux_out, void* stream);
/* log_softmax(dec row) + mu * log_softmax(lm row) and its k largest entries in one launch (the beam search needs nothing
 * else of the score rows): vals / idx as emoasr_topk, lm_at = log_softmax(lm)[idx].  dec: compute dtype [M, V]; lm: f32 raw
 * logits [M, V] or NULL. */
int emoasr_beam_scores_topk(int dtype, int M, int V, int k, const void* dec, long ldd, const float* lm, long ldl, float mu,
                            float* vals, int* idx, float* lm_at, void* stream);
/* CTCPrefixScorer.initial_state: r f32 [T,2] from the CTC log-probs x f32 [T,V] */
int emoasr_ctc_prefix_init(int T, int V, const float* x, int blank, float* r, void* stream);
/* CTCPrefixScorer.__call__ for nb beams x cw candidates.  Beam m's previous state is
 * prev_states[parent[m], pcand[m]] (prev_states f32 [*, cw_prev, T, 2]) or init_state when
 * prev_states == NULL; last[m] / out_len[m] = last label and number of labels of the prefix.
 * -> log_psi f32 [nb,cw], states f32 [nb,cw,T,2] */
int emoasr_ctc_prefix_score(int nb, int T, int V, int cw, const float* x, const float* prev_states, int cw_prev,
                            const int* parent, const int* pcand, const float* init_state, const int* last,
                            const int* out_len, const int* cands, int blank, int eos, float* log_psi,
                            float* states, void* stream);

/* ---- RNN-Transducer decoder (decoders/rnn_transducer.py:81-240) ----------------------
 * LSTM cell (nn.LSTM gate order i,f,g,o): gates_pre T [B,4H] = x.W_ih^T + h.W_hh^T + b;
 * c_prev / c f32 [B,H]; h T rows of stride ldh; gates_act T [B,4H] saved for the backward. */
int emoasr_lstm_cell_fwd(int dtype, int B, int H, const void* gates_pre, const float* c_prev, void* h, long ldh,
                         float* c, void* gates_act, void* stream);
/* dgates_pre from dh_out (row stride lddh) + dh_rec (may be NULL); dc f32 [B,H] is updated in place */
int emoasr_lstm_cell_bwd(int dtype, int B, int H, const void* dh_out, long lddh, const void* dh_rec, float* dc,
                         const void* gates_act, const float* c_prev, const float* c, void* dgates_pre,
                         void* stream);
/* The whole recurrence of one LSTM layer in one cooperative launch (csrc/lstm_coop.hip; bf16, B <= 64, H % 32 == 0, H <= 512):
 * pre [U][B][4H] = x . W_ih^T + b_ih + b_hh, w_hh [4H][H]; outputs hseq [U][B][H], cseq f32 [U][B][H], gact [U][B][4H] (activated
 * i | f | g | o).  h0 / c0 may be NULL (zeros).  emoasr_lstm_seq_supported() -> 1 if this shape runs here (option "lstm_coop").  Launches on DIFFERENT streams are ordered against each other by a per-device event chain (two partly resident cooperative
 * launches would wait for each other's workgroups): streams overlap everything else, not two recurrences. */
int emoasr_lstm_seq_supported(int dtype, int B, int H);
int emoasr_lstm_seq_fwd(int dtype, int U, int B, int H, const void* pre, const void* w_hh, const void* h0, const float* c0,
                        void* hseq, float* cseq, void* gact, void* stream);
/* ... and backward: dgp [U][B][4H] (gradient w.r.t. the gate pre-activations) from dh_seq [U][B][H] (gradient w.r.t. the outputs),
 * the stored gact / cseq and c0 (may be NULL); ws: emoasr_lstm_seq_bwd_ws_bytes(B, H) bytes of scratch.
 * emoasr_lstm_coop_status(): 0 unless a grid barrier of these kernels ever gave up waiting (synchronises the device). */
long emoasr_lstm_seq_bwd_ws_bytes(int B, int H);
int emoasr_lstm_seq_bwd(int dtype, int U, int B, int H, const void* dh_seq, const void* gact, const float* cseq, const float* c0,
                        const void* w_hh, void* dgp, void* ws, long ws_bytes, void* stream);
long emoasr_lstm_coop_status(void);
/* The RNN encoder's bidirectional LSTM layer with per-utterance lengths (csrc/bilstm.hip; engine._RNNEncMixin is the call site):
 * nn.LSTM(bidirectional=True, batch_first=True) over pack_padded_sequence(x, elens) as a per-step chain.  Step s = 0 .. T - 1
 * (T = max elens) of row b works on frame t = s (direction 0, forward) or t = elens[b] - 1 - s (direction 1, reverse); a row with
 * s >= elens[b] is inactive and writes zeros to its frame s (so padded frames of every output are exact zeros, every frame is
 * written once per direction, and no negative t is ever formed).  elens int32 [B] on the device, every entry in 1 .. T.
 * emoasr_bilstm_cell_fwd: pre [B][T][8H] (row stride ldp >= 8H: x . W_ih^T + b_ih + b_hh, direction d's i | f | g | o at columns
 *   4H d ..); rec [2][B][4H] = hstate . W_hh^T of the step (NULL at s = 0: zero state); hstate [2][B][H] in: h of step s - 1, out: of
 *   step s; cstate f32 [2][B][H] likewise; outputs at (d, b, t): hseq [2][B][T][H], hprev [2][B][T][H] (the h the cell started from:
 *   the W_hh gradient is hprev^T-paired with dg, row for row), cseq f32 [2][B][T][H], gact [2][B][T][4H] (activated gates).
 * emoasr_bilstm_cell_bwd: steps s = T - 1 .. 0; dy [B][T][H] is the gradient w.r.t. the summed output (both directions take it);
 *   dh_rec [2][B][H] = dgc of step s + 1 . W_hh (NULL at s = T - 1: dh_rec = dc = 0); dcstate f32 [2][B][H] in/out; outputs
 *   dg [2][B][T][4H] (gradient w.r.t. the gate pre-activations, zero at padded frames) and dgc [2][B][4H] (this step's rows).
 * emoasr_bilstm_out: y [B][T][H] = dropout(x0 + x1) at t < elens[b], 0 beyond (x1 may be NULL: the backward's masked dropout); the
 *   keep mask is emoasr_scale_dropout's of the flat index. */
int emoasr_bilstm_cell_fwd(int dtype, int B, int T, int H, int s, const int* elens, const void* pre, long ldp, const void* rec,
                           void* hstate, float* cstate, void* hseq, void* hprev, float* cseq, void* gact, void* stream);
int emoasr_bilstm_cell_bwd(int dtype, int B, int T, int H, int s, const int* elens, const void* dy, const void* dh_rec,
                           float* dcstate, const void* gact, const float* cseq, void* dg, void* dgc, void* stream);
int emoasr_bilstm_out(int dtype, int B, int T, int H, const int* elens, const void* x0, const void* x1, void* y, float drop_p,
                      uint64_t seed, void* stream);
/* The same layer's recurrence as ONE cooperative launch for both directions (csrc/lstm_coop.hip; the call site is
 * engine._RNNEncMixin, option "lstm_coop"): barrier group = (direction, 64-row batch group), H / 16 workgroups each; same frame map,
 * inputs and outputs as the chain above (pre, hseq, hprev, cseq, gact forward; dy, gact, cseq -> dg backward), w_hh_f / w_hh_r
 * [4H][H].  emoasr_bilstm_seq_supported() -> 1 for bf16, B <= 256, H % 32 == 0, H <= 512 when every workgroup of both kernels
 * is resident by the occupancy query with one CU's worth to spare; otherwise the chain runs.  ws: emoasr_bilstm_seq_bwd_ws_bytes(B, H)
 * bytes of scratch.  A barrier that gave up is reported by emoasr_lstm_coop_status().  Not capturable into a graph. */
int emoasr_bilstm_seq_supported(int dtype, int B, int H);
long emoasr_bilstm_seq_bwd_ws_bytes(int B, int H);
int emoasr_bilstm_seq_fwd(int dtype, int B, int T, int H, const int* elens, const void* pre, long ldp, const void* w_hh_f,
                          const void* w_hh_r, void* hseq, void* hprev, float* cseq, void* gact, void* stream);
int emoasr_bilstm_seq_bwd(int dtype, int B, int T, int H, const int* elens, const void* dy, const void* gact, const float* cseq,
                          const void* w_hh_f, const void* w_hh_r, void* dg, void* ws, long ws_bytes, void* stream);
/* joint network: h[b,t,u,:] = tanh(e[b,t,:] + g[b,u,:]) ; reductions of d(pre-tanh) back to de / dg */
int emoasr_joint_tanh(int dtype, int B, int T, int U, int J, const void* e, const void* g, void* h, void* stream);
int emoasr_joint_reduce(int dtype, int B, int T, int U, int J, const void* d, void* de, void* dg, void* stream);
/* transducer lattice on joint logits T [B,T,U,V] (U = Lmax+1): per-cell lse / blank / label log-probs,
 * alpha, beta f32 [B,T,U], nll[b] = -log p(y_b|x_b) */
int emoasr_rnnt_forward(int dtype, int B, int T, int U, int V, int Lmax, const void* logits, const int* labels,
                        const int* elens, const int* ylens, int blank, float* lse, float* lpb, float* lpy,
                        float* alpha, float* beta, float* nll, void* stream);
/* dlogits = gscale*[gscale_dev]*(softmax*occ - [blank]gamma_b - [label]gamma_y); 0 outside (elens, ylens) */
int emoasr_rnnt_grad(int dtype, int B, int T, int U, int V, int Lmax, const void* logits, const float* lse,
                     const float* lpb, const float* lpy, const float* alpha, const float* beta, const int* labels,
                     const int* elens, const int* ylens, const float* nll, int blank, float gscale,
                     const float* gscale_dev, void* dlogits, void* stream);
/* The transducer's output layer WITHOUT the [B,T,U,V] logits (csrc/gemm_big.hip epilogues + csrc/rnnt.hip; bf16, V % 8 == 0,
 * J % 64 == 0).  Replaces `self.output(torch.tanh(...))` + `log_softmax` + warp_rnnt's gathers of rnn_transducer.py:101-115,
 * 147-156 for training: z = h . W^T + bias is formed tile by tile on the MFMA pipeline and reduced in the epilogue.
 *   emoasr_rnnt_head_fwd   cells row0 .. row0 + nrows (h: their joint activations [nrows, J]): per row and 64-column chunk the
 *                          soft-max partials part[c, row0 + n] = (max, sum exp(z - max)) -- part is the WHOLE chunk-major table
 *                          [ceil(V / 64), part_rows, 2] of all cells, every launch fills its rows -- and the two
 *                          logits the lattice reads, zb[n] = z[n, blank], zy[n] = z[n, labels[b, u]] (u < ylens[b]);
 *   emoasr_rnnt_forward_parts   lse from the partials, zb / zy turned into lpb / lpy IN PLACE, then the alpha / beta lattices and
 *                          nll exactly as emoasr_rnnt_forward;
 *   emoasr_rnnt_coef       the per-cell constants of the gradient (coef [cells, 4] = lse, occ, gamma_blank, gamma_label, the last
 *                          three times gscale [* gscale_dev]; ycol [cells] = label column or -1; zeros outside (elens, ylens));
 *   emoasr_rnnt_head_grad  dz[n, :] = exp(z - lse) occ - [blank] gamma_b - [label] gamma_y for the nrows cells of one row chunk,
 *                          z RECOMPUTED from h: the caller walks the cells in chunks (dz chunk -> emoasr_gemm_tn / _nn), so no
 *                          [cells, V] buffer exists in either direction. */
int emoasr_rnnt_head_fwd(int dtype, long row0, int nrows, int T, int U, int V, int J, int Lmax, const void* h, const void* w,
                         const float* bias, const int* labels, const int* ylens, int blank, float* part, long part_rows, float* zb,
                         float* zy, const int* ycol, void* stream);
/* ycol [B*T*U] for emoasr_rnnt_head_fwd: the label column of every lattice cell, labels[b, u] for u < ylens[b], else -1 */
int emoasr_rnnt_ycol(int B, int T, int U, int Lmax, const int* labels, const int* ylens, int* ycol, void* stream);
int emoasr_rnnt_forward_parts(int B, int T, int U, int V, const float* part, const int* elens, const int* ylens, float* lse,
                              float* zb_lpb, float* zy_lpy, float* alpha, float* beta, float* nll, void* stream);
int emoasr_rnnt_coef(int B, int T, int U, int Lmax, const float* lse, const float* lpb, const float* lpy, const float* alpha,
                     const float* beta, const int* labels, const int* elens, const int* ylens, const float* nll, float gscale,
                     const float* gscale_dev, float* coef, int* ycol, void* stream);
int emoasr_rnnt_head_grad(int dtype, int nrows, int V, int J, const void* h, const void* w, const float* bias, const float* coef,
                          const int* ycol, int blank, void* dz, long lddz, void* stream);
/* Cross-entropy vocabulary head WITHOUT the [rows, V] logits (the Transformer LM's output layer: lm/modeling/transformer.py:45-56,
 * 79-99; bf16, V % 8 == 0, V >= 64, K % 64 == 0 -- the Python caller, ops.ce_head_ok, takes it from V >= 256 and 1 024 rows on).  The two epilogues of the transducer head above with occ = gamma_label = row
 * weight and gamma_blank = 0:
 *   emoasr_ce_head_fwd   z = x . w^T + bias is reduced in the product's epilogue: lse[n] = log sum_v exp z[n, v],
 *                        logp[n] = z[n, y[n]] - lse[n] and (when loss != NULL) loss[n] = -wrow[n] * logp[n], with y[n] = labels[n]
 *                        clamped into [0, V) -- rows with an ignored label (-100) carry wrow = 0.  ycol [nrows] receives y;
 *                        part: scratch [ceil(V / 64), nrows, 2] f32; zscr: scratch [2 * nrows] f32.
 *   emoasr_ce_head_grad  dz[n, :] = s[n] * (exp(z[n, :] - lse[n]) - [v == ycol[n]]), s[n] = wrow[n] * gscale [* *gscale_dev], for
 *                        the nrows rows of one row chunk, z RECOMPUTED from x; coef: scratch [nrows, 4] f32.  The caller walks the
 *                        rows in chunks (dz chunk -> emoasr_gemm_nn / emoasr_gemm_tn), so at most one chunk of dz exists.
 *   emoasr_ce_head_sample_fwd  emoasr_ce_head_fwd that also draws, in the same epilogue, one Gumbel-max sample per row:
 *                        sample[n] = argmax_v (z32[n, v] + g(seed, row0 + n, v)), z32 the f32 accumulator + bias (not rounded to
 *                        bf16), g the variate of emoasr_gumbel_noise, ties to the lowest column -- a draw from softmax(z[n]).
 *                        part: scratch [ceil(V / 64), nrows, 4] f32; zscr: scratch [nrows] f32.  Same gates; (lse, ycol, wrow) feed
 *                        emoasr_ce_head_grad as after emoasr_ce_head_fwd. */
int emoasr_ce_head_fwd(int dtype, int nrows, int V, int K, const void* x, const void* w, const float* bias, const int* labels,
                       const float* wrow, float* part, float* zscr, int* ycol, float* lse, float* logp, float* loss, void* stream);
int emoasr_ce_head_sample_fwd(int dtype, int nrows, int V, int K, const void* x, const void* w, const float* bias, const int* labels,
                              const float* wrow, float* part, float* zscr, int* ycol, float* lse, float* logp, float* loss,
                              uint64_t seed, long row0, int* sample, void* stream);
int emoasr_ce_head_grad(int dtype, int nrows, int V, int K, const void* x, const void* w, const float* bias, const float* lse,
                        const int* ycol, const float* wrow, float gscale, const float* gscale_dev, float* coef, void* dz, long lddz,
                        void* stream);
/* out[m] = argmax_v x[m,:V] (first maximum) */
int emoasr_argmax_rows(int dtype, int M, int V, const void* x, long ldx, int* out, void* stream);
/* out[0] = first i < n with x[i] != value (-1: none), out[1] = x[that i] (value: none) -- the windowed greedy
 * transducer search (rnn_transducer.py:194-240) finds the next non-blank frame with one 8-byte D2H copy */
int emoasr_first_not_equal(int n, const int* x, int value, int* out, void* stream);

/* ---- greedy transducer search on the device (csrc/rnnt_greedy.hip; RNNTDecoder._greedy, rnn_transducer.py:194-240) --------------
 * ONE launch per utterance: 32 or 64 co-resident workgroups (64 when H is a multiple of 64 and V >= 64) run the whole time-synchronous
 * search.  Each owns a slice of every matrix (rows of the output and w_dec projections, the LSTM rows of its H / G hidden units), kept
 * in LDS; per step a [V x J] GEMV + arg-max, per emitted label two LSTM layers + a [J x H] GEMV.  The hidden state, the joint input and
 * the per-workgroup arg-max candidates travel between the workgroups as DATA-TAGGED 8-byte words (value + 12-bit step tag in one relaxed
 * store, readers poll for the tag): no grid barrier, no host round trip per label; a wait that gives up sets the error flag.
 * e_all [T, J] = w_enc . eouts + bias in the compute dtype; b_lstm0 / b_lstm1 = bias_ih + bias_hh [4H] of the two layers;
 * ws: emoasr_rnnt_greedy_ws_bytes(H, J) bytes (cleared by the call).
 * Outputs (device): hyp int32 [max_len + 1], align int32 [T + max_len + 1] (the arg-max of every joint evaluation, in order),
 * lens int32 [2] = {len(hyp), len(align)}.  emoasr_rnnt_greedy_status: 0 unless a wait of the last launch in `ws` gave up
 * (synchronises the stream).
 * emoasr_rnnt_greedy_supported (the MODEL): bf16 or f32, two LSTM layers, E / H / J multiples of 8, H a multiple of the G workgroups
 * with at most 16 hidden units per workgroup, E <= 1024, H <= 1024, J <= 1024, V >= G, J >= G.
 * emoasr_rnnt_greedy_fits (ONE utterance): _supported, and the workgroup's LDS image within 160 KB, T + max_len + 2 < 4095 (the step
 * tag), V < 2^20.  An utterance that does not fit takes the launch chain (engine.rnnt_greedy falls back per utterance). */
long emoasr_rnnt_greedy_fits(int dtype, int E, int H, int J, int V, int nl, int T, int max_len);
long emoasr_rnnt_greedy_supported(int dtype, int E, int H, int J, int V, int nl);
long emoasr_rnnt_greedy_ws_bytes(int H, int J);
int emoasr_rnnt_greedy(int dtype, int T, int E, int H, int J, int V, int blank, int eos, int max_len, const void* e_all,
                       const void* emb, const void* w_ih0, const void* w_hh0, const float* b_lstm0, const void* w_ih1,
                       const void* w_hh1, const float* b_lstm1, const void* w_dec, const float* b_dec, const void* w_out,
                       const float* b_out, void* ws, long ws_bytes, int* hyp, int* align, int* lens, void* stream);
long emoasr_rnnt_greedy_status(const void* ws, void* stream);

/* ---- one expansion round of the transducer beam search in five launches (csrc/rnnt_beam.hip; RNNTDecoder._beam_search,
 * rnn_transducer.py:242-325: the per-round recurrency + joint + log_softmax + topk of the reference's alignment-length-synchronous
 * search).  nb <= 16 live hypotheses; LSTM states live in slot-addressed pools ph [slots, H] (compute dtype) / pc [slots, H] (f32).
 * All index lists are int64 device arrays (the search's uploaded control words), so the launches can be captured into a graph.
 *   emoasr_rnnt_beam_lstm : one LSTM layer step: x_i = xtab[xidx[i]] (embedding rows by label id / the layer below's new h by slot),
 *                           (h, c) = pools[src[i]] -> gates = W_ih x + b + W_hh h -> new (h, c) written to pools[dst[i]];
 *                           bias = bias_ih + bias_hh [4H]; dst must not alias any src of the same round; the index lists may live
 *                           in pinned host memory (each word is read once); copy_dst != NULL: the launch also copies copy_n <= 192
 *                           int64 words copy_src -> copy_dst (the host-resident control record to its device twin)
 *   emoasr_rnnt_beam_joint: hj[i] = tanh(e_all[*t] + w_dec . ph[dst[i]] + b_dec)   (rnn_transducer.py:147-156 without the output layer)
 *   emoasr_rnnt_beam_pick : out[i] = { log_softmax(logits[i])[blank], the k best of log_softmax(logits[i])[1:] (descending, ties ->
 *                           lowest index), their indices relative to column 1 (as floats) }, out row stride ldo >= 1 + 2 k */
int emoasr_rnnt_beam_lstm(int dtype, int nb, int nin, int H, const void* xtab, long ldx, const long long* xidx, const void* w_ih,
                          const void* w_hh, const float* bias, void* ph, float* pc, const long long* src, const long long* dst,
                          const long long* copy_src, long long* copy_dst, int copy_n, void* stream);
int emoasr_rnnt_beam_joint(int dtype, int nb, int H, int J, int Tmax, const void* ph, const long long* dst, const void* w_dec,
                           const float* b_dec, const void* e_all, const long long* t, void* hj, void* stream);
int emoasr_rnnt_beam_pick(int dtype, int nb, int V, int k, int blank, const void* logits, long ldl, float* out, long ldo,
                          void* stream);

/* ---- batched transducer beam search with the bookkeeping on the device (csrc/rnnt_beam_book.hip, csrc/rnnt_beam.hip;
 * engine.rnnt_beam_search_batch): S searches of W <= 16 rows each, R = S W rows per launch, no host round trip between rounds.
 * Control words ctl: int64 [5][R], row s W + i: last label, source slot, destination slot, active flag, row of the search's current
 * frame in the stacked [sum of T, J] matrix w_enc . eouts + b.  row_off: int32 [S + 1], the frames before search s in that matrix.
 * Search s owns the slots s (E + 1) W .. (s + 1)(E + 1) W - 1 of the state pools (E = num_expands <= 15); slot s (E + 1) W must
 * hold the zero state when the search starts.
 *   emoasr_rnnt_beam_lstm_rows / _joint_rows: emoasr_rnnt_beam_lstm / _joint over R rows in tiles of 16 (one tile per blockIdx.y),
 *       row by row the same arithmetic.  A row whose active flag is 0 (or whose indices are outside nx / nslots) is a zero row of
 *       the staged image: it writes no pool slot and no row of hj.  hj is [R][J]; e_row (int64 [R]) names each row's row of e_all.
 *   emoasr_rnnt_beam_ws_bytes: the workspace of S searches over total_frames frames in all: S fixed states of
 *       EMOASR_RNNT_BEAM_STATE_BYTES, then 32 bytes per trie node, W total_frames (num_expands - 1) + S nodes.  -1 outside the limits.
 *   emoasr_rnnt_beam_start : every search at [(<sos> = eos)], score 0, slot 0, frame 0, round 0; writes the control words of round 0
 *   emoasr_rnnt_beam_book  : after the pick kernel of a round (rec: f32 [R][ldr], ldr >= 1 + 2 W, k = W): the round's bookkeeping
 *       (rnn_transducer.py:264-321, 348-359: blank extensions to the frame list, grown candidates, stable order by double score,
 *       merge of equal label sequences by log-add, cut to W; after round num_expands - 1 the same on the frame list, next frame)
 *       and the next round's control words.  A search whose frames are used up keeps its beams; its rows stay inactive.
 *   emoasr_rnnt_beam_finish: out_tok int32 [S][W][Lmax + 1], out_len [S][W], out_score f64 [S][W], out_n [S], best first, as
 *       emoasr_ctc_beam_batch writes them; hypotheses keep the leading <sos>.
 * Refusals (workspace short, a label outside 1 .. V - 1, offsets not rising, a hypothesis longer than Lmax + 1) are OR-ed into
 * *status (the bits of the CTC searches: 1 label, 2 offsets, 4 too long, 8 workspace, 32 no slot), the search stops and finish
 * gives out_n[s] = -1. */
#define EMOASR_RNNT_BEAM_MAX_WIDTH 16
#define EMOASR_RNNT_BEAM_MAX_EXPANDS 15
#define EMOASR_RNNT_BEAM_STATE_BYTES 8736
int emoasr_rnnt_beam_lstm_rows(int dtype, int R, int nin, int H, const void* xtab, long ldx, long nx, const long long* xidx,
                               const void* w_ih, const void* w_hh, const float* bias, void* ph, float* pc, long nslots,
                               const long long* src, const long long* dst, const long long* active, void* stream);
int emoasr_rnnt_beam_joint_rows(int dtype, int R, int H, int J, int e_rows, const void* ph, long nslots, const long long* dst,
                                const long long* active, const void* w_dec, const float* b_dec, const void* e_all,
                                const long long* e_row, void* hj, void* stream);
long emoasr_rnnt_beam_ws_bytes(int S, int total_frames, int W, int num_expands);
int emoasr_rnnt_beam_start(int S, int W, int num_expands, int V, int eos, const int* row_off, long long* ctl, void* ws,
                           long ws_bytes, int* status, void* stream);
int emoasr_rnnt_beam_book(int S, int W, int num_expands, int V, int eos, const int* row_off, const float* rec, long ldr,
                          long long* ctl, void* ws, long ws_bytes, int* status, void* stream);
int emoasr_rnnt_beam_finish(int S, int W, int num_expands, int V, int eos, const int* row_off, int Lmax, int* out_tok, int* out_len,
                            double* out_score, int* out_n, void* ws, long ws_bytes, int* status, void* stream);

/* ---- batched transducer GREEDY search in lockstep, the bookkeeping on the device (csrc/rnnt_greedy_batch.hip;
 * engine.rnnt_greedy_batch, rnn_transducer.py:194-240): S searches, each step scores up to K consecutive frames of every live search
 * against its current decoder state (S K joint rows), no host round trip between steps.
 * Control words ctl: int64 [4 S + 3 S K]: [4][S] for emoasr_rnnt_beam_lstm_rows (label, source slot, destination slot, active), then
 * [3][S K] for emoasr_rnnt_beam_joint_rows (slot to read, active, row of the stacked [sum of T, J] matrix w_enc . eouts + b); an
 * inactive row's words are zero.  Search s owns the slots 2 s and 2 s + 1 of the state pools; slot 2 s must hold the zero state
 * when the search starts.  row_off: int32 [S + 1] as for the beam search.  state: int32 [S][4] (frame, current slot, finished, -).
 *   emoasr_rnnt_greedy_batch_start: every search with frames consumes <eos> from slot 2 s into slot 2 s + 1 and points its rows at
 *       the frames 0 .. K - 1 (rows past its last frame inactive); a search without frames is finished; *live = the others
 *   emoasr_rnnt_greedy_batch_book : after the output product of a step (logits [S K][ldl] of the compute dtype): per search the
 *       arg-max of every active row (the first maximum, as emoasr_argmax_rows), then the reference's rule -- first non-blank row k:
 *       k blanks and the token to the alignment, the token to the hypothesis, frame += k, one LSTM step into the other slot; all
 *       blank: the blanks, frame += active rows -- and the next step's words.  A search finishes at its last frame or once its
 *       hypothesis is longer than max_len (max_len + 1 labels are kept); it then leaves its rows inactive and *live falls by one.
 *       hyp int32 [S][ldh >= max_len + 1], align int32 [S][lda >= longest T + max_len + 1], lens int32 [S][2] = {len(hyp), len(align)}. */
#define EMOASR_RNNT_GREEDY_BATCH_MAX_FRAMES 16
int emoasr_rnnt_greedy_batch_start(int S, int K, int eos, int max_len, const int* row_off, long long* ctl, int* state, int* lens,
                                   int* live, void* stream);
int emoasr_rnnt_greedy_batch_book(int dtype, int S, int K, int V, int blank, int max_len, const int* row_off, const void* logits,
                                  long ldl, long long* ctl, int* state, int* hyp, long ldh, int* align, long lda, int* lens, int* live,
                                  void* stream);

/* ---- RNN-LM shallow fusion inside the batched transducer search (csrc/rnnt_beam_lm.hip; engine.rnnt_beam_search_batch with lm=).
 * The LM's LSTM states live in pools beside ph / pc under the same slot numbers and are stepped by emoasr_rnnt_beam_lstm_rows under
 * the same control words; these two entry points are what a fused round adds.
 *   emoasr_rnnt_beam_gather_rows: out[r] = pool[dst[r]] (H values of the compute dtype) for an active row with 0 <= dst[r] < nslots,
 *       a zero row otherwise (active == NULL: every row is active).  out is [R][H].
 *   emoasr_rnnt_beam_pick_lm    : emoasr_rnnt_beam_pick with f[v] = lp[v] + mu * lq[v] in place of lp[v] for the candidates v in
 *       1 .. V - 1: lp = log_softmax(logits[r, :V]), lq = log_softmax(lm_logits[r, :V_lm])[:V], V_lm >= V, mu = mu[r / W] (one f32 per
 *       search), the product and the sum rounded to f32 separately.  out[r] = { lp[blank], the k best f (descending, ties -> lowest
 *       index), their indices relative to column 1 as floats }, ldo >= 1 + 2 k, k < V.  mu = 0 gives emoasr_rnnt_beam_pick's record
 *       bit for bit.  A row with active[r] == 0 writes nothing (active == NULL: every row is active).  Both logit matrices are of the
 *       compute dtype. */
int emoasr_rnnt_beam_pick_lm(int dtype, int R, int V, int V_lm, int k, int blank, int W, const void* logits, long ldl,
                             const void* lm_logits, long ldlm, const float* mu, const long long* active, float* out, long ldo,
                             void* stream);
int emoasr_rnnt_beam_gather_rows(int dtype, int R, int H, const void* pool, long nslots, const long long* dst,
                                 const long long* active, void* out, void* stream);

/* ---- one step of the RNN LM for the hypotheses of a beam search (csrc/rnnlm.hip; lm/modeling/rnn.py:62-81, RNNLM.predict): L + 2
 * launches -- one per LSTM layer, emoasr_gemm_nt for the vocabulary head, a log-softmax.  1 <= nb <= 32 rows.  Row i reads the
 * embedding of ids[i] (int32), the state (h, c) of every layer from the slot pools ph [L][slots][H] (compute dtype) / pc
 * [L][slots][H] (f32) at src[i] (src[i] < 0: the zero state) and writes the new state at dst[i]; several rows may share one src, no
 * dst may equal any src of the same call.  log_softmax(output(h_top)) of row i goes to logp[row_dst[i]] (f32, row stride ldlogp,
 * logp_rows rows; row_dst NULL: row i).  ids / src / dst / row_dst are int32 DEVICE arrays (the call can be captured into a graph);
 * w_ih / w_hh / bias are HOST arrays of L device pointers ([4H][E or H], [4H][H], f32 [4H] = bias_ih + bias_hh); ws:
 * emoasr_rnnlm_step_ws_bytes(dtype, H, V) bytes.  Rounding as the sequence forward: f32 accumulation, h in the compute dtype, c in
 * f32.  EMO_F32X3 runs the f32 kernels (the head's product is split).  emoasr_rnnlm_step_supported() -> 1 if the shape is inside
 * the kernel's plan (bf16: E, H % 8 == 0; f32: % 4; H % 8 == 0; the LDS image of the rows fits). */
int emoasr_rnnlm_step_supported(int dtype, int nb, int L, int E, int H);
long emoasr_rnnlm_step_ws_bytes(int dtype, int H, int V);
int emoasr_rnnlm_step(int dtype, int nb, int L, int E, int H, int V, int slots, const int* ids, const void* emb,
                      const void* const* w_ih, const void* const* w_hh, const float* const* bias, void* ph, float* pc,
                      const int* src, const int* dst, const void* w_out, const float* b_out, float* logp, long ldlogp,
                      int logp_rows, const int* row_dst, void* ws, long ws_bytes, void* stream);
/* The same step for any R >= 1 rows in ONE call (L layer launches with the tiles of 32 rows on blockIdx.y, one emoasr_gemm_nt), addressed
 * by the arrays of the batched joint search: row r reads the embedding of ids[r], the state at slot src_base +
 * parent[r] (parent: GLOBAL rows, as emoasr_beam_update_batch writes n_parent; a parent outside 0 .. R - 1: the zero state) and writes
 * the new state at slot dst_base + r.  The R source slots and the R destination slots lie inside the pools and do not overlap (the
 * two halves of a double-buffered pool: src_base / dst_base in {0, R}, slots = 2 R).  Every row gets the bits emoasr_rnnlm_step
 * gives it.  The RAW f32 logits output(h_top) + b_out go to logits [R][ldl] (no log-softmax: emoasr_beam_scores_topk forms it); ws:
 * emoasr_rnnlm_step_rows_ws_bytes(dtype, R, H) bytes.  ids / parent are int32 DEVICE arrays [R], the weight tables HOST arrays of L
 * device pointers; the call can be captured into a graph.  emoasr_rnnlm_step_rows_supported: emoasr_rnnlm_step_supported at 32 rows. */
typedef struct emoasr_rnnlm_rows {
  int L, E, H, V, R;
  const void* emb;                               /* [V][E] */
  const void* const* w_ih; const void* const* w_hh; const float* const* bias;
  const void* w_out; const float* b_out;         /* [V][H], f32 [V] */
  void* ph; float* pc; int slots, src_base, dst_base;
  float* logits; long ldl;
  void* ws; long ws_bytes;
} emoasr_rnnlm_rows_t;
int emoasr_rnnlm_step_rows_supported(int dtype, int L, int E, int H);
long emoasr_rnnlm_step_rows_ws_bytes(int dtype, int R, int H);
int emoasr_rnnlm_step_rows(int dtype, const emoasr_rnnlm_rows_t* rl, const int* ids, const int* parent, void* stream);

/* ---- LAS decoder: location-aware additive attention, one decoder position (decoders/las.py:289-342; csrc/las.hip) ----
 *   f[t][c] = Conv1d(1, 10, 201, padding 100, no bias)(aw_prev)[c][t]
 *   e[t]    = w_score . tanh(pk[t] + pq + W_conv f[t] + b_conv)      t >= elens[b]: -FLT_MAX (elens NULL: no mask)
 *   aw      = softmax_t(e);  awd[t] = aw[t] * keep(seed, step, b, t) / (1 - drop_p);  ctx = sum_t awd[t] eouts[t]
 * pk = W_key eouts + b_key [B,T,A] and pq = W_query q + b_query [B,A] arrive from the GEMMs (compute dtype T); score.w_score.bias
 * shifts every e[t] alike and never enters.  The weights stay f32; keep() is the counter-based mask of common.h at element
 * (step * B + b) * T + t, derived alike by the forward, the backward and emoasr_las_dropmask (uint8 [B,T], 1 = kept) -- never stored.
 * A % 8 == 0, A <= 512, D % 8 == 0; B, T free.  pk_bstride / eo_bstride: elements between rows' [T,A] / [T,D] blocks (0: every
 * row reads the same utterance -- the beam search's hypotheses).
 * forward (2 launches): reads pk, pq, aw_prev (NULL: zeros, position 0), filt, w_conv, b_conv, w_score, eouts, elens; writes
 *   scores (scratch f32 [B,T]), aw (the DROPPED weights f32 [B,T]), lse (f32 [B], NULL: not wanted), ctx (T, rows of stride ctx_ld).
 * backward (1 launch): reads the above with aw / ctx / lse as the forward left them, dctx (T, row stride dctx_ld) and daw (f32 [B,T]
 *   the gradient arriving at aw from the next position's convolution, NULL: none); ACCUMULATES into dpq f32 [B,A], daw_prev f32
 *   [B,T] (NULL at position 0), dpk f32 [B,T,A], deouts f32 [B,T,D] (NULL: skipped), dw_score [A], dw_conv [A,10], db_conv [A],
 *   dfilt [10,201] (all f32; f32 atomics where tiles or rows meet, so the caller zero-fills what it has not accumulated into). */
#define EMOASR_LAS_CONV_CHANNELS 10
#define EMOASR_LAS_CONV_WIDTH 201
typedef struct {
  int B, T, A, D;
  const void* pk; long pk_bstride;
  const void* pq;
  const float* aw_prev;
  const float *filt, *w_conv, *b_conv, *w_score;
  const void* eouts; long eo_bstride;
  const int* elens;
  float drop_p; uint64_t seed; int step;
  float *scores, *aw, *lse;
  void* ctx; long ctx_ld;
  const void* dctx; long dctx_ld;
  const float* daw;
  float *dpq, *daw_prev, *dpk, *deouts, *dw_score, *dw_conv, *db_conv, *dfilt;
} emoasr_las_attend_t;
int emoasr_las_attend_fwd(int dtype, const emoasr_las_attend_t* a, void* stream);
int emoasr_las_attend_bwd(int dtype, const emoasr_las_attend_t* a, void* stream);
int emoasr_las_dropmask(const emoasr_las_attend_t* a, unsigned char* mask, void* stream);

/* ---- masked LM: the masked copies of the pseudo-log-likelihood (lm/modeling/bert.py:54-86) ----
 * ys int32 [B,N] with lengths ylens has R = sum(ylens) masked copies; copy r belongs to the sequence b with
 * row0[b] <= r < row0[b+1] (row0 int32 [B+1]: prefix sums of ylens) and masks pos = r - row0[b].  For j < r_count, r = r_begin + j:
 *   ids[j,:] = ys[b,:ylens[b]] with [pos] = mask_id, then pad_id up to Np;  klens[j] = ylens[b];
 *   idx[j] = j*Np + pos (the flat row to gather);  labels[j] = ys[b,pos].
 * One wave per output row, nothing is written outside the r_count rows; every pointer is device memory. */
int emoasr_mlm_expand(int B, int N, int Np, const int* ys, const int* ylens, const int* row0, int r_begin, int r_count,
                      int mask_id, int pad_id, int* ids, int* klens, int* idx, int* labels, void* stream);

/* ---- ELECTRA (lm/modeling/electra.py:20-132): generator sampling, corruption, the discriminator's binary head ----
 * emoasr_sample_rows: logits [M,V] (row stride ld >= V, any V >= 2), one 256-thread block per row, ONE pass over the row:
 *   lse[m] (may be NULL) = log sum_v exp z[m,v];  loss[m] = -w[m] * (z[m,labels[m]] - lse[m]) (0 for w[m] == 0);
 *   sample[m] = argmax_v (f32(z[m,v]) + g(seed, row0 + m, v)), ties to the lowest column: a draw from softmax(z[m]).
 *   g = -log(-log(u)), u = (k + 0.5) * 2^-24, k = the 24-bit counter hash of (seed, (row0 + m) * V + v) -- a function of the seed
 *   and the element alone, so a caller that walks M in chunks (row0) draws the same samples.
 * emoasr_gumbel_noise: out[m,v] (f32, row stride ldo) = that g, from the same device function (tests; not on the training path). */
int emoasr_sample_rows(int dtype, int M, int V, const void* logits, long ld, const int* labels, const float* w, uint64_t seed,
                       long row0, float* loss, float* lse, int* sample, void* stream);
int emoasr_gumbel_noise(int M, int V, uint64_t seed, long row0, float* out, long ldo, void* stream);
/* generated[BN] = ids with samples[m] at the flat rows sel[m] (m < M, each row named once); replaced[BN] (f32 0 / 1) =
 * generated != (ids with labels[m] at sel[m]);  counters[0] = number replaced, counters[1] = number masked (= M).  M == 0 copies the
 * ids and zeroes the rest.  Nothing is written outside [0, BN). */
int emoasr_electra_corrupt(int BN, int M, const int* ids, const int* sel, const int* labels, const int* samples, int* generated,
                           float* replaced, int* counters, void* stream);
/* discriminator_predictions.dense_prediction + BCEWithLogits rows over h [M,H] (the GELU output of .dense):
 *   z[m] = h[m,:] . wp + bp[0];  loss[m] (may be NULL) = w[m] * (max(z,0) - z*y[m] + log1p(exp(-|z|)));  sig[m] (may be NULL) = sigmoid(z)
 * backward: dz = w * (sigmoid(z) - y) * gscale * [gscale_dev];  dh[m,:] = dz[m] * wp;  dwp += sum_m dz[m] h[m,:];  dbp += sum_m dz[m]
 * (f32 atomics into the gradient slots, one per column and block of 64 rows). */
int emoasr_bce_head_fwd(int dtype, int M, int H, const void* h, long ldh, const void* wp, const float* bp, const float* y,
                        const float* w, float* z, float* loss, float* sig, void* stream);
int emoasr_bce_head_bwd(int dtype, int M, int H, const void* h, long ldh, const void* wp, const float* z, const float* y,
                        const float* w, float gscale, const float* gscale_dev, void* dh, long lddh, float* dwp, float* dbp,
                        void* stream);

/* ---- CTC error correction (asr/test_asr_correct.py:39-172): token confidences and the recogniser / LM fusion ----
 * emoasr_ctc_token_conf: logits [B,T,V] (row stride ld >= V, utterance stride T * ld), lse f32 [B*T] their row log-sum-exps, best
 *   int32 [B,T] the greedy frame ids.  A token of utterance b is a maximal run of equal non-blank frames below min(elens[b], T)
 *   (the CTC collapse: token j is hyp[b,j] of emoasr_ctc_greedy).  For token j:
 *     frame[b,j] = the frame t of the run with the largest exp(logits[b,t,id] - lse[b,t]) (f32), the earliest on ties;
 *     conf[b,j]  = that value;   ntok[b] = number of tokens.   frame / conf are [B,T]; entries from ntok[b] on are left alone.
 *   One wave per utterance; frames at or past elens[b] are never read; an id outside [0, V) counts as blank.
 * emoasr_correct_fuse: for row i < n: a = asr[asr_rows[i]] (asr_rows int32 [n], NULL: row i; clamped to [0, asr_nrows)), with its
 *   log-sum-exp asr_lse[that row]; l = lm[i] (its log-sum-exp over all V_lm columns is formed in the kernel);
 *     out_id[i] = argmax_{v < n_cols} (1 - w) exp(a[v] - lse_a) + w exp(l[v] - lse_l), lowest v on ties;  out_val[i] = that maximum.
 *   n_cols <= min(V_asr, V_lm); 0 <= w <= 1; the two dtypes are independent (EMO_F32 / EMO_BF16).  One 256-thread block per row,
 *   f32 accumulation, 16-byte loads on 16-byte aligned rows (element loads for the ragged end and for unaligned rows). */
int emoasr_ctc_token_conf(int dtype, int B, int T, int V, const void* logits, long ld, const float* lse, const int* best,
                          const int* elens, int blank, int* frame, float* conf, int* ntok, void* stream);
int emoasr_correct_fuse(int dtype_asr, int dtype_lm, int n, int V_asr, int V_lm, int n_cols, const void* asr, long ld_asr,
                        const float* asr_lse, const int* asr_rows, long asr_nrows, const void* lm, long ld_lm, float w,
                        int* out_id, float* out_val, void* stream);
/* The grid of thresholds and weights (one recogniser pass, one LM pass per threshold, one fuse launch for all weights).
 * emoasr_correct_mask_grid: hyp int32 [B,T] the collapsed greedy ids; ntok [B], conf [B,T], frame [B,T] as emoasr_ctc_token_conf
 *   leaves them; ths f32 [NT] on the device.  For threshold k and utterance b (the pair k * B + b):
 *     ys[k,b,j]        = mask_id where j < ntok[b] and conf[b,j] < ths[k] (strictly), hyp[b,j] for the other j < ntok[b], pad_id from
 *                        ntok[b] on (ys int32 [NT,B,T]: Lmax = T);
 *     num_masked[k,b]  = the number of masked tokens of the pair (int32 [NT,B]);
 *     lm_rows, asr_rows (int32, room for NT * B * T entries; sum(num_masked) are written): the masked positions in (threshold,
 *                        utterance, token) order; lm_rows[i] = (k * B + b) * T + j is the position's row of ys viewed flat, so it
 *                        names (k, b, j) as well; asr_rows[i] = b * T + frame[b,j] its recogniser row.
 *   A pair's place in the lists is the sum of the counts before it (a scan, no atomics): the lists are a fixed function of the
 *   inputs.  ntok[b] is clamped to [0, T]; NT * B * T <= 2^31 - 1.  One wave per pair, two launches.
 * emoasr_correct_fuse_grid: emoasr_correct_fuse for the NW weights `weights` (f32 [NW] on the HOST, each in [0, 1]; 1 <= NW <=
 *   EMO_CORRECT_MAX_WEIGHTS per launch): out_id / out_val are [NW, n], row k what emoasr_correct_fuse gives for w = weights[k], bit
 *   for bit.  Both rows are read once: exp(a[v] - lse_a) and exp(l[v] - lse_l) are formed once per column, every weight keeps its
 *   own running (value, column).  Same dtypes, strides and alignment rules as emoasr_correct_fuse. */
#define EMO_CORRECT_MAX_WEIGHTS 16
int emoasr_correct_mask_grid(int B, int T, int NT, const int* hyp, const int* ntok, const float* conf, const int* frame,
                             const float* ths, int mask_id, int pad_id, int* ys, int* num_masked, int* lm_rows, int* asr_rows,
                             void* stream);
int emoasr_correct_fuse_grid(int dtype_asr, int dtype_lm, int n, int V_asr, int V_lm, int n_cols, const void* asr, long ld_asr,
                             const float* asr_lse, const int* asr_rows, long asr_nrows, const void* lm, long ld_lm,
                             const float* weights, int NW, int* out_id, float* out_val, void* stream);

/* ---- N-best rescoring and error-label alignment (asr/rescore/test_rescore_grid.py, asr/rescore/align_hyps.py) ----
 * emoasr_edit_align: P pairs of int32 token sequences.  Hypothesis p is hyp[hyp_off[p] .. hyp_off[p+1]); its reference is sequence
 *   r = ref_idx[p] (NULL: r = p) of the n_ref references, ref[ref_off[r] .. ref_off[r+1]), so the hypotheses of one utterance share
 *   one reference.  Per pair, exactly compute_wer of asr/metrics.py:20-105: an empty hypothesis is one token that matches nothing;
 *   the backtrace from (R, H) takes C when the tokens match, else I when d == left + 1, else S when d == diag + 1, else D; row 0
 *   gives I, column 0 gives D.
 *     counts[p] int32 [4]        = (n_sub, n_ins, n_del, dist)
 *     ops (may be NULL)          uint8 'C' / 'S' / 'I' / 'D' in sequence order from ops[ops_off[p]]: max(H, 1) + n_del of them;
 *                                the caller leaves R + max(H, 1) slots per pair (ops_off int64 [P])
 *     labels (label_mode != NONE) uint8, one per hypothesis token at labels[hyp_off[p] + j] (nothing for an empty hypothesis):
 *       EMOASR_ALIGN_SI   the ops without the deletions;
 *       EMOASR_ALIGN_SID  align_hyps.py:43-55 as it runs: a deletion with no label before it, or after a label other than C,
 *                         turns the next C into D; a deletion after a C is dropped.
 *   max_hyp_len / max_ref_len are the caller's bounds on the lengths; one over EMOASR_EDIT_MAX_LEN is an error return.  The
 *   direction codes of a pair (2 bits per cell) live in LDS up to EMOASR_EDIT_LDS_WORDS 64-bit words; a larger pair keeps them in
 *   ws[ws_off[p] .. ws_off[p+1]) (ws 64-bit words, ws_off int64 [P+1]), emoasr_edit_align_ws_words(R, H) words of it (0: LDS; -1:
 *   over the limit).  A pair that breaks the declared bounds, its offsets or its workspace is not computed: its counts are -1 and
 *   bit 0 of status[0] (int32, zeroed by the caller) is set.  One wave per pair; nothing is written outside the outputs.
 * emoasr_rescore_grid: rows k of utterance u are utt_off[u] .. utt_off[u+1]-1 (N rows, U utterances).  For cell g = a * G2 + b:
 *     best[g][u]  = the first row of u with the largest (score_asr[k] + lm_w[a] * score_lm[k]) + len_w[b] * ylen[k], every product
 *                   and sum rounded once to f64 (no fused multiply-add); -1 for an utterance without rows.  Scores are finite.
 *     totals[g]   int64 [3] = (n_sub, n_ins, n_del) of counts [N][4] summed over the winners.  G1 * G2 <= 65535. */
#define EMOASR_EDIT_MAX_LEN 4096
#define EMOASR_EDIT_LDS_WORDS 4096
enum { EMOASR_ALIGN_NONE = 0, EMOASR_ALIGN_SI = 1, EMOASR_ALIGN_SID = 2 };
long emoasr_edit_align_lds_words(void);   /* EMOASR_EDIT_LDS_WORDS, for callers that size workspaces without this header */
long emoasr_edit_align_ws_words(int ref_len, int hyp_len);
int emoasr_edit_align(int P, int n_ref, int max_hyp_len, int max_ref_len, const int* hyp, const int* hyp_off, const int* ref,
                      const int* ref_off, const int* ref_idx, int label_mode, int* counts, unsigned char* ops,
                      const long* ops_off, unsigned char* labels, void* ws, const long* ws_off, int* status, void* stream);
int emoasr_rescore_grid(int N, int U, int G1, int G2, const double* score_asr, const double* score_lm, const int* ylen,
                        const int* utt_off, const int* counts, const double* lm_w, const double* len_w, int* best,
                        long long* totals, void* stream);

/* ---- one Conformer encoder layer, forward, sequenced on the host in C++ ---------
 * ConformerEncoderLayer.forward (asr/modeling/conformer.py:146-225) with relative-position attention:
 *   x += 0.5 * drop(FFN_macaron(LN(x)));  x += drop(RelMHA(LN(x)));  x += drop(ConvModule(LN(x)));
 *   x += 0.5 * drop(FFN(LN(x)));  y = LN(x)
 * as ONE call that enqueues the ~24 kernels above on `stream` (the caller pays one FFI crossing per
 * layer instead of one per kernel).  Every intermediate the backward needs is written to
 * caller-provided buffers (emoasr_conformer_fwd_t); mean / rstd / u pointers may be NULL for inference.
 * Weights (w*, pw*, wqkv [3d,d], wpos, wout) are in the compute dtype, everything else f32.
 * seed[] = {ffm_in, ffm_out, att_probs, att_out, conv_out, ff_in, ff_out} dropout streams. */
typedef struct emoasr_ffn_params {
  const float *ln_g, *ln_b;
  const void* w1; const float* b1;   /* [F,d], [F] */
  const void* w2; const float* b2;   /* [d,F], [d] */
} emoasr_ffn_params_t;
typedef struct emoasr_conformer_layer {
  int d, H, F, K;                    /* model dim, heads, FFN inner dim, depthwise kernel size */
  emoasr_ffn_params_t ffm, ff;
  const float *att_ln_g, *att_ln_b;
  const void* wqkv; const float* bqkv;
  const void* wpos;
  const float *bias_u, *bias_v;
  const void* wout; const float* bout;
  const float *cv_ln_g, *cv_ln_b;
  const void* pw1; const float* pw1_b;   /* [2d,d] */
  const float *dw_w, *dw_b;              /* [d,K], [d] */
  const float *bn_g, *bn_b;
  float *bn_rm, *bn_rv; long long* bn_nbt;
  const void* pw2; const float* pw2_b;
  const float *fin_ln_g, *fin_ln_b;
  /* optional (bf16 backward, NULL = absent): TRANSPOSED copies of the weights whose data-gradient products are long reductions
   * onto one 256-column tile -- ffm / ff w1 as [d,F], wqkv as [d,3d], pw1 as [d,2d] (emoasr_transpose_cast_batched keeps them
   * current).  dX = dY . W is then the NT product dY . (W^T)^T, which the large-tile kernel takes (csrc/gemm_big.hip). */
  const void *ffm_w1t, *ff_w1t, *wqkv_t, *pw1_t;
  /* likewise optional (round 5): transposed copies of the K = d products' weights -- ffm / ff w2 as [F,d], wout and pw2 as [d,d] --
   * so that their data gradients run as NT products too (the k-major B tile of the NN form is read with transposing LDS loads) */
  const void *ffm_w2t, *ff_w2t, *wout_t, *pw2_t;
} emoasr_conformer_layer_t;
typedef struct emoasr_ffn_stash {
  void *h, *u, *a, *y;               /* LN out [M,d], pre-activation [M,F] (optional), activation [M,F], block output [M,d] */
  float *mean, *rstd;
} emoasr_ffn_stash_t;
/* Stacked micro-batches ("segments"): the reference accumulates gradients over `accum_grad` independent forward /
 * backward passes (asr/train_asr.py:106-128).  Here up to EMOASR_MAX_SEGMENTS of those micro-batches go through a layer
 * TOGETHER: their rows are concatenated (segment s = B[s] utterances padded to T[s] frames; M = sum B[s] T[s] rows), so every
 * row-wise kernel -- the projections, LayerNorms, the vocabulary head -- runs once over all of them, while attention stays per
 * utterance, the depthwise convolution sees each segment's own zero padding and BatchNorm takes its batch statistics PER
 * SEGMENT and updates the running statistics once per segment, in order -- the arithmetic of the separate passes.
 * n = 0 (or 1 with B[0], T[0]): one dense batch. */
typedef struct emoasr_segments {
  int n;
  int B[EMOASR_MAX_SEGMENTS], T[EMOASR_MAX_SEGMENTS];
} emoasr_segments_t;
typedef struct emoasr_conformer_fwd {
  int B, T;                          /* dense batch; with seg.n > 1: B = sum seg.B, T = max seg.T (informative) */
  const void* x;                     /* [M, d], M = B*T or the stacked row count */
  const void* pos_t;                 /* [2T-1, d] relative position table (after dropout), compute dtype; stacked: the
                                      * segments' tables one after the other, sum (2 T[s] - 1) rows */
  const int* klens;                  /* int32 [B] valid frames (stacked: all segments' utterances in order) */
  int training;                      /* batch statistics + running-stat update in BatchNorm */
  float p_enc, p_att;
  uint64_t seed[7];
  emoasr_ffn_stash_t ffm, ff;
  void *at_h, *qkv, *pp, *o, *at_y; float *lse, *at_mean, *at_rstd;
  void *cv_h, *g, *gl, *c, *z, *cv_y; float *bmean, *bvar, *bn_part, *cv_mean, *cv_rstd;
  void* y; float *fin_mean, *fin_rstd;
  emoasr_segments_t seg;             /* stacked micro-batches; lse is [H * M]: segment s at H * (its first row), laid out
                                      * [B[s], H, T[s]]; bmean / bvar are [n, d]; bn_part holds the segments' partial-sum
                                      * areas (emoasr_dwconv_stats_floats(B[s], T[s], d) floats each) back to back */
  /* optional (bf16 training with attention dropout): room for the layer's attention keep mask as bits, uint32
   * [M, H, att_mask_nw] with att_mask_nw >= emoasr_attn_dropmask_words(longest T).  The forward hashes the mask once (on the
   * attention's side stream, under the macaron feed-forward block) and the attention forward and both backward passes test bits
   * (emoasr_attn_t::keep_mask); it is part of the stash the backward takes.  NULL: every kernel hashes for itself. */
  unsigned* att_mask; int att_mask_nw;
  int att_mask_ready;                /* 1: att_mask already holds (or is being filled on the attention's side stream with) this layer's
                                      * bits -- emoasr_conformer_attn_masks hashed all layers' masks at the start of the pass */
} emoasr_conformer_fwd_t;
/* The attention keep masks of ALL nl layers of an encoder pass, hashed up front on the attention's side stream (forked from
 * `stream` here): called before the convolution front-end, the ~0.05 ms of integer hashing per layer run under its MFMA-bound
 * products instead of beside each layer's memory-bound kernels.  seeds[l] = the layer's att_probs dropout stream (seed[2] of its
 * emoasr_conformer_fwd_t); masks + l * layer_stride_words = its att_mask [M, H, nw]. */
int emoasr_conformer_attn_masks(int dtype, int nl, const emoasr_segments_t* seg, int B, int T, int H, int d, const int* klens,
                                float p_att, const uint64_t* seeds, unsigned* masks, long layer_stride_words, int nw, void* stream);
int emoasr_conformer_layer_fwd(int dtype, const emoasr_conformer_layer_t* layer,
                               const emoasr_conformer_fwd_t* io, void* stream);
/* Backward of the same layer (training-mode forward with stash) as one call: gradient kernels in the order the
 * reference's autograd runs them (conformer.py:146-225 backwards), the layer's nine weight-gradient products as one grouped
 * launch.  `grads`: the layer struct again with every parameter pointer replaced by the address of its f32 gradient
 * (accumulated into; d/H/F/K and the running-statistics fields are ignored).  `st`: the emoasr_conformer_fwd_t the forward
 * call was given (its buffers still intact).  dy / dx: gradient w.r.t. the layer's output / input, [B*T, d].
 * ws: emoasr_conformer_layer_bwd_ws_bytes(...) bytes, no initialisation, reusable by the next layer's call.
 * ln_part: 5 areas of emoasr_layernorm_bwd_scratch_floats(d) floats, ln_part_stride floats apart, that receive the
 * dgamma / dbeta partial sums of the layer's LayerNorms (order: final, feed-forward, convolution, attention, macaron);
 * the caller folds them with emoasr_layernorm_bwd_finalize (one launch for the whole backward sweep). */
typedef struct emoasr_conformer_bwd {
  const void* dy;
  void* dx;
  void* ws; size_t ws_bytes;
  float* ln_part; long ln_part_stride;
  /* f32 only (the attention backward of f32 layers is the materialised emoasr_attn_bwd, one call per stacked micro-batch):
   * emoasr_conformer_layer_bwd_img_bytes_seg(...) bytes holding every micro-batch's P^T / dS^T / dBD images, ZERO-filled by the
   * caller once per backward sweep (the masks of a sweep are the same in every layer) and passed to every layer's call. */
  void* attn_img; size_t attn_img_bytes;
} emoasr_conformer_bwd_t;
size_t emoasr_conformer_layer_bwd_ws_bytes(int dtype, int B, int T, int d, int H, int F, int K);
/* The convolution module's per-utterance part for stacked micro-batches, every kernel taking ALL segments in one launch (bf16;
 * csrc/convfused.hip).  Same arithmetic as emoasr_glu_dwconv_fwd + emoasr_bn_stats_finalize + emoasr_bn_swish_fwd (forward) and
 * emoasr_bn_swish_bwd_sums + emoasr_conv_bwd_fused (backward) called once per segment, in order: the depthwise convolution sees each
 * segment's own zero padding, BatchNorm takes its batch statistics per segment (bmean / bvar [n, C]) and moves the running
 * statistics once per segment, each update bit for bit the one of emoasr_bn_stats_finalize on that segment.  g / dg [M, 2C],
 * c / z / dz [M, C]; part: the segments' emoasr_dwconv_stats_floats areas back to back -- scratch: with more than one segment the
 * merge CONSUMES it (it leaves every segment's centred sum of squares in the first C floats of the segment's area; the dense
 * emoasr_bn_stats_finalize leaves `part` as it found it);
 * scratch sizes from emoasr_conv_module_bwd_seg_scratch_floats (which = 0: BatchNorm sums, 1: depthwise weight-gradient partials).
 * Reference: conformer.py:126-133 and its autograd. */
int emoasr_conv_module_fwd_seg(int dtype, const emoasr_segments_t* seg, int C, int K, const void* g, const float* w,
                               const float* bias, void* c, float* part, float* bmean, float* bvar, float* running_mean,
                               float* running_var, float momentum, long long* num_batches_tracked, const float* gamma,
                               const float* beta, float eps, void* z, int training, void* stream);
long emoasr_conv_module_bwd_seg_scratch_floats(const emoasr_segments_t* seg, int C, int K, int which);
int emoasr_conv_module_bwd_seg(int dtype, const emoasr_segments_t* seg, int C, int K, const void* dz, const void* c,
                               const float* bmean, const float* bvar, const float* gamma, const float* beta, float eps,
                               float* dgamma, float* dbeta, const void* g, const float* w, void* dg, float* dw, float* dbias,
                               float* bn_scratch, float* dw_scratch, void* stream);
size_t emoasr_conformer_layer_bwd_ws_bytes_seg(int dtype, const emoasr_segments_t* seg, int d, int H, int F, int K);
/* emoasr_set_option("wgrad_side", 1): emoasr_conformer_layer_bwd puts its grouped weight-gradient launch on a side stream (one
 * per (device, caller stream)) where it runs under the NEXT layer's gradient chain.  The launch reads the call's workspace: callers
 * then alternate between TWO workspaces from call to call (a call waits for the launch issued two calls earlier before it touches
 * its workspace) and call emoasr_wgrad_side_join(keep, stream) before anything reads the weight gradients or frees a workspace:
 * the caller's stream waits for the launches in flight -- all of them (keep = 0) or all but the latest (keep = 1: the gradients of
 * every layer but the one just finished are final; for a per-layer gradient hook one layer behind the sweep).  Captured streams run
 * the launch inline. */
int emoasr_wgrad_side_join(int keep, void* stream);
size_t emoasr_conformer_layer_bwd_img_bytes_seg(int dtype, const emoasr_segments_t* seg, int d, int H);   /* 0 for bf16 */
int emoasr_conformer_layer_bwd(int dtype, const emoasr_conformer_layer_t* layer, const emoasr_conformer_layer_t* grads,
                               const emoasr_conformer_fwd_t* st, const emoasr_conformer_bwd_t* io, void* stream);

/* ---- beam-search step runtime (inference): the Transformer decoder over the whole prefix and the
 * Transformer LM's next-token distribution, each as ONE call per output step ---------------------------
 * emoasr_transformer_decoder_infer: TransformerDecoder.forward_one_step (decoders/transformer.py:148-159;
 * layers: transformer.py:156-198, eps 1e-12, ReLU FFN) for nb live hypotheses of L tokens each.  Like the
 * reference it recomputes the prefix (no self-attention cache); unlike it, the cross-attention keys / values
 * of the encoder memory are projected once per utterance (kv[l]: [nb,T,2*dd], K then V) and only the LAST
 * position goes through the output projection: logits_last [nb,V].
 * emoasr_bert_lm_infer: TransformerLM.predict (lm/modeling/transformer.py:62-77 over the BERT-style stack,
 * modeling_bert.py:159-303,360-436): log-softmax of the next-token logits at position L-1, f32 [nb,V].
 * `ws`: scratch of at least emoasr_decode_ws_bytes(...) bytes. */
typedef struct emoasr_lin { const void* w; const float* b; } emoasr_lin_t;   /* weight (compute dtype), bias f32 */
typedef struct emoasr_lnp { const float *g, *b; } emoasr_lnp_t;
typedef struct emoasr_decoder_layer {
  emoasr_lnp_t ln1, ln2, ln3;
  emoasr_lin_t qkv, out;        /* self-attention: fused [3dd,dd] projection, output */
  emoasr_lin_t q2, out2;        /* source attention (K / V come from the cache) */
  emoasr_lin_t w1, w2;          /* feed-forward [F,dd], [dd,F] */
} emoasr_decoder_layer_t;
typedef struct emoasr_decoder_infer {
  int nb, L, T, dd, H, F, V;
  const int* ids;               /* int32 [nb,L] */
  const void* embed; const float* pe; float emb_scale;   /* token table [V,dd], abs. position table f32 [>=L,dd] */
  const int *kself, *kmem;      /* int32 [nb]: valid prefix length (= L), valid memory frames */
  const void* const* kv;        /* nl pointers */
  emoasr_lnp_t ln_out; emoasr_lin_t out;
  void* logits_last;
  void* ws; size_t ws_bytes;
} emoasr_decoder_infer_t;
typedef struct emoasr_bert_layer {
  emoasr_lin_t qkv, attn_out; emoasr_lnp_t ln_attn;
  emoasr_lin_t inter, out; emoasr_lnp_t ln_out;
} emoasr_bert_layer_t;
typedef struct emoasr_bert_infer {
  int nb, L, d, H, F, V;
  const int* ids; const void* word_emb; const float* pe;  /* pe = position + token-type-0 embeddings, f32 [>=L,d] */
  emoasr_lnp_t ln_emb;
  const int* klens;
  emoasr_lin_t transform; emoasr_lnp_t ln_transform; const float* out_bias;
  float* logp;
  void* ws; size_t ws_bytes;
} emoasr_bert_infer_t;
size_t emoasr_decode_ws_bytes(int dtype, int nb, int L, int d, int H, int F, int V);
int emoasr_transformer_decoder_infer(int dtype, int nl, const emoasr_decoder_layer_t* layers,
                                     const emoasr_decoder_infer_t* io, void* stream);
int emoasr_bert_lm_infer(int dtype, int nl, const emoasr_bert_layer_t* layers, const emoasr_bert_infer_t* io,
                         void* stream);

/* ---- the same two networks one POSITION at a time, with self-attention K / V caches, and the beam bookkeeping on the
 * device (csrc/decode_rt.hip): a step is a fixed launch sequence without host input, so it can be captured in a HIP graph.
 * Caches: compute dtype [nl][nb][Lmax][d] (K and V separately).  `pos` (device int) = position of the token in `ids`
 * (prefix length - 1); klens (device int32 [nb]) = pos + 1.  emoasr_beam_cache_gather re-orders the caches of a new step's
 * hypotheses by their parent: dst[l][b][t < pos] = src[l][parent[b]][t]. */
typedef struct emoasr_decoder_step {
  int nb, Lmax, T, dd, H, F, V;
  const int* ids; const int* pos; const int* klens;
  const void* embed; const float* pe; float emb_scale;
  const int* kmem; const void* const* kv;       /* as in emoasr_decoder_infer_t */
  void* kcache; void* vcache;
  emoasr_lnp_t ln_out; emoasr_lin_t out;
  void* logits_last;                             /* [nb, V] compute dtype */
  void* ws; size_t ws_bytes;                     /* emoasr_decode_step_ws_bytes() */
} emoasr_decoder_step_t;
typedef struct emoasr_bert_step {
  int nb, Lmax, d, H, F, V;
  const int* ids; const int* pos; const int* klens;
  const void* word_emb; const float* pe; emoasr_lnp_t ln_emb;
  void* kcache; void* vcache;
  emoasr_lin_t transform; emoasr_lnp_t ln_transform; const float* out_bias;
  float* logp;                                   /* f32 [nb, V] log-probabilities of the next token */
  int raw_logits;                                /* 1: leave the raw logits in logp (no log-softmax) */
  void* ws; size_t ws_bytes;
} emoasr_bert_step_t;
size_t emoasr_decode_step_ws_bytes(int dtype, int nb, int d, int H, int F, int V);
int emoasr_transformer_decoder_step(int dtype, int nl, const emoasr_decoder_layer_t* layers, const emoasr_decoder_step_t* io,
                                    void* stream);
int emoasr_bert_lm_step(int dtype, int nl, const emoasr_bert_layer_t* layers, const emoasr_bert_step_t* io, void* stream);
/* Small-M pieces of those steps (csrc/rowlin.hip; bf16): y[M <= 16, N] = act(LN?(x) . W^T + bias) (+ res | LayerNorm(res)) with the
 * LayerNorms computed inside the kernel, and single-query attention of row b of qkv [nb, 3d] against the caches, appending
 * the new key / value at *pos first. */
int emoasr_rowlin(int M, int N, int K, const void* x, long ldx, const float* lna_g, const float* lna_b, float lna_eps,
                  const void* w, const float* bias, int act, const void* res, long ldres, const float* lnr_g,
                  const float* lnr_b, float lnr_eps, void* y, int out_f32, long ldy, void* stream);
int emoasr_attn_step(int nb, int d, int H, int Lmax, const void* qkv, void* kcache, void* vcache, const int* pos, void* out,
                     void* stream);
/* The steps run as one cooperative launch per network (csrc/decode_coop.hip, option "decode_coop", bf16, <= 16 hypotheses): 0 when
 * none of its grid barriers ever gave up waiting, 1 otherwise (results of that step are then undefined), -1 on a runtime error.
 * Synchronises the device. */
long emoasr_decode_coop_status(void);

/* ---- Transformer-LM shallow fusion inside the batched transducer search, over a PREFIX TREE (csrc/lm_tree.hip;
 * engine.rnnt_beam_search_batch with a Transformer LM under decoder.rnnt_tlm_fusion = "device").  Every token a hypothesis appends is
 * one NODE whose key / value rows are written once and never copied; a state slot (the slot numbers of the prediction network's
 * pools) holds the node ids of its prefix: llen int32 [nslots] (prefix length; 0 in a search's zero-state slot), lanc int32
 * [nslots][Lcap] (node ids, oldest first).  Search s owns the nodes s * node_cap .. (s + 1) * node_cap - 1 of the pools (compute
 * dtype [nl][nodes][d], K and V separately, nodes = S * node_cap) and has taken nnodes[s] of them so far.
 *   emoasr_lm_tree_advance: one launch per round, one wave per search, no atomics.  Row i = s W + w of the control words
 *       emoasr_rnnt_beam_book wrote (source slot, destination slot, active; int64 [R = S W] each) is LIVE when active[i] != 0 and both
 *       slots lie in 0 .. nslots - 1 and 0 <= p = llen[src[i]].  A live row whose prefix would exceed Lcap (p >= Lcap) raises
 *       EMOASR_LM_TREE_OVERLEN in status[s]; the live rows left take the nodes s * node_cap + nnodes[s] + 0, 1, ... in row order
 *       (inactive rows take none) until the search's node_cap is used up, every row past that raises EMOASR_LM_TREE_POOL_FULL.  A row
 *       that got a node copies lanc[src][:p] to lanc[dst], appends the node, sets llen[dst] = p + 1 and records row_node[i] = node,
 *       row_pos[i] = p; every other row records row_node[i] = -1 and changes nothing else.  No live row's source slot may be another
 *       row's destination in the same launch (the book kernel's mark and sweep guarantees it).
 *   emoasr_lm_tree_attn: single-query attention GATHERED through the lists, one wave per (row, head): a row with row_node[i] >= 0
 *       writes k / v (row i of qkv [R, 3d] = q | k | v) at its node of this layer's pools, then out[i] = softmax(q . K[lanc[dst[i]]
 *       [0 .. p]]^T / sqrt(dk)) . V[...] with f32 accumulation (p + 1 = llen[dst[i]] keys, the new one last).  dk = d / H in 8 .. 128,
 *       a multiple of 8; 8 Lcap + 1536 bytes of LDS (<= 64 KB).  A row with row_node[i] < 0, a slot or a length out of range writes
 *       nothing; node ids read from a list are clamped into the pool.
 *   emoasr_lm_tree_step: the launch chain of emoasr_bert_lm_step for R rows of any count -- embedding of label lab[i] (int64 control
 *       words; clamped into the table) + pe[row_pos[i]], LayerNorm, per layer (qkv product, emoasr_lm_tree_attn, output product,
 *       LayerNorm, feed-forward, LayerNorm), the prediction head -> RAW logits [R, V] of the compute dtype (emoasr_rnnt_beam_pick_lm
 *       takes its own log-softmax).  No host input between the launches.  Rows with row_node[i] < 0 carry zeros / stale values. */
#define EMOASR_LM_TREE_OVERLEN 1
#define EMOASR_LM_TREE_POOL_FULL 2
typedef struct emoasr_lm_tree {
  int S, W, nslots, Lcap, node_cap;
  int* llen; int* lanc; int* nnodes;            /* [nslots], [nslots][Lcap], [S] */
  int* row_node; int* row_pos;                  /* [S W] each, written by advance */
  int* status;                                  /* [S], bits are only ever raised */
} emoasr_lm_tree_t;
typedef struct emoasr_lm_tree_step {
  int d, H, F, V, n_emb;
  const long long* lab; const long long* dst;   /* control words, [S W] each */
  const void* word_emb; const float* pe; emoasr_lnp_t ln_emb;     /* word_emb [n_emb, d]; pe f32 [>= Lcap, d] */
  void* kpool; void* vpool;                     /* compute dtype [nl][S node_cap][d] */
  emoasr_lin_t transform; emoasr_lnp_t ln_transform; const float* out_bias;
  void* logits;                                 /* compute dtype [S W, V] */
  void* ws; size_t ws_bytes;                    /* emoasr_lm_tree_step_ws_bytes() */
} emoasr_lm_tree_step_t;
int emoasr_lm_tree_advance(const emoasr_lm_tree_t* t, const long long* src, const long long* dst, const long long* active,
                           void* stream);
int emoasr_lm_tree_attn(int dtype, const emoasr_lm_tree_t* t, int d, int H, const void* qkv, void* kpool, void* vpool,
                        const long long* dst, void* out, void* stream);
size_t emoasr_lm_tree_step_ws_bytes(int dtype, int R, int d, int F);
int emoasr_lm_tree_step(int dtype, int nl, const emoasr_bert_layer_t* layers, const emoasr_lm_tree_t* t,
                        const emoasr_lm_tree_step_t* io, void* stream);
/* The same tree under the fused CTC search (csrc/ctc_beam_lm.hip; decoder.ctc_tlm_fusion = "device"): the tree's slots are the rows of
 * the LM pool (search s owns the slots s * nslots / S .. and the nodes s * node_cap ..), the rows of a step are the frame's RECORDS.
 *   emoasr_lm_tree_advance_rec: rec int32 [6][rec_cap] (search, node id, parent id, token, src row, dst row) and rec_count int32 [1]
 *       as emoasr_ctc_beam_lm_frame left them on the device; row_node, row_pos, lab and dst hold rec_cap entries.  Record r <
 *       *rec_count with src < 0 starts from the empty prefix (p = 0), otherwise p = llen[src]; it takes one node of its search's share
 *       (one atomicAdd: which record gets which node is not defined, nothing else depends on the order of the records), copies
 *       lanc[src][:p] to lanc[dst], appends the node, sets llen[dst] = p + 1, row_node[r] = node, row_pos[r] = p and the control words
 *       lab[r] = token, dst[r] = dst row, which emoasr_lm_tree_attn / _step read.  p >= Lcap raises EMOASR_LM_TREE_OVERLEN in
 *       status[search], a share that is used up EMOASR_LM_TREE_POOL_FULL; such a row, a row r >= *rec_count, a record that names a
 *       search outside 0 .. S - 1 or a slot outside that search's share, and (lm_weight f64 [S] given) a record of a search with
 *       lm_weight <= 0 get row_node[r] = -1, lab[r] = 0, dst[r] = -1 and change nothing else.  No record's src row may be another
 *       record's dst row in the same launch (the frame kernel frees a row one frame after its prefix left the beam).
 *   emoasr_lm_tree_attn_rows / emoasr_lm_tree_step_rows: emoasr_lm_tree_attn / _step over the first R rows (R >= 0; the entry points
 *       above are these with R = S W): launches and products are sized by R, rows >= R are neither read nor written.
 *   emoasr_log_softmax_rows_to: row r < n of x [n, V_lm] (compute dtype, row stride ldx) is normalised over all V_lm columns with the
 *       body of emoasr_log_softmax, its first V columns go to row row_dst[r] of the f32 pool out (row stride ld_lm, out_rows rows):
 *       bit-equal to emoasr_log_softmax of the same row.  A row with row_dst outside the pool or (row_ok given) row_ok[r] < 0 is
 *       dropped; columns >= V and every other row of the pool are not touched. */
int emoasr_lm_tree_advance_rec(const emoasr_lm_tree_t* t, const int* rec, int rec_cap, const int* rec_count, const double* lm_weight,
                               long long* lab, long long* dst, void* stream);
int emoasr_lm_tree_attn_rows(int dtype, const emoasr_lm_tree_t* t, int R, int d, int H, const void* qkv, void* kpool, void* vpool,
                             const long long* dst, void* out, void* stream);
int emoasr_lm_tree_step_rows(int dtype, int nl, const emoasr_bert_layer_t* layers, const emoasr_lm_tree_t* t,
                             const emoasr_lm_tree_step_t* io, int R, void* stream);
int emoasr_log_softmax_rows_to(int dtype, int n, int V_lm, int V, const void* x, long ldx, const int* row_dst, const int* row_ok,
                               float* out, long ld_lm, int out_rows, void* stream);
/* times the cooperative step kernel of a chain (0 decoder, 1 LM) was enqueued or captured since the library was loaded */
long emoasr_decode_coop_launches(int chain);
int emoasr_beam_cache_gather(int dtype, int nl, int nb, int Lmax, int d, const void* src_k, const void* src_v, void* dst_k,
                             void* dst_v, const int* parent, const int* pos, void* stream);
/* Beam bookkeeping of one output step (decoders/transformer.py:215-290) for up to 32 beams x 32 candidates, one workgroup:
 * candidate scores in numpy-float32 arithmetic, accumulated hypothesis scores in double (Python float), stable orders,
 * <eos> -> result (score + len_weight * len(hyp incl. sos/eos); empty hypotheses dropped), the rest -> the next step's
 * beams.  All arrays live on the device; `state` carries pos / n_alive / n_results / done between steps (done: the kernel
 * returns immediately, so replaying a captured step past the end is harmless).  hist_parent / hist_token [max_steps][bw]
 * record the surviving beams of every step (the host rebuilds the token sequences once, at the end). */
typedef struct emoasr_beam_state { int pos, n_alive, n_results, done; } emoasr_beam_state_t;
typedef struct emoasr_beam_update {
  int bw, cw, eos;
  float one_minus_lam, lam, mu;                  /* f32(1 - ctc_weight), f32(ctc_weight), f32(lm_weight) */
  double len_weight;
  const float* vals; const int* cands;           /* [bw, cw] top candidates of scores_att(+lm) per beam */
  const float* lm_at;                            /* [bw, cw] LM log-probs at the candidates, or NULL */
  const float* psi;                              /* [bw, cw] CTC prefix scores, or NULL (no CTC term) */
  double* score; float* score_ctc;               /* [bw] current beams; overwritten with the next step's */
  int *n_ids, *n_parent, *n_pcand, *n_last, *n_outlen, *n_klens;   /* [bw] inputs of the next step */
  int *hist_parent, *hist_token;
  double* res_score; int* res_step; int* res_parent;               /* [bw] finished hypotheses */
  emoasr_beam_state_t* state;
  int* host_mirror;                              /* optional: pinned host memory (device-visible) that receives a copy of `state`
                                                  * at the end of every live step -- the host polls it instead of copying */
} emoasr_beam_update_t;
int emoasr_beam_update(const emoasr_beam_update_t* u, void* stream);
/* One whole output step (cache gather, decoder step, LM step on `side_stream` when given, log-softmax + LM fusion, top-cw,
 * CTC prefix scores, beam update) from one call.  parent / pcand / last / out_len of the CURRENT beams are upd.n_parent /
 * n_pcand / n_last / n_outlen as the previous step's update left them; *_prev are the previous step's caches and CTC scorer
 * states [bw, cw, T, 2] (before the first step: the initial state at [0, 0]).  lm_nl == 0: no LM; upd.psi == NULL: no CTC. */
typedef struct emoasr_joint_step {
  int dec_nl; const emoasr_decoder_layer_t* dec_layers; emoasr_decoder_step_t dec;
  int lm_nl; const emoasr_bert_layer_t* lm_layers; emoasr_bert_step_t lm;
  const void *dec_k_prev, *dec_v_prev, *lm_k_prev, *lm_v_prev;
  const int* parent;
  float* scores_pre;                               /* f32 [bw, V] */
  const float* ctc_x; int T; int blank;            /* CTC log-probs f32 [T, V] */
  const float* states_prev; float* states_cur;
  emoasr_beam_update_t upd;
} emoasr_joint_step_t;
int emoasr_joint_beam_step(int dtype, const emoasr_joint_step_t* js, void* stream, void* side_stream);
/* Parts of the step on ONE stream (mask: 1 = decoder chain incl. its cache gather, 2 = LM chain, 4 = scoring tail), and the
 * parts as HIP graphs: build captures part 0 / 1 / 2 (decoder / LM / tail) of slot 0 / 1 (even / odd steps), or updates the
 * instantiated graph with a new utterance's pointers; launch replays it.  The caller orders the three launches of a step
 * with events: the two chains on two streams, the tail after both (~185 kernels per ~0.1 ms of host time, against
 * ~1.1 ms for launching them one by one). */
int emoasr_joint_beam_step_parts(int dtype, const emoasr_joint_step_t* js, int parts, void* stream);
int emoasr_joint_beam_graph_build(int dtype, const emoasr_joint_step_t* js, int slot, int part, void* stream);
int emoasr_joint_beam_graph_launch(int slot, int part, void* stream);

/* ---- the joint search for S utterances at once (csrc/decode_batch.hip, csrc/decode_rt.hip).  A search is
 * one utterance; S searches of width W occupy rows s * W .. s * W + W - 1 of every per-hypothesis array (nb = S * W rows) and
 * all live searches are at the same output position.  A finished search keeps its rows: they are computed and ignored. */
/* Single-query cross-attention of every search's W hypotheses against that search's own memory: q [S * W, dd], kv the
 * projected memories stacked over the searches [sum T_s, 2 dd] (K in the first dd columns, V in the second), moff
 * (device int32 [S + 1]) the first row of every search, out [S * W, dd].  1 <= W <= 32, dd / H in {32, 64, 128}, T_s >= 1.
 * A row's result does not depend on S or on the other searches.  emoasr_group_offsets_check verifies a HOST copy of the
 * offsets (rising, T_s >= 1) before they are uploaded. */
int emoasr_attn_step_group(int dtype, int S, int W, int dd, int H, const void* q, const void* kv, const int* moff, void* out,
                           void* stream);
int emoasr_group_offsets_check(int S, const int* moff_host);
/* emoasr_beam_update for S searches, one workgroup each: u's arrays hold nb = S * bw rows (vals / cands / psi / lm_at
 * [nb, cw]), u.state is state[S], hist_parent / hist_token are [max_pos][S][bw], the results of search s are at s * bw.
 * n_parent is a GLOBAL row (s * bw + parent); n_pcand, the history and res_parent are local to the search.  *pos is the shared
 * output position: a one-thread launch after the S workgroups advances it once per live step, sets ctl[0] when every search
 * has finished and writes u.host_mirror = {pos, finished searches} (payload first, position last).  A step replayed after
 * ctl[0] is set, or at pos >= max_pos, changes nothing. */
typedef struct emoasr_beam_update_batch {
  emoasr_beam_update_t u;
  int S, max_pos;
  int* pos;
  int* ctl;
} emoasr_beam_update_batch_t;
int emoasr_beam_update_batch(const emoasr_beam_update_batch_t* b, void* stream);
/* The ragged twins of emoasr_ctc_prefix_init / emoasr_ctc_prefix_score: x the stacked emissions [sum T_s, V], xoff (device
 * int32 [S + 1]); row m belongs to search m / W and runs over that search's T_s frames; states [nb, cw, Tmax, 2].  The init
 * writes search s's initial state to r + s * r_stride. */
int emoasr_ctc_prefix_init_ragged(int S, int V, const float* x, const int* xoff, int blank, float* r, long r_stride, void* stream);
int emoasr_ctc_prefix_score_ragged(int nb, int W, int Tmax, int V, int cw, const float* x, const int* xoff,
                                   const float* prev_states, int cw_prev, const int* parent, const int* pcand, const int* last,
                                   const int* out_len, const int* cands, int blank, int eos, float* log_psi, float* states,
                                   void* stream);
/* The launch chain of emoasr_transformer_decoder_step on nb = S * W rows with emoasr_attn_step_group in place of the
 * cross-attention: d.kv[l] is layer l's STACKED memory projection [sum T_s, 2 dd]; d.T and d.kmem are not read. */
typedef struct emoasr_decoder_step_group {
  emoasr_decoder_step_t d;
  int S, W;
  const int* moff;
} emoasr_decoder_step_group_t;
size_t emoasr_decode_step_group_ws_bytes(int dtype, int nb, int d, int H, int F, int V);
int emoasr_transformer_decoder_step_group(int dtype, int nl, const emoasr_decoder_layer_t* layers,
                                          const emoasr_decoder_step_group_t* io, void* stream);
/* One output step of all S searches as a linear chain on one stream: cache gathers, decoder step, LM step
 * (emoasr_bert_lm_step on nb rows), emoasr_beam_scores_topk, the ragged CTC scorer (xoff = dec.moff), the batched update. */
typedef struct emoasr_joint_batch_step {
  int dec_nl; const emoasr_decoder_layer_t* dec_layers; emoasr_decoder_step_group_t dec;
  int lm_nl; const emoasr_bert_layer_t* lm_layers; emoasr_bert_step_t lm;
  const void *dec_k_prev, *dec_v_prev, *lm_k_prev, *lm_v_prev;
  const int* parent;
  const float* ctc_x; int Tmax; int blank;
  const float* states_prev; float* states_cur;
  emoasr_beam_update_batch_t upd;
} emoasr_joint_batch_step_t;
int emoasr_joint_beam_batch_step(int dtype, const emoasr_joint_batch_step_t* js, void* stream);

/* ---- the fusion grid of the joint search (csrc/decode_grid.hip, csrc/decode_rt.hip).  A search is an
 * (utterance, lm_weight) pair.  Rows as above: search s owns rows s * W .. s * W + W - 1.  sutt (device int32 [S]) is the
 * utterance of every search, searches of one utterance are consecutive; moff / xoff (device int32 [U + 1]) are the first frames
 * of the U UTTERANCES, whose frames are stored once.  Every kernel gives a row the bits its scalar twin above gives it on
 * that row's search (the twin run with one offset entry per search over replicated frames, and with the search's weight). */
/* emoasr_attn_step_group with one workgroup per (group, head): groups (device int32 [G, 3]) = {first row, rows, utterance} of up
 * to max_rows <= 32 consecutive rows whose searches share one utterance; q / out [nb, dd].  Rows of a group beyond its count, and
 * the rows of an entry that does not fit (rows outside 0 .. nb, more than max_rows rounded up to 8, utterance outside 0 .. U - 1)
 * are never written.  emoasr_cell_groups_check verifies a HOST copy of the table: the groups cover rows 0 .. nb - 1 once, in
 * order. */
int emoasr_attn_step_cells(int dtype, int G, int max_rows, int nb, int U, int dd, int H, const void* q, const void* kv,
                           const int* moff, const int* groups, void* out, void* stream);
int emoasr_cell_groups_check(int G, const int* groups_host, int max_rows, int nb, int U);
/* emoasr_beam_scores_topk with the weight of row m in mu_row[m] (device f32 [M]; not read when lm == NULL) */
int emoasr_beam_scores_topk_rows(int dtype, int M, int V, int k, const void* dec, long ldd, const float* lm, long ldl,
                                 const float* mu_row, float* vals, int* idx, float* lm_at, void* stream);
/* The ragged CTC scorer pair with search s over the frames of utterance sutt[s].  The init computes an utterance's initial
 * state once and writes it to r + s * r_stride of each of its searches. */
int emoasr_ctc_prefix_init_cells(int S, int U, int V, const float* x, const int* xoff, const int* sutt, int blank, float* r,
                                 long r_stride, void* stream);
int emoasr_ctc_prefix_score_cells(int nb, int W, int Tmax, int V, int cw, const float* x, const int* xoff, const int* sutt,
                                  const float* prev_states, int cw_prev, const int* parent, const int* pcand, const int* last,
                                  const int* out_len, const int* cands, int blank, int eos, float* log_psi, float* states,
                                  void* stream);
/* emoasr_beam_update_batch with the LM weight of search s in mu[s] (device f32 [S], rounded as u.mu is); u.mu is not read */
int emoasr_beam_update_cells(const emoasr_beam_update_batch_t* b, const float* mu, void* stream);
/* One output step of all S searches: the linear chain of emoasr_joint_beam_batch_step with the kernels above.  js.dec.moff holds
 * the U utterances' offsets, js.dec.S the searches; js.upd.u.len_weight must be 0 (a result's score is then its hypothesis
 * score; the caller adds len_weight * (position + 2) in double for every length weight of the grid); mu_row [S * W] repeats
 * mu[s] for the rows of search s. */
typedef struct emoasr_joint_grid_step {
  emoasr_joint_batch_step_t js;
  int U, n_groups, group_rows;                   /* utterances; rows of `groups`; the most rows of a group */
  const int* sutt; const int* groups;
  const float* mu; const float* mu_row;
} emoasr_joint_grid_step_t;
int emoasr_joint_beam_grid_step(int dtype, const emoasr_joint_grid_step_t* gs, void* stream);
/* The two chains above with the stateful RNN LM in place of the Transformer LM: js.lm_nl must be 0 (js.lm and
 * the LM's cache pointers are not read); emoasr_rnnlm_step_rows(rl, ids = js.dec.d.ids, parent = js.parent) takes the place of the
 * LM's cache gather and emoasr_bert_lm_step, rl->logits (raw f32, rl->R = the chain's rows, rl->V = the decoder's V) is the `lm`
 * operand of emoasr_beam_scores_topk (weight js.upd.u.mu) / _rows (weight gs->mu_row). */
int emoasr_joint_beam_batch_step_rnnlm(int dtype, const emoasr_joint_batch_step_t* js, const emoasr_rnnlm_rows_t* rl, void* stream);
int emoasr_joint_beam_grid_step_rnnlm(int dtype, const emoasr_joint_grid_step_t* gs, const emoasr_rnnlm_rows_t* rl, void* stream);

/* ---- the LAS beam search for S utterances at once (csrc/las_beam.hip).  Rows as above: search s owns
 * rows s * W .. s * W + W - 1; `state` is the array emoasr_beam_update_batch keeps, `parent` its n_parent (GLOBAL rows).  A row at
 * or past its search's n_alive, and every row of a search that is done, is SKIPPED: nothing of it is read (its parent may hold
 * anything) and nothing is written for it.  A live row whose parent lies outside its own search is read from the search's row 0. */
/* One decoder position of the location-aware attention (emoasr_las_attend_fwd's arithmetic with drop_p = 0) for all rows:
 * pk [sum T_s, A] / eouts [sum T_s, D] the searches' stacked key projections / encoder frames (once per utterance), moff (device
 * int32 [S + 1]) their first rows, pq [S * W, A]; aw_src / aw_dst f32 [S * W, Tmax] the previous weights (read at the PARENT's row,
 * frames 0 .. T_s - 1) and the new ones (written at the row's own), scores f32 [S * W, Tmax] scratch, ctx rows of stride ctx_ld.
 * Tmax >= every T_s.  Score pass: one workgroup per (32-frame tile of a search, search) -- the filter and the tile of pk are fetched
 * once for all live rows; context pass: one workgroup per (64 context columns, search) -- every eouts tile is fetched once for the
 * W rows.  Tiles count from the search's own first frame: a row's bits do not depend on S or on the other searches.
 * 1 <= W <= 32, A % 8 == 0, A <= 512, D % 8 == 0, ctx_ld % 8 == 0. */
typedef struct emoasr_las_attend_group {
  int S, W, A, D, Tmax;
  int rows;                      /* sum T_s: a search whose frames do not lie inside [0, rows) or exceed Tmax is skipped */
  const void* pk;
  const void* eouts;
  const int* moff;
  const void* pq;
  const float* aw_src;
  const int* parent;
  const emoasr_beam_state_t* state;
  const float *filt, *w_conv, *b_conv, *w_score;
  float* scores;
  float* aw_dst;
  void* ctx; long ctx_ld;
} emoasr_las_attend_group_t;
int emoasr_las_attend_group(int dtype, const emoasr_las_attend_group_t* a, void* stream);
/* emoasr_las_attend_group for the fusion grid: a search is an (utterance, lm_weight) pair.  g.S counts the
 * SEARCHES, g.moff (device int32 [U + 1]) holds the first frames of the U UTTERANCES, whose pk / eouts rows are stored once;
 * search s runs over the frames of utterance sutt[s] (device int32 [S], searches of one utterance consecutive).  The kernels are
 * the group form's own, compiled with one more flag: a row gets the bits emoasr_las_attend_group gives it when run with one offset
 * entry per search over replicated frames.  A search whose sutt[s] lies outside 0 .. U - 1 is skipped like a finished one.
 * emoasr_las_cells_check verifies a HOST copy of the map (0 .. U - 1 in order, consecutive, every utterance present) before the
 * upload. */
typedef struct emoasr_las_attend_cells {
  emoasr_las_attend_group_t g;
  int U;
  const int* sutt;
} emoasr_las_attend_cells_t;
int emoasr_las_attend_cells(int dtype, const emoasr_las_attend_cells_t* c, void* stream);
int emoasr_las_cells_check(int S, const int* sutt_host, int U);
/* Parent row -> child row for the small state arrays of a step, one launch: item k copies row_bytes (a multiple of 16, both
 * pointers 16-byte aligned) from src + parent[r] * row_bytes to dst + r * row_bytes for every live row r.  Exact copies. */
#define EMOASR_LAS_GATHER_MAX 16
typedef struct emoasr_las_gather_item { const void* src; void* dst; long row_bytes; } emoasr_las_gather_item_t;
typedef struct emoasr_las_state_gather {
  int S, W, n;
  const int* parent;
  const emoasr_beam_state_t* state;
  emoasr_las_gather_item_t item[EMOASR_LAS_GATHER_MAX];
} emoasr_las_state_gather_t;
int emoasr_las_state_gather(const emoasr_las_state_gather_t* g, void* stream);
/* The prefix tree of csrc/lm_tree.hip under this search (decoder.las_tlm_fusion = "device"), advanced from the
 * lockstep book: ids / parent (device int32 [S W]: emoasr_beam_update_batch's n_ids / n_parent) and `state`.  One launch per step, one
 * wave per search, no atomics.  The tree's slots are two halves of S W (nslots >= 2 S W): row r = s W + w reads slot src_base + parent'
 * and writes slot dst_base + r, (src_base, dst_base) = (0, S W) on even steps and (S W, 0) on odd ones; the two ranges must lie apart
 * inside the slots.  Rows are live and parents corrected by the rule above; a live row with p = llen[src] >= Lcap raises
 * EMOASR_LM_TREE_OVERLEN in status[s], the live rows left take the nodes s * node_cap + nnodes[s] + 0, 1, ... in row order until the
 * share is used up (then EMOASR_LM_TREE_POOL_FULL).  A row that got a node copies lanc[src][:p] to lanc[dst], appends the node, sets
 * llen[dst] = p + 1, row_node[r] = node, row_pos[r] = p, lab[r] = ids[r], dst[r] = its slot; every other row records row_node[r] = -1,
 * row_pos[r] = 0, lab[r] = 0, dst[r] = -1 and changes nothing else.  lab / dst: the int64 control words of emoasr_lm_tree_step. */
int emoasr_lm_tree_advance_beam(const emoasr_lm_tree_t* t, const int* ids, const int* parent, const emoasr_beam_state_t* state,
                                int src_base, int dst_base, long long* lab, long long* dst, void* stream);

/* ---- optimizer (asr/train_asr.py:84-92, torch.optim.Adam semantics) ---------- */
/* out[0] += sum x^2 */
int emoasr_sqnorm(long n, const float* x, float* out, void* stream);
/* Adam with coupled L2 weight decay.  gnorm_sq (device, 1 float): gradients are
 * scaled by min(1, clip/(sqrt(gnorm_sq)+1e-6)) when clip > 0 (clip_grad_norm_);
 * the whole update is skipped on device if gnorm_sq is NaN/Inf (train_asr.py:88-89). */
int emoasr_adam_step(long n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, const float* gnorm_sq,
                     float clip, float grad_mult, void* stream);
/* the same; a skipped step also increments *skipped (device int, may be NULL): the host subtracts it from its step
 * counters at its next synchronisation point, so that the schedule position and the bias correction follow the number of
 * updates actually applied, as in the reference (which does not call optimizer.step() on a NaN norm) */
int emoasr_adam_step_ex(long n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, const float* gnorm_sq, float clip, float grad_mult, int* skipped,
                        void* stream);
/* torch.optim.AdamW (lm/train_lm.py:188-195) over the flat arena: p *= 1 - lr * wd, then the Adam update without the coupled
 * decay term; clip / NaN skip / skipped counter as emoasr_adam_step_ex.  The arena is described by a span table on the DEVICE:
 * span_end [nspans] (ascending element offsets, every one a multiple of 64 except the last = n; span k is
 * [span_end[k-1], span_end[k])) and span_wd [nspans]: the span's weight decay, or a NEGATIVE value for a span the update leaves
 * bit-identical (a parameter that never received a gradient: no decay, no moments -- torch skips `grad is None`). */
int emoasr_adamw_step(long n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2, float eps,
                      int step, const float* gnorm_sq, float clip, float grad_mult, int* skipped, const long* span_end,
                      const float* span_wd, int nspans, void* stream);

/* ---- on-GPU features --------------------------------------------------------- */
/* SpecAugment (asr/spec_augment.py:39-95): zero (or fill) bands.  spans int32
 * [B, nf+nt, 2] = (start, end) per mask, first nf are frequency masks; built on the
 * host from the reference's sampling rule.  x f32 [B,T,F] in place. */
int emoasr_specaug_apply(int B, int T, int F, float* x, const int* spans, int nf, int nt,
                         const int* xlens, const float* fill, void* stream);
/* Kaldi-compatible log-mel filterbank (corpora/utils/wav_to_feats.py:26-33 defaults):
 * wav f32 [n_samples] (already scaled by 2^15) -> feats f32 [T, n_mel];
 * mel_fb f32 [n_mel, n_fft/2+1] from the host. */
int emoasr_fbank(const float* wav, long n_samples, int frame_len, int frame_shift, int n_fft, int n_mel,
                 float preemph, const float* window, const float* mel_fb, float* feats, int T,
                 void* stream);
/* (x - mean[f]) / std[f] in place, f32 [M,F] */
int emoasr_cmvn(int M, int F, float* x, const float* mean, const float* std, void* stream);

/* ---- CTC prefix beam search: per-frame bookkeeping (host) ------------------------------------------------- */
/* The prefix bookkeeping of CTCDecoder._beam_search / _merge_ctc_paths (asr/modeling/decoders/ctc.py:262-344, 372-397) as native
 * HOST code in IEEE doubles, bit-identical to the reference's python floats: extend every live prefix by blank / repeat and by the
 * frame's top-k labels, merge equal label sequences (path probabilities folded, the first path's LM / length scores kept), stable
 * sort by asr + lm + length bonus, keep beam_width.  The acoustic side (projection, log-soft-max, top-k) and the LM stay device
 * calls (emoasr_gemm_nt / emoasr_log_softmax / emoasr_topk; LM rows cached on the device, a frame brings only its k candidate
 * columns to the host).  emoasr_ctc_beam_step: row = the frame's log-probabilities f32 [V] (host), top = its k best labels (best
 * first; the blank is skipped), lm_lp = [live, k] LM log-probabilities of those labels after each live prefix or NULL;
 * parent / tok [beam_width] receive how each surviving prefix was formed (index into the previous live set; appended label or
 * -1 for an unchanged prefix).  -> number of live prefixes (< 0: error).  A search starts with the single prefix (<eos>). */
typedef struct emoasr_ctc_beam emoasr_ctc_beam_t;
emoasr_ctc_beam_t* emoasr_ctc_beam_new(int beam_width, int blank, int eos, double len_weight, double lm_weight);
void emoasr_ctc_beam_free(emoasr_ctc_beam_t* h);
int emoasr_ctc_beam_size(const emoasr_ctc_beam_t* h);
int emoasr_ctc_beam_step(emoasr_ctc_beam_t* h, const float* row, const int* top, int k, const double* lm_lp, int* parent, int* tok);
int emoasr_ctc_beam_prefix(const emoasr_ctc_beam_t* h, int i, int* toks, int cap);   /* -> length of live prefix i */
int emoasr_ctc_beam_scores(const emoasr_ctc_beam_t* h, double* total);              /* -> number of live prefixes */

/* ---- CTC prefix beam search, batched, on the device (no LM) ------------------------------------------------
 * emoasr_ctc_beam_batch: the same search for B utterances in one launch, for the case without LM fusion (the N-best lists of
 *   `test_asr.py --nbest --beam_width N` on a CTC model).  Results equal the host search above with lm_lp = NULL: the same
 *   hypotheses in the same order; per value the same sequence of double operations (NEG = -1e10, lse2(a, b) = m + log(exp(a - m) +
 *   exp(b - m)) with m the larger operand, rows widened from f32, total = (asr + 0.0) + len_weight * (plain labels of the parent
 *   + 1), nothing contracted), so the scores differ by the ulps of the device's exp / log against the host's only.
 *     logp  f32 [rows, V] (row stride ld), emoasr_log_softmax over all frames of all utterances; utterance b owns rows
 *           row_off[b] .. row_off[b+1] (int32 [B+1], rising from 0)
 *     top   int32 [rows, k], emoasr_topk of logp, best first, k = min(W, V) distinct labels per row; a blank among them is skipped
 *     out_tok int32 [B, W, max_frames + 1]; out_len int32 [B, W]; out_score f64 [B, W], best first; out_n int32 [B]: the number
 *           of live prefixes (< W when few frames or a small V cannot fill the beam).  Every hypothesis starts with eos.  Only the
 *           first out_n[b] rows of an utterance, and the first out_len tokens of a row, are written.  An utterance of 0 frames
 *           gives the single prefix (eos) with score 0.0.
 *     ws    emoasr_ctc_beam_batch_ws_bytes(B, rows, W) bytes, 8-byte aligned, any content: the per-utterance tries that give every
 *           prefix a canonical node id (the kernel clears its share); -1 from the query: W outside the limit.
 *   Limits: 1 <= W <= EMOASR_CTC_BEAM_MAX_WIDTH (an error return otherwise), no LM.  Ties of the total go to the candidate seen
 *   first (live prefix i, then its stay, then its extensions in top order): std::stable_sort's order.
 *   An utterance is not searched, gets out_n[b] = -1 and sets a bit of status[0] (int32, zeroed by the caller) when its top holds
 *   a label outside [0, V) (bit 0), its row_off falls or is negative (bit 1), it has more than max_frames frames (bit 2) or its
 *   share of ws is short (bit 3).  One workgroup per utterance; nothing is written outside the outputs and ws. */
#define EMOASR_CTC_BEAM_MAX_WIDTH 32
long emoasr_ctc_beam_batch_ws_bytes(int B, int total_rows, int W);
int emoasr_ctc_beam_batch(int B, int V, int W, int k, const float* logp, long ld, const int* row_off, const int* top, int blank,
                          int eos, double len_weight, int max_frames, int* out_tok, int* out_len, double* out_score, int* out_n,
                          void* ws, long ws_bytes, int* status, void* stream);

/* ---- CTC prefix beam search with LM shallow fusion, batched, on the device, one frame per launch -----------
 * A *search* is one (utterance, (lm_weight, len_weight)) pair.  S searches run over B utterances; several searches may name the
 * same utterance (the cells of a fusion grid) and share its logp / top rows, which are only read.  Results equal
 * emoasr_ctc_beam_step fed the same f32 LM rows as lm_lp: the same hypotheses in the same order, per value the same sequence of
 * double operations.  On top of emoasr_ctc_beam_batch's arithmetic: for live prefix i, lm_run starts at the prefix's LM term and,
 * for j = 1..k in top order with the blank skipped, lm_run = lm_run + lm_weight * (double)lm_logp[slot_i][top[t][j-1]] (one rounded
 * multiply, one rounded add); extension j carries the running value (the reference's `score_lm +=`, ctc.py:309-310), the stay the
 * prefix's own term; a fold keeps the LM term and length bonus of the candidate seen first; total = (asr + lm) + len_bonus.  A
 * search with lm_weight <= 0 reads no LM row, adds nothing and equals emoasr_ctc_beam_batch bit for bit.
 *     utt        int32 [S]: the utterance of each search; lm_weight / len_weight f64 [S]
 *     logp, ld, row_off, top, blank, eos, k = min(W, V): as for emoasr_ctc_beam_batch; max_frames >= the longest utterance
 *     lm_logp    f32 [S * slots, ld_lm >= V]: the pool of LM next-token rows.  Search s owns rows s * slots .. (s + 1) * slots - 1 and
 *                uses the first min(slots, emoasr_ctc_beam_lm_slots(W)) of them; emoasr_ctc_beam_lm_slots(W) = 2 W + 2 is enough
 *                (<= W live after the previous frame + <= W taken at this one; the row of a prefix that left the beam returns to
 *                the free list at the start of the NEXT frame, so this frame's records may still name it as a parent).
 *     rec        int32 [6, rec_cap], rec_count int32 [1]: the NEW prefixes of the launch (extensions without a live twin, and the
 *                root at init), column r = (search, node id, parent node id, token, src row, dst row) in rows 0..5; src / dst are
 *                rows of the pool, src = -1 for the root.  The caller must fill pool row dst with the LM's next-token row after
 *                that prefix (one LM step: token, state of src -> state of dst) before the next launch.  rec_cap >= S * W (init:
 *                >= S).  The count is zeroed by each call; the order of records of different searches is not defined and no
 *                result depends on it.
 *     ws         emoasr_ctc_beam_lm_ws_bytes(S, max_frames, W) bytes, 8-byte aligned: per search its live set (id, parent, last,
 *                n_plain, len, p_b, p_nb, lm, len_bonus, total, LM row), free list and waiting list, then its trie share.  It
 *                carries the searches from init through the frames to finish.
 *   emoasr_ctc_beam_lm_init    every search becomes the root (eos) with row 0 of its share; S root records.
 *   emoasr_ctc_beam_lm_frame   advances every search whose utterance has a frame t by that frame (t = 0, 1, .. in order); one
 *                              256-thread workgroup per search.
 *   emoasr_ctc_beam_lm_finish  out_tok int32 [S, W, max_frames + 1], out_len int32 [S, W], out_score f64 [S, W], out_n int32 [S],
 *                              as emoasr_ctc_beam_batch writes them per utterance.
 *   Limits: 1 <= W <= EMOASR_CTC_BEAM_MAX_WIDTH (an error return otherwise, nothing written).  A search is retired (no further
 *   writes, out_n = -1) and sets a bit of status[0] (int32, zeroed by the caller): bits 0-3 as emoasr_ctc_beam_batch (label outside
 *   [0, V); falling row_off; more frames than max_frames; workspace or record list short), bit 4: utt[s] outside [0, B), bit 5: no
 *   free row left in its share of the pool.  Nothing is written outside the outputs, rec / rec_count, status and ws. */
long emoasr_ctc_beam_lm_ws_bytes(int S, int max_frames, int W);
long emoasr_ctc_beam_lm_slots(int W);
int emoasr_ctc_beam_lm_init(int S, int B, int W, const int* row_off, const int* utt, int eos, int max_frames, int slots, void* ws,
                            long ws_bytes, int* rec, int rec_cap, int* rec_count, int* status, void* stream);
int emoasr_ctc_beam_lm_frame(int S, int B, int V, int W, int k, int t, const float* logp, long ld, const int* row_off,
                             const int* top, const int* utt, const double* lm_weight, const double* len_weight, int blank, int eos,
                             int max_frames, const float* lm_logp, long ld_lm, void* ws, long ws_bytes, int* rec, int rec_cap,
                             int* rec_count, int* status, void* stream);
int emoasr_ctc_beam_lm_finish(int S, int W, int max_frames, int eos, int* out_tok, int* out_len, double* out_score, int* out_n,
                              const void* ws, long ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
