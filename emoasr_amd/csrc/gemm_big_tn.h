// Host interface of the eight-wave 256x256 TN tile (gemm_big_tn.hip), used by the dispatch in gemm.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/emoasr_hip.h"

struct BigTnProblem {   // one product, bf16 operands: the fields of TnArgs in gemm.hip
  int N1, N2, K;
  const void* A; long lda;
  const void* B; long ldb;
  float* C; long ldc;
  float alpha;
  int k_tiles_per_split;   // filled by emo_tn_big_launch
  float* colsum;
  float colsum_scale;
};

// shapes the kernel takes (the caller adds: bf16, option "tn_big" on)
bool emo_tn_big_fits(int N1, int N2, int K, long lda, long ldb);
// one launch over n <= EMOASR_TN_GROUP_MAX products; splits[i] = wanted k slices of product i
int emo_tn_big_launch(int n, const BigTnProblem* probs, const int* splits, hipStream_t s);

// Conv2d weight gradient over nseg micro-batches in one launch (bf16, C % 256 == 0): dw [C, 9C] and dbias [C] (may be NULL) are
// accumulated into; blocks = the launch's block budget, max_splits = the most k slices the atomic traffic allows
bool emo_tn_big_conv_fits(int nseg, const emoasr_conv2_wgrad_seg_t* segs, int F1, int C);
int emo_tn_big_conv_launch(int nseg, const emoasr_conv2_wgrad_seg_t* segs, int F1, int C, float* dw, float* dbias, int blocks,
                           int max_splits, hipStream_t s);
