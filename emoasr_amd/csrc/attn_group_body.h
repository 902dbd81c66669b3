// The body of the grouped single-query cross-attention kernels, included INSIDE the kernel (text, not a function: both kernels
// compile from the same tokens, and emoasr_attn_step_group's to the code it always had).  The including kernel is a template over
// <T, DK, TK, WB> and provides: H, q, kv, scale, out; the macro EMO_ATTN_GROUP_OF_BLOCK, statements that define h (the head), W (the
// queries of this workgroup, unless W is a parameter), r0 (long: the first memory row) and Ts (memory rows) -- it may return for a
// workgroup without work; and the macro EMO_ATTN_ROW(w) -> the global row (long) of query w.
//
// LDS: the W queries (f32), one tile of TK keys and values (f32; the key rows padded by
// one float so that the TK lanes of a score column hit TK banks), the W x TK scores / probabilities and the running (max, sum,
// rescale) of every query.  Per tile: scores (a thread owns one key j and the queries w0, w0 + 256 / TK, ...: the key element is
// read once for all of them), the online soft-max update by 8 lanes per query, then P . V into the thread's own (query, column)
// accumulators (one column, the queries w1, w1 + 256 / DK, ...: the value element is read once for all of them).  The next
// tile's 16-byte chunks are fetched into registers before the current tile is computed.  Everything a row sees is its own
// search's memory in tiles counted from that memory's first row, so a row's bits do not depend on S, on WB or on the other rows
// of the workgroup.
  // WB: the group size rounded up to 8 / 16 / 24 / 32 -- the loops over a thread's queries have compile-time bounds and no
  // branches (queries W .. WB - 1 are zero rows whose results are never written)
  constexpr int NACC = WB * DK / G_THREADS;       // (query, column) accumulators per thread
  constexpr int WSTEP = G_THREADS / DK;           // ... their queries are WSTEP apart
  constexpr int NSC = WB * TK / G_THREADS;        // (query, key) scores per thread
  constexpr int SSTEP = G_THREADS / TK;
  constexpr int VN = Chunk16<T>::N;
  constexpr int CH = DK / VN;                     // chunks of a K (or V) row
  constexpr int NCH = TK * CH / G_THREADS;        // chunks of a K (or V) tile per thread
  static_assert(NACC * G_THREADS == WB * DK && NSC * G_THREADS == WB * TK && WB % 8 == 0 && WB <= G_MAXW && NCH * G_THREADS == TK * CH && NCH >= 1, "tiling");
  __shared__ float s_q[WB][DK];
  __shared__ float s_k[TK][DK + 1];
  __shared__ float s_v[TK][DK];
  __shared__ float s_p[WB][TK];
  __shared__ float s_m[G_MAXW], s_l[G_MAXW], s_a[G_MAXW];
  const int tid = threadIdx.x;
  const int dd = H * DK;
  EMO_ATTN_GROUP_OF_BLOCK
  Chunk16<T> ck[NCH], cv[NCH];
  auto fetch = [&](int t0) {   // rows t0 .. t0 + TK - 1 of the search (zero past its end)
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int x = tid + k * G_THREADS, j = x / CH, cc = x - j * CH;
      if (t0 + j < Ts) {
        const T* row = kv + (r0 + t0 + j) * 2 * dd + h * DK + cc * VN;
        ck[k] = *reinterpret_cast<const Chunk16<T>*>(row);
        cv[k] = *reinterpret_cast<const Chunk16<T>*>(row + dd);
      } else {
        ck[k].zero();
        cv[k].zero();
      }
    }
  };
  fetch(0);
  for (int i = tid; i < WB * DK; i += G_THREADS) {
    const int w = i / DK, c = i - w * DK;
    s_q[w][c] = w < W ? to_f32(q[EMO_ATTN_ROW(w) * dd + h * DK + c]) : 0.f;
  }
  if (tid < G_MAXW) { s_m[tid] = -INFINITY; s_l[tid] = 0.f; s_a[tid] = 0.f; }
  float acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.f;
  const int pc = tid % DK, pw = tid / DK;    // P . V: the thread's column and first query
  const int sj = tid % TK, sw = tid / TK;    // scores: the thread's key and first query
  for (int t0 = 0; t0 < Ts; t0 += TK) {
    const int n = min(TK, Ts - t0);
    __syncthreads();                         // (the previous tile's P . V has read s_v / s_p; the first pass: s_q is written)
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int x = tid + k * G_THREADS, j = x / CH, cc = x - j * CH;
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        s_k[j][cc * VN + e] = ck[k].get(e);
        s_v[j][cc * VN + e] = cv[k].get(e);
      }
    }
    if (t0 + TK < Ts) fetch(t0 + TK);        // in flight while this tile is computed
    __syncthreads();
    {
      // per (query, key): four interleaved partial sums (shorter chains: less rounding), the scale once at the end
      float d[NSC][4];
#pragma unroll
      for (int k = 0; k < NSC; ++k) d[k][0] = d[k][1] = d[k][2] = d[k][3] = 0.f;
      for (int c = 0; c < DK; c += 4) {
        const float k0 = s_k[sj][c], k1 = s_k[sj][c + 1], k2 = s_k[sj][c + 2], k3 = s_k[sj][c + 3];
#pragma unroll
        for (int k = 0; k < NSC; ++k) {
          const int w = sw + k * SSTEP;
          d[k][0] = fmaf(s_q[w][c], k0, d[k][0]);
          d[k][1] = fmaf(s_q[w][c + 1], k1, d[k][1]);
          d[k][2] = fmaf(s_q[w][c + 2], k2, d[k][2]);
          d[k][3] = fmaf(s_q[w][c + 3], k3, d[k][3]);
        }
      }
#pragma unroll
      for (int k = 0; k < NSC; ++k) {
        const int w = sw + k * SSTEP;
        s_p[w][sj] = sj < n ? ((d[k][0] + d[k][1]) + (d[k][2] + d[k][3])) * scale : -INFINITY;
      }
    }
    __syncthreads();
    {  // 8 lanes per query (the 8 lanes are neighbours inside one wave)
      const int w = tid >> 3, sub = tid & 7;
      if (w < W) {
        float mx = -INFINITY;
        for (int j = sub; j < TK; j += 8) mx = fmaxf(mx, s_p[w][j]);
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        mx = fmaxf(mx, __shfl_xor(mx, 4));
        const float m_old = s_m[w];
        const float m_new = fmaxf(m_old, mx);   // finite: every tile holds at least one valid key
        float sum = 0.f;
        for (int j = sub; j < TK; j += 8) {
          const float p = expf(s_p[w][j] - m_new);   // (masked: exp(-inf) = 0)
          s_p[w][j] = p;
          sum += p;
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        if (sub == 0) {
          const float a = expf(m_old - m_new);       // (first tile: exp(-inf) = 0)
          s_a[w] = a;
          s_l[w] = s_l[w] * a + sum;
          s_m[w] = m_new;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      acc[i] *= s_a[pw + i * WSTEP];
    }
    for (int j = 0; j < n; ++j) {            // (keys in ascending order into every accumulator)
      const float v = s_v[j][pc];
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        acc[i] = fmaf(s_p[pw + i * WSTEP][j], v, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int w = pw + i * WSTEP;
    if (w < W) out[EMO_ATTN_ROW(w) * dd + h * DK + pc] = from_f32<T>(acc[i] / s_l[w]);
  }
