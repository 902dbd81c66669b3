// The body of the fused score + top-k kernels (see csrc/beam_score_step.h), included INSIDE the kernel (text, not a function: both
// kernels compile from the same tokens, and emoasr_beam_scores_topk's to the code it always had).  The including kernel is a
// template over <T> and provides V, k, dec, ldd, lm, ldl, vals, idx, lm_at, lm_lds and mu (float: the weight of row blockIdx.x).
  extern __shared__ float sbuf[];      // [V] the decoder row (f32), later the scores | [16][k] x 2 survivors | (lm_lds) [V] the LM row
  __shared__ float red4[4][16];
  const long m = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* drow = dec + m * ldd;
  const float* lrow = lm ? lm + m * ldl : nullptr;
  // Both rows go to LDS first, four strided elements of each per thread and trip (8 loads in flight): read where they are used,
  // inside three loops of ~V / 1024 dependent trips each, the rows cost ~30 global round trips -- most of the kernel's 41 us.
  // A thread only ever reads back the elements it staged itself (v = tid mod 1024), so no barrier is needed.
  float* slm = (lrow && lm_lds) ? sbuf + V + 32 * k : nullptr;
  for (int v0 = tid; v0 < V; v0 += 4096) {
    float a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = v0 + 1024 * u;
      a[u] = v < V ? to_f32(drow[v]) : 0.f;
      b[u] = (slm && v < V) ? lrow[v] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = v0 + 1024 * u;
      if (v < V) { sbuf[v] = a[u]; if (slm) slm[v] = b[u]; }
    }
  }
  const float* lsrc = slm ? slm : lrow;   // (LM row too long for LDS: read from global memory as before)
  // ---- the two log-sum-exps ----
  float mxd = -INFINITY, mxl = -INFINITY;
  for (int v = tid; v < V; v += 1024) {
    mxd = fmaxf(mxd, sbuf[v]);
    if (lrow) mxl = fmaxf(mxl, lsrc[v]);
  }
  for (int o = 32; o > 0; o >>= 1) { mxd = fmaxf(mxd, __shfl_xor(mxd, o)); mxl = fmaxf(mxl, __shfl_xor(mxl, o)); }
  if (lane == 0) { red4[0][wave] = mxd; red4[1][wave] = mxl; }
  __syncthreads();
  mxd = red4[0][0]; mxl = red4[1][0];
  for (int w = 1; w < 16; ++w) { mxd = fmaxf(mxd, red4[0][w]); mxl = fmaxf(mxl, red4[1][w]); }
  float sd = 0.f, sl = 0.f;
  for (int v = tid; v < V; v += 1024) {
    sd += expf(sbuf[v] - mxd);
    if (lrow) sl += expf(lsrc[v] - mxl);
  }
  for (int o = 32; o > 0; o >>= 1) { sd += __shfl_xor(sd, o); sl += __shfl_xor(sl, o); }
  if (lane == 0) { red4[2][wave] = sd; red4[3][wave] = sl; }
  __syncthreads();
  sd = 0.f; sl = 0.f;
  for (int w = 0; w < 16; ++w) { sd += red4[2][w]; sl += red4[3][w]; }
  const float lsed = mxd + logf(sd), lsel = lrow ? mxl + logf(sl) : 0.f;
  // ---- scores; local best of this thread's elements ----
  // Two levels, so that a round costs no workgroup barrier: every wave selects the k best of its own lanes' elements (a round = two
  // DPP reductions -- the maximum, then the lowest index among the lanes that hold it -- and a rescan of the lanes' elements),
  // then wave 0 merges the 16 x k survivors the same way.  The elements being rescanned sit in REGISTERS (V <= 16 K, k <= 32;
  // beyond that the LDS copies are walked): a rescan loop over LDS with a run-time trip count waits ~130 cycles per element for
  // one useful lane, which -- not the reductions, the barrier or the global loads -- was 2 us per round (42 us at k = 15).
  constexpr int NE = 16, NM = 8;
  const bool e_regs = V <= NE * 1024;
  float lb = -INFINITY; int li = 0x7fffffff;
  float e[NE];
  if (e_regs) {
#pragma unroll
    for (int u = 0; u < NE; ++u) {
      const int v = tid + 1024 * u;
      e[u] = -INFINITY;
      if (v < V) {
        float r = sbuf[v] - lsed;
        if (lrow) r += mu * (lsrc[v] - lsel);
        e[u] = r;
        if (r > lb) { lb = r; li = v; }   // ascending v: ties keep the lower index
      }
    }
  } else {
    for (int v = tid; v < V; v += 1024) {
      float r = sbuf[v] - lsed;
      if (lrow) r += mu * (lsrc[v] - lsel);
      sbuf[v] = r;
      if (r > lb) { lb = r; li = v; }
    }
  }
  float* cand_v = sbuf + V;                              // [16][k] survivors of the waves (dynamic LDS after the score row)
  int* cand_i = reinterpret_cast<int*>(cand_v + 16 * k);
  for (int j = 0; j < k; ++j) {
    const float best = topk_wave_max(lb);
    const int bi = topk_wave_min(lb == best ? li : 0x7fffffff);
    if (lane == 0) { cand_v[wave * k + j] = best; cand_i[wave * k + j] = bi; }
    if (e_regs) {   // every lane: drop the winner if it is mine, take the best of what is left
      lb = -INFINITY; li = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < NE; ++u) {
        if (tid + 1024 * u == bi) e[u] = -INFINITY;
        if (e[u] > lb) { lb = e[u]; li = tid + 1024 * u; }
      }
    } else if (bi != 0x7fffffff && (bi & 1023) == tid) {
      sbuf[bi] = -INFINITY;
      lb = -INFINITY; li = 0x7fffffff;
      for (int v = tid; v < V; v += 1024) {
        const float c = sbuf[v];
        if (c > lb) { lb = c; li = v; }
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    // lane owns survivors lane, lane + 64, ... of the 16 k (indices are unique; -inf / 0x7fffffff entries are never picked)
    const int n = 16 * k;
    const bool m_regs = n <= NM * 64;
    float cv[NM]; int ci[NM];
#pragma unroll
    for (int u = 0; u < NM; ++u) {
      const int c = lane + 64 * u;
      cv[u] = (m_regs && c < n) ? cand_v[c] : -INFINITY;
      ci[u] = (m_regs && c < n) ? cand_i[c] : 0x7fffffff;
    }
    float mb = -INFINITY; int mi = 0x7fffffff;
    auto rescan = [&]() {
      mb = -INFINITY; mi = 0x7fffffff;
      if (m_regs) {
#pragma unroll
        for (int u = 0; u < NM; ++u)
          if (cv[u] > mb || (cv[u] == mb && ci[u] < mi)) { mb = cv[u]; mi = ci[u]; }
      } else {
        for (int c = lane; c < n; c += 64) {
          const float xv = cand_v[c];
          const int xi = cand_i[c];
          if (xv > mb || (xv == mb && xi < mi)) { mb = xv; mi = xi; }
        }
      }
    };
    rescan();
    for (int j = 0; j < k; ++j) {
      const float best = topk_wave_max(mb);
      int bi = topk_wave_min(mb == best ? mi : 0x7fffffff);
      if (bi != 0x7fffffff) {
        if (m_regs) {
#pragma unroll
          for (int u = 0; u < NM; ++u)
            if (ci[u] == bi) { cv[u] = -INFINITY; ci[u] = 0x7fffffff; }
        } else {
          for (int c = lane; c < n; c += 64)
            if (cand_i[c] == bi) { cand_v[c] = -INFINITY; cand_i[c] = 0x7fffffff; }
        }
        rescan();
      }
      if (bi == 0x7fffffff) bi = 0;
      if (lane == 0) {
        vals[m * k + j] = best;
        idx[m * k + j] = bi;
        if (lm_at) lm_at[m * k + j] = lrow ? lsrc[bi] - lsel : 0.f;   // (from the LDS copy: a global load here was a round trip per round)
      }
    }
  }
