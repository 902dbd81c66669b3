// The body of the CTC prefix scorer kernels (see csrc/beam_score_step.h), included INSIDE the kernel (text, not a function: all
// kernels compile from the same tokens, and the existing ones to the code they always had).  The including kernel provides the
// constant RAGGED, the parameters Tn, V, cw, x, prev_states, cw_prev, parent, pcand, init_state, last, out_len, cands, blank, eos,
// log_psi, states, xoff, W, and the macro EMO_CTC_FRAMES_OF(s) -> the index into xoff of search s's frames.
  __shared__ float s_rn[64], s_rb[64];
  const int m = blockIdx.x / cw, c = blockIdx.x % cw, lane = threadIdx.x;
  const float* rp = prev_states ? prev_states + ((long)parent[m] * cw_prev + pcand[m]) * Tn * 2 : init_state;
  const int tok = cands[m * cw + c];
  const int olen = out_len[m];
  const bool same = olen > 0 && tok == last[m];
  float* r = states + ((long)m * cw + c) * Tn * 2;
  if constexpr (RAGGED) {   // (after the slots are addressed with the common stride)
    const int s = EMO_CTC_FRAMES_OF(m / W);
    x += (long)xoff[s] * V;
    Tn = xoff[s + 1] - xoff[s];
  }
  const int start = olen > 1 ? olen : 1;
  // rows before `start` keep their initial value: LOG_0, except r[0][0] = x[0][tok] for an empty prefix
  for (int t = lane; t < start && t < Tn; t += 64) {
    r[2 * t] = (t == 0 && olen == 0) ? x[tok] : EMO_LOG0;
    r[2 * t + 1] = EMO_LOG0;
  }
  // The three recursions have one shape, v <- logaddexp(v, a_t) + b_t:
  //   lane 0: r^n   a = phi_t            b = x_t[tok]
  //   lane 1: psi   a = phi_t + x_t[tok] b = 0
  //   lane 2: r^b   a = r^n_{t-1}        b = x_t[blank]     (a comes from lane 0, one step behind)
  // so lanes 0..2 run them in lockstep: one logaddexp per frame on the critical path instead of three.
  const float v0 = (start == 1 && olen == 0) ? x[tok] : EMO_LOG0;
  float v = lane == 2 ? EMO_LOG0 : v0;  // rn = psi = v0, rb = LOG_0
  for (int t0 = start; t0 < Tn; t0 += 64) {
    const int t = t0 + lane;
    // lane i keeps frame t0 + i's inputs in registers; the recurrence lanes fetch them with v_readlane (the LDS copies they used
    // to read cost a ~130-cycle round trip per frame on top of the dependent exp / log chain: 53 us at T' 285)
    float my_phi = 0.f, my_x = 0.f, my_xb = 0.f;
    if (t < Tn) {
      const float pn = rp[2 * (t - 1)], pb = rp[2 * (t - 1) + 1];
      my_phi = same ? pb : np_logaddexp(pn, pb);
      my_x = x[(long)t * V + tok];
      my_xb = x[(long)t * V + blank];
    }
    const int n = min(64, Tn - t0);
    for (int i = 0; i < n; ++i) {
      const float rn_prev = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
      const float phi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_phi), i));
      const float xt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_x), i));
      const float xbl = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_xb), i));
      const float a = lane == 0 ? phi : (lane == 1 ? phi + xt : rn_prev);
      const float bb = lane == 0 ? xt : (lane == 1 ? 0.f : xbl);
      if (lane < 3) {
        // same formula as np_logaddexp with the hardware exp / log (v_exp_f32, v_log_f32): |error| < 1e-7 in
        // absolute terms per step against scores of magnitude 10..100 (the library expf / log1pf pair is ~4x
        // the latency of this loop's critical path)
        const float d = v - a;
        v = (d > 0.f ? v + __logf(1.f + __expf(-d)) : a + __logf(1.f + __expf(d))) + bb;
      }
      if (lane == 0) s_rn[i] = v;
      if (lane == 2) s_rb[i] = v;
    }
    __builtin_amdgcn_wave_barrier();
    if (t < Tn) { r[2 * t] = s_rn[lane]; r[2 * t + 1] = s_rb[lane]; }
    __builtin_amdgcn_wave_barrier();
  }
  float psi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 1));
  if (lane == 0) {
    if (tok == eos) psi = np_logaddexp(rp[2 * (Tn - 1)], rp[2 * (Tn - 1) + 1]);
    if (tok == blank) psi = EMO_LOG0;
    log_psi[m * cw + c] = psi;
  }
