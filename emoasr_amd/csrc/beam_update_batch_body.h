// The body of the batched beam bookkeeping kernels, included INSIDE the kernel (text, not a function: both kernels compile from
// the same tokens, and emoasr_beam_update_batch's to the code it always had).  The including kernel provides b
// (emoasr_beam_update_batch_t) and the macro EMO_UPDATE_MU(s) -> the f32 LM weight of search s.
// beam_update_kernel (csrc/decode_rt.hip) for search s = blockIdx.x: the same arithmetic in the same order on rows
// s * bw .. s * bw + bw - 1.  n_parent is the GLOBAL row of the parent (emoasr_beam_cache_gather and the CTC scorer index
// all nb rows); n_pcand, the history and res_parent stay local to the search.  The position is the shared word *u.pos: the
// workgroups only read it, the tail kernel advances it after all of them.
  __shared__ float sc[32][32];
  __shared__ int sel_j[32][32];
  __shared__ double cscore[1024];
  __shared__ int c_m[1024], c_j[1024];
  __shared__ int sorted_e[32];
  const emoasr_beam_update_t& u = b.u;
  const int s = blockIdx.x;
  emoasr_beam_state_t* st = u.state + s;
  const int pos = *b.pos;
  if (st->done || pos >= b.max_pos) return;   // (max_pos: the rows of the history and of the caches)
  const int tid = threadIdx.x;
  const int bw = u.bw, cw = u.cw, na = st->n_alive;
  const int R = s * bw;                 // first global row of the search
  const float* vals = u.vals + (long)R * cw;
  const int* cands = u.cands + (long)R * cw;
  const float* psi = u.psi ? u.psi + (long)R * cw : nullptr;
  const float* lm_at = u.lm_at ? u.lm_at + (long)R * cw : nullptr;
  double* score = u.score + R;
  float* score_ctc = u.score_ctc + R;
  const float f1 = u.one_minus_lam, fl = u.lam, fm = EMO_UPDATE_MU(s);
  for (int i = tid; i < na * cw; i += 256) {
    const int m = i / cw, j = i - m * cw;
    float v;
    if (psi) {
      v = f1 * vals[m * cw + j] + fl * (psi[m * cw + j] - score_ctc[m]);
      if (lm_at) v = v + fm * lm_at[m * cw + j];
    } else {
      v = vals[m * cw + j];
    }
    sc[m][j] = v;
  }
  __syncthreads();
  const int keep = min(bw, cw);
  for (int i = tid; i < na * cw; i += 256) {
    const int m = i / cw, j = i - m * cw;
    const float v = sc[m][j];
    int r = 0;
    for (int k = 0; k < cw; ++k) r += (sc[m][k] > v) || (sc[m][k] == v && k < j);
    if (r < keep) sel_j[m][r] = j;
  }
  __syncthreads();
  const int nc = na * keep;
  for (int e = tid; e < nc; e += 256) {
    const int m = e / keep, r = e - m * keep, j = sel_j[m][r];
    c_m[e] = m; c_j[e] = j;
    cscore[e] = score[m] + (double)sc[m][j];
  }
  __syncthreads();
  for (int e = tid; e < nc; e += 256) {
    const double v = cscore[e];
    int r = 0;
    for (int k = 0; k < nc; ++k) r += (cscore[k] > v) || (cscore[k] == v && k < e);
    if (r < bw) sorted_e[r] = e;
  }
  __syncthreads();
  if (tid != 0) return;
  int a = 0, nres = st->n_results;
  const int nsel = min(bw, nc);
  int* hp = u.hist_parent + ((long)pos * b.S + s) * bw;
  int* ht = u.hist_token + ((long)pos * b.S + s) * bw;
  int *n_ids = u.n_ids + R, *n_parent = u.n_parent + R, *n_pcand = u.n_pcand + R;
  for (int r = 0; r < nsel; ++r) {
    const int e = sorted_e[r], m = c_m[e], j = c_j[e];
    const int tok = cands[m * cw + j];
    if (tok == u.eos) {
      if (pos < 1) continue;  // empty hypothesis
      u.res_score[R + nres] = cscore[e] + u.len_weight * (double)(pos + 2);
      u.res_step[R + nres] = pos;
      u.res_parent[R + nres] = m;
      ++nres;
      if (nres >= bw) break;
    } else {
      n_ids[a] = tok; n_parent[a] = R + m; n_pcand[a] = j;
      score[a] = cscore[e];
      score_ctc[a] = psi ? psi[m * cw + j] : 0.f;
      hp[a] = m; ht[a] = tok;
      ++a;
    }
  }
  for (int k = a; k < bw; ++k) {  // unused slots: copies of the search's slot 0
    n_ids[k] = a > 0 ? n_ids[0] : u.eos;
    n_parent[k] = a > 0 ? n_parent[0] : R;
    n_pcand[k] = a > 0 ? n_pcand[0] : 0;
    score[k] = 0.0; score_ctc[k] = 0.f;
    hp[k] = -1; ht[k] = -1;
  }
  for (int k = 0; k < bw; ++k) {
    u.n_last[R + k] = n_ids[k];
    u.n_outlen[R + k] = pos + 1;
    u.n_klens[R + k] = pos + 2;
  }
  st->n_alive = a;
  st->n_results = nres;
  st->done = (nres >= bw || a == 0) ? 1 : 0;
  st->pos = pos + 1;
