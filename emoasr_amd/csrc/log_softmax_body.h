// The row reduction of log_softmax_kernel (csrc/decoder.hip) and log_softmax_rows_to_kernel (csrc/lm_tree.hip), included inside both:
// a 256-thread workgroup over `row` (const T*, V columns), `red` its float[16] in LDS.  Leaves `lse`; a column's result is
// to_f32(row[v]) - lse.  One body, so that the rows of both kernels are bit-equal.
  float mx = -INFINITY;
  for (int v = threadIdx.x; v < V; v += 256) mx = fmaxf(mx, to_f32(row[v]));
  mx = block_max(mx, red);
  float se = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) se += expf(to_f32(row[v]) - mx);
  se = block_sum(se, red);
  const float lse = mx + logf(se);
