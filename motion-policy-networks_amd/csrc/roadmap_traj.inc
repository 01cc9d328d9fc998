// roadmap_traj.inc -- the seed trajectory of a polyline in joint space: the planner's line for a one-edge polyline; else
// the polyline resampled by arc length to T waypoints and rounded by opt.smooth_passes passes of (1/4, 1/2, 1/4).  The
// clause "traj" of mpx_franka_roadmap's contract (include/mpinets_hip.h).  Included as a statement block, last in the
// kernel, by roadmap_tail.inc (the roadmap kernels: the polyline is the path found) and, behind shortcut_kernel.inc, by the
// two joint-space shortcut kernels of roadmap.hip and roadmap_cloud.hip (the polyline returned); the compiler sees the lines it saw when roadmap_tail.inc wrote them out (profiles/shortcut_timing.md has the
// instruction-stream comparison).
//   in scope: b, tid, T, nan, st (0: there is a polyline), hops (its edges), V, opt (.smooth_passes), float *nodes and
//             int *path (vertex i is nodes[path[i]]), qs[7], qg[7] (its ends), float *dist (2 V), float *tbuf (2 x 64 x 7),
//             and the kernel's output traj
  // ---- the seed trajectory: thread = waypoint ------------------------------------------------------------------------------------
  float *out = traj + (size_t)b * T * 7;
  if (st != 0) {
    for (int i = tid; i < T * 7; i += ROADMAP_THREADS) out[i] = nan;
    return;
  }
  const bool end = tid == 0 || tid == T - 1;
  if (hops == 1) {  // the planner's line itself
    if (tid < T) {
      const float s = (float)tid / (float)(T - 1);
#pragma unroll
      for (int j = 0; j < 7; ++j)
        out[tid * 7 + j] = tid == 0 ? qs[j] : tid == T - 1 ? qg[j] : mpx_fma(s, qg[j] - qs[j], qs[j]);
    }
    return;
  }
  float *cum = dist, *len = dist + V;  // (the search is over: cum[i] = arc length at path node i, len[i] = |edge i|)
  __syncthreads();
  if (tid == 0) {
    cum[0] = 0.0f;
    for (int i = 0; i < hops; ++i) {
      len[i] = roadmap_length(nodes + path[i] * 7, nodes + path[i + 1] * 7);
      cum[i + 1] = cum[i] + len[i];
    }
  }
  __syncthreads();
  if (tid < T) {
    const float s = ((float)tid / (float)(T - 1)) * cum[hops];
    int i = 0;
    for (int e = 1; e < hops; ++e)
      if (cum[e] <= s) i = e;
    const float f = len[i] > 0.0f ? fminf((s - cum[i]) / len[i], 1.0f) : 0.0f;
    const float *pa = nodes + path[i] * 7, *pb = nodes + path[i + 1] * 7;
#pragma unroll
    for (int j = 0; j < 7; ++j) tbuf[tid * 7 + j] = tid == 0 ? qs[j] : tid == T - 1 ? qg[j] : mpx_fma(f, pb[j] - pa[j], pa[j]);
  }
  __syncthreads();
  float *src = tbuf, *dst = tbuf + 64 * 7;
  for (int pass = 0; pass < opt.smooth_passes; ++pass) {  // (1/4, 1/2, 1/4) on the interior, each pass from the previous one
    if (tid < T) {
#pragma unroll
      for (int j = 0; j < 7; ++j)
        dst[tid * 7 + j] = end ? src[tid * 7 + j]
                               : mpx_fma(0.25f, src[(tid - 1) * 7 + j] + src[(tid + 1) * 7 + j], 0.5f * src[tid * 7 + j]);
    }
    __syncthreads();
    float *swap = src;
    src = dst, dst = swap;
  }
  if (tid < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) out[tid * 7 + j] = src[tid * 7 + j];
  }
