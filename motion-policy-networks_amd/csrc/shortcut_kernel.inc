// shortcut_kernel.inc -- the body of a shortcut kernel, from the caller's polyline to the returned one: the row check, the
// length before, `passes` passes of (reverse on odd passes | densify to <= P points | greedy furthest-free-chord walk with a
// K-ary search | reverse back), the length after, points_out / count_out / the trace.  The clauses "Pass", "Densify", "Greedy"
// and the outputs of mpx_franka_shortcut's contract (include/mpinets_hip.h), which mpx_gripper_shortcut's refers to.  Included
// as a statement block by roadmap.hip and roadmap_cloud.hip (joint space: the seed trajectory's statements, roadmap_traj.inc,
// follow it) and by gripper_shortcut.hip and gripper_shortcut_cloud.hip (SE(3): the guide poses, gripper_poses.inc, follow it).
//   in scope: b, tid, opt (.points, .passes, .fanout, .resolution), Pin, nan, inf, the operands points, count and the outputs
//             status, points_out, count_out, length, chords_out, configs_out; in LDS float *poly (2 x P x 7), *dist (2 P),
//             int *path, *sel, *pidx, *pieces, *blocked (P each), *off, *first (P + 1 each), *ctl (4); the helpers of
//             roadmap_device.h
//   the hooks roadmap_search.inc has -- SHORTCUT_LENGTH(a, e): the length of the segment between the vertices float a[7], e[7];
//             SHORTCUT_POINT(a, e, f, q): float q[7] (registers or LDS) = the point at fraction f from a toward e; SHORTCUT_HIT(q): q is invalid --
//             and, where a vertex can be bad beyond "not finite", SHORTCUT_VERTEX_BAD(v)
//   leaves:   st (0 or 2), n (the vertices returned, 0 with st 2), float *cur (the returned polyline), P, path[i] = i
// Three mappings: thread = vertex (load, reverse, densify, copy), thread = interior configuration across the concatenated
// chords of one probe level (roadmap_search.inc's first[] prefix mapping), thread = output row (what follows).  The anchor
// walk, the probes and the prefix sums are serial on thread 0.  Every branch around a barrier is workgroup-uniform: it reads
// a value from LDS behind a barrier, a kernel argument, or a barrier's own reduction.
const int P = opt.points;
const int cnt = count[b];
float *cur = poly, *oth = poly + P * 7;
bool broken = cnt < 2 || cnt > Pin;
if (tid < P) path[tid] = tid;  // (what follows walks nodes[path[i]]: the returned polyline in its own order)
if (!broken && tid < cnt) {
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const float v = points[((size_t)b * Pin + tid) * 7 + j];
    cur[tid * 7 + j] = v;
    broken |= !(fabsf(v) < inf);
  }
#ifdef SHORTCUT_VERTEX_BAD
  broken |= SHORTCUT_VERTEX_BAD((cur + tid * 7));
#endif
}
const int st = __syncthreads_or(broken) ? 2 : 0;  // (publishes the polyline and path[])
int n = st == 0 ? cnt : 0;                        // the vertices of the current polyline
int n_chords = 0, n_configs = 0;                  // (thread 0's)
float before = nan, after = nan;
if (st == 0) {
  if (tid == 0) {
    before = 0.0f;
    for (int i = 0; i + 1 < n; ++i) before += SHORTCUT_LENGTH((cur + i * 7), (cur + (i + 1) * 7));
  }
  for (int pass = 0; pass < opt.passes && n > 2; ++pass) {
    const bool backward = (pass & 1) != 0;
    if (backward) {  // thread = vertex
      if (tid < n) {
#pragma unroll
        for (int j = 0; j < 7; ++j) oth[tid * 7 + j] = cur[(n - 1 - tid) * 7 + j];
      }
      __syncthreads();
      float *swap = cur;
      cur = oth, oth = swap;
    }
    // ---- densify: cur (n vertices) -> oth (N <= P points); off[i] is where vertex i lands ----------------------------------
    if (tid == 0) {
      float *w = dist;
      float L = 0.0f;
      for (int i = 0; i + 1 < n; ++i) {
        w[i] = SHORTCUT_LENGTH((cur + i * 7), (cur + (i + 1) * 7));
        L += w[i];
      }
      const int extra = P - n;
      int left = (L > 0.0f && L < inf && extra > 0) ? extra : 0;
      off[0] = 0;
      for (int i = 0; i + 1 < n; ++i) {
        const float x = floorf(w[i] * (float)extra / L);
        const int m = left == 0 ? 0 : x >= (float)left ? left : x >= 1.0f ? (int)x : 0;
        left -= m;
        off[i + 1] = off[i] + 1 + m;
      }
      ctl[1] = off[n - 1] + 1;
    }
    __syncthreads();
    const int N = ctl[1];
    if (tid < N) {  // thread = dense point: on the last edge i with off[i] <= tid (the last vertex is its own)
      int i = 0, top = n;
      while (top - i > 1) {
        const int mid = (i + top) >> 1;
        if (off[mid] <= tid) i = mid; else top = mid;
      }
      const int k = tid - off[i];
      if (k == 0) {
#pragma unroll
        for (int j = 0; j < 7; ++j) oth[tid * 7 + j] = cur[i * 7 + j];
      } else {
        const float f = (float)k / (float)(off[i + 1] - off[i]);
        SHORTCUT_POINT((cur + i * 7), (cur + (i + 1) * 7), f, (oth + tid * 7))
      }
    }
    __syncthreads();
    // ---- greedy: sel[] = the dense points kept.  One iteration is one probe level: thread 0 reads the level before,
    // moves the anchor while nothing is left to search, lays out the next level's chords; everyone tests them ---------------
    const float *D = oth;
    int a = 0, lo = 1, hi = N - 1, kept = 1, level = 0;  // (thread 0's)
    if (tid == 0) sel[0] = 0;
    for (;;) {
      if (tid == 0) {
        if (level > 0) {
          if (!blocked[level - 1]) {
            lo = hi;
          } else {
            int best = -1;
            for (int i = 0; i + 1 < level; ++i)
              if (!blocked[i]) best = i;
            if (best >= 0) lo = pidx[best];
            hi = pidx[best + 1] - 1;
          }
        }
        level = 0;
        bool done = false;
        while (hi <= lo) {  // nothing left to search: lo is the furthest point known to be reachable from a
          sel[kept++] = lo;
          a = lo;
          if (a == N - 1) {
            done = true;
            break;
          }
          lo = a + 1, hi = N - 1;
        }
        if (!done) {
          const int span = hi - lo, K = opt.fanout;
          first[0] = 0;
          for (int k = 1; k <= K; ++k) {
            const int pr = lo + (span * k + K - 1) / K;
            if (level > 0 && pidx[level - 1] == pr) continue;
            pidx[level] = pr;
            pieces[level] = roadmap_pieces(SHORTCUT_LENGTH((D + a * 7), (D + pr * 7)), opt.resolution);
            first[level + 1] = first[level] + pieces[level] - 1;
            blocked[level] = 0;
            ++level;
          }
          n_chords += level, n_configs += first[level];
        }
        ctl[0] = kept, ctl[2] = level, ctl[3] = a;
      }
      __syncthreads();
      const int probes = ctl[2];
      if (probes == 0) break;
      const float *qa = D + ctl[3] * 7;
      const int total = first[probes];
      for (int c = tid; c < total; c += ROADMAP_THREADS) {  // thread = interior configuration
        int i = 0, top = probes;                            // the last chord with first[i] <= c
        while (top - i > 1) {
          const int mid = (i + top) >> 1;
          if (first[mid] <= c) i = mid; else top = mid;
        }
        const float *qe = D + pidx[i] * 7;
        const float f = (float)(c - first[i] + 1) / (float)pieces[i];
        float q[7];
        SHORTCUT_POINT(qa, qe, f, q)
        if (SHORTCUT_HIT(q)) blocked[i] = 1;  // (every lane that stores, stores 1)
      }
      __syncthreads();
    }
    n = ctl[0];
    if (tid < n) {  // thread = vertex kept
#pragma unroll
      for (int j = 0; j < 7; ++j) cur[tid * 7 + j] = D[sel[tid] * 7 + j];
    }
    __syncthreads();
    if (backward) {
      if (tid < n) {
#pragma unroll
        for (int j = 0; j < 7; ++j) oth[tid * 7 + j] = cur[(n - 1 - tid) * 7 + j];
      }
      __syncthreads();
      float *swap = cur;
      cur = oth, oth = swap;
    }
  }
  if (tid == 0) {
    after = 0.0f;
    for (int i = 0; i + 1 < n; ++i) after += SHORTCUT_LENGTH((cur + i * 7), (cur + (i + 1) * 7));
  }
}

// ---- what goes out -----------------------------------------------------------------------------------------------------------
if (tid == 0) {
  status[b] = st, count_out[b] = n;
  length[2 * (size_t)b] = before, length[2 * (size_t)b + 1] = after;
  if (chords_out) chords_out[b] = n_chords;
  if (configs_out) configs_out[b] = n_configs;
}
for (int i = tid; i < P * 7; i += ROADMAP_THREADS) points_out[(size_t)b * P * 7 + i] = i < n * 7 ? cur[i] : nan;
