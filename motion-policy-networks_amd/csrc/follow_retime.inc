// follow_retime.inc -- the follower's retiming: lane = output waypoint, at its share of the dense path's arc length, found by
// a bisection of fixed length over arc[] and interpolated between the two steps round it.  Included as a statement block
// by follow.hip and follow_cloud.hip behind the barrier that ends the time loop (dls_direction.inc's idiom).
//   in scope: lane, T, n (steps taken), total (their arc length), q[7] (the state: path[n]), P, A (problem b's rows of
//             path and arc, rows 0 .. n written)
//   defines:  int t (this lane's waypoint), float qt[7] (its configuration)
  const int t = lane < T ? lane : T - 1;  // (lanes past the trajectory repeat the last waypoint and never store)
  float qt[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) qt[j] = q[j];  // waypoint T-1 is path[n], the state itself; with n = 0 every waypoint is
  if (n > 0 && t < T - 1) {
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < 7; ++j) qt[j] = P[j];
    } else {
      const float st = ((float)t / (float)(T - 1)) * total;
      int i0 = 0, i1 = n - 1;  // arc[i0] <= st (arc[0] = 0); the answer lies in i0 .. i1
      for (int r = 0; r < FOLLOW_BISECT_ROUNDS; ++r) {
        if (i0 < i1) {
          const int mid = (i0 + i1 + 1) >> 1;
          if (A[mid] <= st)
            i0 = mid;
          else
            i1 = mid - 1;
        }
      }
      const float a0 = A[i0], den = A[i0 + 1] - a0;
      const float frac = den > 0.0f ? fminf(fmaxf((st - a0) / den, 0.0f), 1.0f) : 0.0f;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const float p0 = P[(size_t)i0 * 7 + j];
        qt[j] = mpx_fma(frac, P[(size_t)(i0 + 1) * 7 + j] - p0, p0);
      }
    }
  }
