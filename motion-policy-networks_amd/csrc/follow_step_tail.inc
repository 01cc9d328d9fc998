// follow_step_tail.inc -- steps 6 and 7 of one time step of the follower: the acceleration, the integration (position
// first, then the velocity), the clamp into the limits, the arc length, and lane 0's store of the dense path.  Included as
// a statement block INSIDE the time loop of follow.hip and follow_cloud.hip, behind the kernel's own obstacle term
// (dls_direction.inc's idiom).
//   in scope: i (the step, from 1), lane, opt, lo[7], hi[7], q[7], v[7], u[7] (the attractor), g[7] (the obstacle
//             gradient), total, nw, n, P, A (problem b's rows of path and arc)
//   updates:  q, v, total (the arc length so far), nw, n = i; writes P[i], A[i]
    // 6. the acceleration, 7. position first, then the velocity; the clamp into the limits stops a joint
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float barrier = fmaxf(0.0f, (lo[j] + opt.limit_band) - q[j]) - fmaxf(0.0f, q[j] - (hi[j] - opt.limit_band));
      const float a = ((opt.attract * u[j] - opt.repel * g[j]) + opt.limit_gain * barrier) - opt.damping * v[j];
      const float moved = q[j] + opt.dt * v[j];
      float vn = fminf(fmaxf(v[j] + opt.dt * a, -opt.speed_limit), opt.speed_limit);
      const float qn = fminf(fmaxf(moved, lo[j]), hi[j]);
      if (qn != moved) vn = 0.0f;
      const float dj = qn - q[j];
      ss = j == 0 ? dj * dj : mpx_fma(dj, dj, ss);
      q[j] = qn, v[j] = vn;
    }
    total += sqrtf(ss);
    ++nw;
    n = i;
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 7; ++j) P[(size_t)i * 7 + j] = q[j];
      A[i] = total;
    }
