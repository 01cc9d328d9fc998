// follow_state.inc -- the follower's state as given, and what makes it bad input: a joint outside the limits, a velocity
// or one of the first three rows of a guide pose that is not finite, a progress that is out of range.  Included as a
// statement block by follow.hip and follow_cloud.hip (dls_direction.inc's idiom: the compiler sees the lines each kernel
// wrote out itself).
//   in scope: b, lane, W, limits, q_start, v_init, progress_init (the last two may be NULL), my_poses (problem b's)
//   defines:  float lo[7], hi[7] (the limits), q[7], v[7]; int w, nw, fin (guide pose, steps spent on it, finished);
//             bool bad (wave-uniform)
  float lo[7], hi[7], q[7], v[7];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    lo[j] = limits[2 * j], hi[j] = limits[2 * j + 1];
    q[j] = q_start[(size_t)b * 7 + j];
    v[j] = v_init ? v_init[(size_t)b * 7 + j] : 0.0f;
    bad |= !((q[j] >= lo[j]) & (q[j] <= hi[j])) | !(__builtin_fabsf(v[j]) < __builtin_inff());  // (NaN fails)
  }
  int w = progress_init ? progress_init[(size_t)b * 3 + 0] : 0;
  int nw = progress_init ? progress_init[(size_t)b * 3 + 1] : 0;
  int fin = progress_init ? (progress_init[(size_t)b * 3 + 2] != 0) : 0;
  bad |= (w < 0) | (w >= W) | (nw < 0);
  {
    bool pose_bad = false;
    if (lane < W) {  // lane = guide pose: its first three rows
#pragma unroll
      for (int i = 0; i < 12; ++i) pose_bad |= !(__builtin_fabsf(my_poses[16 * lane + i]) < __builtin_inff());
    }
    bad |= __any(pose_bad) != 0;
  }
