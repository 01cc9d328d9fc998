// dls_device.h -- the damped-least-squares direction toward a right_gripper pose, stated once for ik.hip (64 starts, one
// per lane) and follow.hip (the attractor of the follower, one state per wave): the rotation vector of the orientation
// error here, and the Jacobian and the 6x6 solve as a statement block in dls_direction.inc.
#pragma once
#include "franka_device.h"

// rotvec of E = A B^T (row-major 3x3 each): w = sin(theta) axis from the antisymmetric part, theta = atan2(|w|, cos).
// Returns theta.  (|w| -> 0 with cos < 0, a half turn about an unknown axis, yields a zero vector: such a lane moves on
// its position error and leaves the half turn within a step.)
__device__ __forceinline__ float ik_rotvec(const float *a, const float *b, float (&w)[3]) {
  float E[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      E[3 * i + k] = mpx_fma(a[3 * i + 2], b[3 * k + 2], mpx_fma(a[3 * i + 1], b[3 * k + 1], a[3 * i] * b[3 * k]));
  w[0] = 0.5f * (E[7] - E[5]);
  w[1] = 0.5f * (E[2] - E[6]);
  w[2] = 0.5f * (E[3] - E[1]);
  const float c = 0.5f * ((E[0] + E[4] + E[8]) - 1.0f);
  const float s = sqrtf(mpx_fma(w[2], w[2], mpx_fma(w[1], w[1], w[0] * w[0])));
  const float theta = atan2f(s, c);
  const float k = s > 1e-7f ? theta / s : 1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] *= k;
  return theta;
}
