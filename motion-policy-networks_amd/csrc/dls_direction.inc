// dls_direction.inc -- dq = J^T (J J^T + lambda^2 I)^-1 e with e = [pt - p ; rotvec(Rt R^T)] and the geometric Jacobian
// J[:, j] = [z_j x (p - o_j) ; z_j], through an unrolled 6x6 Cholesky (A = J J^T + lambda^2 I = L L^T, positive definite for
// lambda > 0: no pivoting), and the scale that makes max |dq_j scale| <= step_clip.  Included as a statement block by
// ik.hip and follow.hip (franka_live_rows.inc's idiom: as an inline function franka_ik_kernel came out with 1736 other
// instruction lines of 3300; included, the compiler sees the lines it saw when the kernel wrote them out).
//   in scope: float o[7][3], z[7][3] (origin and z axis of the seven joint frames), Rigid eff (right_gripper), Rt[9], pt[3]
//             (the target), lam2
//   DLS_STEP_CLIP: the largest joint step
//   defines:  float dq[7], scale -- the step is dq[j] * scale
    float e[6];
    {
      float w[3];
      ik_rotvec(Rt, eff.r, w);
#pragma unroll
      for (int i = 0; i < 3; ++i) e[i] = pt[i] - eff.t[i], e[3 + i] = w[i];
    }
    float J[6][7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float dx = eff.t[0] - o[j][0], dy = eff.t[1] - o[j][1], dz = eff.t[2] - o[j][2];
      J[0][j] = mpx_fma(z[j][1], dz, -(z[j][2] * dy));
      J[1][j] = mpx_fma(z[j][2], dx, -(z[j][0] * dz));
      J[2][j] = mpx_fma(z[j][0], dy, -(z[j][1] * dx));
      J[3][j] = z[j][0], J[4][j] = z[j][1], J[5][j] = z[j][2];
    }
    // A = J J^T + lambda^2 I = L L^T (lower triangle in place), then L y' = e, L^T y = y'
    float L[6][6], inv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = 0; k <= i; ++k) {
        float acc = i == k ? lam2 : 0.0f;
#pragma unroll
        for (int j = 0; j < 7; ++j) acc = mpx_fma(J[i][j], J[k][j], acc);
        L[i][k] = acc;
      }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      float d = L[k][k];
#pragma unroll
      for (int m = 0; m < k; ++m) d = mpx_fma(-L[k][m], L[k][m], d);
      const float root = sqrtf(d);
      inv[k] = 1.0f / root;
      L[k][k] = root;
#pragma unroll
      for (int i = k + 1; i < 6; ++i) {
        float v = L[i][k];
#pragma unroll
        for (int m = 0; m < k; ++m) v = mpx_fma(-L[i][m], L[k][m], v);
        L[i][k] = v * inv[k];
      }
    }
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      float v = e[i];
#pragma unroll
      for (int m = 0; m < i; ++m) v = mpx_fma(-L[i][m], y[m], v);
      y[i] = v * inv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      float v = y[i];
#pragma unroll
      for (int m = i + 1; m < 6; ++m) v = mpx_fma(-L[m][i], y[m], v);
      y[i] = v * inv[i];
    }
    float dq[7], big = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      float v = 0.0f;
#pragma unroll
      for (int i = 0; i < 6; ++i) v = mpx_fma(J[i][j], y[i], v);
      dq[j] = v;
      big = fmaxf(big, __builtin_fabsf(v));
    }
    const float scale = big > (DLS_STEP_CLIP) ? (DLS_STEP_CLIP) / big : 1.0f;
