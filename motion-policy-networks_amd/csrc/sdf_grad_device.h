// sdf_grad_device.h -- analytic gradients of the single-primitive signed distances of sdf_device.h: the derivative of the
// function those forms EVALUATE (autograd of geometry.py:276-287 / :486-506), not of an ideal distance field.
// sgn / box_grad serve the collision hinge (loss.hip, which exposes this gradient per point: tests/test_gpu_loss_float64.py
// holds it to float64 there) and the trajectory optimiser (plan.hip), which also uses the per-primitive forms below.
#pragma once
#include "sdf_device.h"

__device__ __forceinline__ float sgn(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

// gradient of the 2-norm-of-positive-parts + clamped-max "box" distance w.r.t. d (n = 2 or 3);
// mirrors autograd of geometry.py:276-284 (norm has zero gradient at the origin; max picks the first index)
template <int ND>
__device__ __forceinline__ void box_grad(const float (&d)[ND], float (&g)[ND]) {
  float n2 = 0.0f;
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    float m = fmaxf(d[i], 0.0f);
    n2 = mpx_fma(m, m, n2);
  }
  const float outside = sqrtf(n2);
  int arg = 0;
  float mx = d[0];
#pragma unroll
  for (int i = 1; i < ND; ++i)
    if (d[i] > mx) {
      mx = d[i];
      arg = i;
    }
#pragma unroll
  for (int i = 0; i < ND; ++i) {
    float gi = (outside > 0.0f && d[i] > 0.0f) ? d[i] / outside : 0.0f;
    if (mx < 0.0f && i == arg) gi += 1.0f;
    g[i] = gi;
  }
}

// d(cuboid_sdf_live)/d(local point) at the local point (px, py, pz) = mpx_project(f, world point); dims = full sizes
__device__ __forceinline__ void cuboid_sdf_grad_local(float px, float py, float pz, float dx, float dy, float dz, float &l0,
                                                      float &l1, float &l2) {
  float d[3] = {__builtin_fabsf(px) - dx / 2.0f, __builtin_fabsf(py) - dy / 2.0f, __builtin_fabsf(pz) - dz / 2.0f};
  float g[3];
  box_grad<3>(d, g);
  l0 = g[0] * sgn(px), l1 = g[1] * sgn(py), l2 = g[2] * sgn(pz);
}

// d(cylinder_sdf_live)/d(local point); zero radial part on the axis (rho = 0), as autograd of the norm gives
__device__ __forceinline__ void cylinder_sdf_grad_local(float px, float py, float pz, float radius, float height, float &l0,
                                                        float &l1, float &l2) {
  const float rho = sqrtf(mpx_fma(py, py, px * px));
  float d[2] = {rho - radius, __builtin_fabsf(pz) - height / 2.0f};
  float g[2];
  box_grad<2>(d, g);
  const float ir = rho > 0.0f ? g[0] / rho : 0.0f;
  l0 = ir * px, l1 = ir * py, l2 = g[1] * sgn(pz);
}

// local gradient -> world: M^T l, M = rows 0..2 x cols 0..2 of the STORED inverse frame (not assumed orthonormal: the
// reference's matrix for a quaternion with roll is not a rotation, and the SDF kernels evaluate with it as stored)
__device__ __forceinline__ void sdf_grad_to_world(const float *__restrict__ f, float l0, float l1, float l2, float &gx,
                                                  float &gy, float &gz) {
  gx = mpx_fma(f[8], l2, mpx_fma(f[4], l1, f[0] * l0));
  gy = mpx_fma(f[9], l2, mpx_fma(f[5], l1, f[1] * l0));
  gz = mpx_fma(f[10], l2, mpx_fma(f[6], l1, f[2] * l0));
}
