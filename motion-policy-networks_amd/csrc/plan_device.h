// plan_device.h -- the pieces of the covariant-gradient planner that do not depend on what the environment is made of:
// shared by plan.hip (cuboids and cylinders) and cloud_field.hip (a distance field of a point cloud).  Every function
// states one clause of mpx_franka_plan's contract (include/mpinets_hip.h) and is inlined into its caller.
#pragma once
#include "franka_device.h"
#include "philox.h"

enum { STREAM_PLAN = 14 };
enum { PLAN_BIT_ENV = 1, PLAN_BIT_SELF = 2, PLAN_BIT_JERK = 4 };

// joint limits and the endpoints of problem b -> an endpoint lies outside the limits (NaN fails both comparisons).
// (& and | on purpose: all four operands are loaded either way, and with && / || here franka_plan_cloud_kernel spills
// 8 SGPRs that it does not spill otherwise -- profiles/franka_device_isa.md)
__device__ __forceinline__ bool plan_endpoints(const float *limits, const float *q_start, const float *q_goal, int b,
                                               float (&lo)[7], float (&hi)[7], float (&qs)[7], float (&qg)[7]) {
  bool bad_end = false;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    lo[j] = limits[2 * j], hi[j] = limits[2 * j + 1];
    qs[j] = q_start[(size_t)b * 7 + j], qg[j] = q_goal[(size_t)b * 7 + j];
    bad_end |= !((qs[j] >= lo[j]) & (qs[j] <= hi[j])) | !((qg[j] >= lo[j]) & (qg[j] <= hi[j]));
  }
  return bad_end;
}

// M[t,u] = min(t,u) (n + 1 - max(t,u)) / (n + 1): an exact integer product, one division
__device__ __forceinline__ void plan_fill_metric(float *Mtab, int T, int n) {
  for (int i = threadIdx.x; i < T * T; i += blockDim.x) {
    const int a = i / T, c = i - a * T;
    const int mn = a < c ? a : c, mx = a < c ? c : a;
    Mtab[i] = (float)(mn * (n + 1 - mx)) / (float)(n + 1);
  }
}

// waypoint t of candidate k of global problem `gid`: the line L and the drawn start q
__device__ __forceinline__ void plan_candidate(int k, int t, int T, uint32_t gid, uint32_t seed_lo, uint32_t seed_hi,
                                               float spread, const float (&qs)[7], const float (&qg)[7],
                                               const float (&lo)[7], const float (&hi)[7], float (&L)[7], float (&q)[7]) {
  const float s = (float)t / (float)(T - 1);
  float bump, unused;
  mpx_sincos(3.14159265358979323846f * s, bump, unused);
  const Philox p0 = philox4x32(2u * (uint32_t)k, gid, STREAM_PLAN, 0u, seed_lo, seed_hi);
  const Philox p1 = philox4x32(2u * (uint32_t)k + 1u, gid, STREAM_PLAN, 0u, seed_lo, seed_hi);
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const float line = mpx_fma(s, qg[j] - qs[j], qs[j]);
    L[j] = t == 0 ? qs[j] : t == T - 1 ? qg[j] : line;
    const float u = u01(j < 4 ? p0.c[j] : p1.c[j - 4]);
    const float delta = (spread * mpx_fma(2.0f, u, -1.0f)) * ((hi[j] - lo[j]) * 0.5f);
    const float moved = fminf(fmaxf(mpx_fma(bump, delta, L[j]), lo[j]), hi[j]);
    q[j] = (k == 0 || t == 0 || t == T - 1) ? L[j] : moved;
  }
}

// one joint's share of a sphere's gradient: w . (z_j x (x - o_j)) for the joints j < nj upstream of the sphere's link
template <int nj>
__device__ __forceinline__ void plan_joint_terms(const float (&o)[7][3], const float (&z)[7][3], float x, float y, float zz,
                                                 float wx, float wy, float wz, float (&g)[7]) {
#pragma unroll
  for (int j = 0; j < nj; ++j) {
    const float rx = x - o[j][0], ry = y - o[j][1], rz = zz - o[j][2];
    const float cx = mpx_fma(z[j][1], rz, -(z[j][2] * ry));
    const float cy = mpx_fma(z[j][2], rx, -(z[j][0] * rz));
    const float cz = mpx_fma(z[j][0], ry, -(z[j][1] * rx));
    g[j] += mpx_fma(wz, cz, mpx_fma(wy, cy, wx * cx));
  }
}

// row t of M g, g of the interior waypoints u = 1..n in buf[u * 7 + j], u ascending
__device__ __forceinline__ void plan_metric_product(const float *Mtab, const float *buf, int T, int n, int t,
                                                    float (&acc)[7]) {
  for (int u = 1; u <= n; ++u) {
    const float m = Mtab[u * T + t];
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[j] = mpx_fma(m, buf[u * 7 + j], acc[j]);
  }
}

// q_t <- clamp(q_t - step (smooth_weight (q_t - L_t) + (M g)_t), lo, hi)
__device__ __forceinline__ void plan_update(float step, float smooth_weight, const float (&acc)[7], const float (&L)[7],
                                            const float (&lo)[7], const float (&hi)[7], float (&q)[7]) {
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const float dir = mpx_fma(smooth_weight, q[j] - L[j], acc[j]);
    q[j] = fminf(fmaxf(mpx_fma(-step, dir, q[j]), lo[j]), hi[j]);
  }
}

// PLAN_BIT_JERK of the third differences that start at waypoint `lane` (the trajectory in buf[t * 7 + j])
__device__ __forceinline__ int plan_jerk_bits(const float *buf, int lane, int T, float max_jerk) {
  int bits = 0;
  if (lane + 3 < T) {
    const float lim = max_jerk * MPX_PLAN_JERK_SHARE;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float q0 = buf[lane * 7 + j], q1 = buf[(lane + 1) * 7 + j], q2 = buf[(lane + 2) * 7 + j],
                  q3 = buf[(lane + 3) * 7 + j];
      const float v0 = q1 - q0, v1 = q2 - q1, v2 = q3 - q2;
      const float jerk = (v2 - v1) - (v1 - v0);
      if (!(__builtin_fabsf(jerk) <= lim)) bits |= PLAN_BIT_JERK;
    }
  }
  return bits;
}

// refined configuration r = seg substeps + i of the trajectory in buf: fma((float)i / (float)substeps, q_{seg+1} - q_seg, q_seg)
__device__ __forceinline__ void plan_refined(const float *buf, int r, int substeps, float (&qq)[7]) {
  const int seg = r / substeps, i = r - seg * substeps;
  if (i == 0) {
#pragma unroll
    for (int j = 0; j < 7; ++j) qq[j] = buf[seg * 7 + j];
  } else {
    const float f = (float)i / (float)substeps;
#pragma unroll
    for (int j = 0; j < 7; ++j) qq[j] = mpx_fma(f, buf[(seg + 1) * 7 + j] - buf[seg * 7 + j], buf[seg * 7 + j]);
  }
}

// PLAN_BIT_SELF of one configuration (the frames of the self model are all the FK the compiler keeps).  (Its own walk: through
// plan.hip's plan_config_bits without an environment cloud_field.hip's planner was 0.6 - 1.3 % slower,
// profiles/franka_device_timing.md)
__device__ __forceinline__ int plan_self_bits(const float *q, float finger, float self_margin) {
  int bits = 0;
  franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
    constexpr int id = decltype(ID)::value;
    if constexpr (franka_self_sphere(id) >= 0) {
      if (franka_self_hit<id>(g, self_margin)) bits |= PLAN_BIT_SELF;
    }
  });
  return bits;
}
