// franka_device.h -- the device side of the Franka geometry entries, each piece stated once: the rigid transforms, the
// Panda chain (FK) and the self-collision model.  Device code only; the host side of the same entries is franka_host.h.
#pragma once
#include "common.h"

// 3x4 rigid transform: r[9] row-major rotation, t[3]
struct Rigid {
  float r[9];
  float t[3];
};

__device__ __forceinline__ Rigid rigid_compose(const Rigid &a, const float (&fr)[9], const float (&ft)[3]) {
  Rigid o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float acc = a.r[3 * i + 0] * fr[0 + c];
      acc = mpx_fma(a.r[3 * i + 1], fr[3 + c], acc);
      acc = mpx_fma(a.r[3 * i + 2], fr[6 + c], acc);
      o.r[3 * i + c] = acc;
    }
    float acc = a.t[i];
    acc = mpx_fma(a.r[3 * i + 0], ft[0], acc);
    acc = mpx_fma(a.r[3 * i + 1], ft[1], acc);
    acc = mpx_fma(a.r[3 * i + 2], ft[2], acc);
    o.t[i] = acc;
  }
  return o;
}

__device__ __forceinline__ Rigid rigid_rotz(const Rigid &p, float s, float c) {
  Rigid o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float a = p.r[3 * i + 0], b = p.r[3 * i + 1];
    o.r[3 * i + 0] = mpx_fma(b, s, a * c);
    o.r[3 * i + 1] = mpx_fma(b, c, -(a * s));
    o.r[3 * i + 2] = p.r[3 * i + 2];
    o.t[i] = p.t[i];
  }
  return o;
}

__device__ __forceinline__ void rigid_apply(const float *f /*12*/, float x, float y, float z, float &ox,
                                            float &oy, float &oz) {
  float a0 = f[0] * x;
  a0 = mpx_fma(f[1], y, a0);
  a0 = mpx_fma(f[2], z, a0);
  float a1 = f[3] * x;
  a1 = mpx_fma(f[4], y, a1);
  a1 = mpx_fma(f[5], z, a1);
  float a2 = f[6] * x;
  a2 = mpx_fma(f[7], y, a2);
  a2 = mpx_fma(f[8], z, a2);
  ox = a0 + f[9];
  oy = a1 + f[10];
  oz = a2 + f[11];
}
// the same operations in the same order on a frame held in registers
__device__ __forceinline__ void rigid_apply(const Rigid &g, float x, float y, float z, float &ox, float &oy, float &oz) {
  ox = mpx_fma(g.r[2], z, mpx_fma(g.r[1], y, g.r[0] * x)) + g.t[0];
  oy = mpx_fma(g.r[5], z, mpx_fma(g.r[4], y, g.r[3] * x)) + g.t[1];
  oz = mpx_fma(g.r[8], z, mpx_fma(g.r[7], y, g.r[6] * x)) + g.t[2];
}

// Franka Panda chain (public URDF constants).  `visit(id, frame)` is called once per frame, in chain order
// (0 = link0 ... 8 = link8, 9 hand, 10 / 11 fingers, 12 / 13 fingertips, 14 right_gripper), with the frame in registers:
// a caller that consumes a frame as soon as it exists (the lanes-as-waypoints collision kernel) never stores the chain.
template <class Visit>
__device__ __forceinline__ void franka_fk_visit(const float *q7, float finger, Visit &&visit) {
  constexpr float SH = 0.70710678118654752440f;
  Rigid cur = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  visit(std::integral_constant<int, 0>{}, cur);
  const float JR[7][9] = {
      {1, 0, 0, 0, 1, 0, 0, 0, 1},  {1, 0, 0, 0, 0, 1, 0, -1, 0}, {1, 0, 0, 0, 0, -1, 0, 1, 0},
      {1, 0, 0, 0, 0, -1, 0, 1, 0}, {1, 0, 0, 0, 0, 1, 0, -1, 0}, {1, 0, 0, 0, 0, -1, 0, 1, 0},
      {1, 0, 0, 0, 0, -1, 0, 1, 0},
  };
  const float JT[7][3] = {
      {0.0f, 0.0f, 0.333f},     {0.0f, 0.0f, 0.0f}, {0.0f, -0.316f, 0.0f}, {0.0825f, 0.0f, 0.0f},
      {-0.0825f, 0.384f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.088f, 0.0f, 0.0f},
  };
  auto joint = [&](auto J) __attribute__((always_inline)) {
    constexpr int j = decltype(J)::value;
    float s, c;
    mpx_sincos(q7[j], s, c);
    Rigid tmp = rigid_compose(cur, JR[j], JT[j]);
    cur = rigid_rotz(tmp, s, c);
    visit(std::integral_constant<int, j + 1>{}, cur);
  };
  joint(std::integral_constant<int, 0>{});
  joint(std::integral_constant<int, 1>{});
  joint(std::integral_constant<int, 2>{});
  joint(std::integral_constant<int, 3>{});
  joint(std::integral_constant<int, 4>{});
  joint(std::integral_constant<int, 5>{});
  joint(std::integral_constant<int, 6>{});
  const float I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float T8[3] = {0.0f, 0.0f, 0.107f};
  Rigid l8 = rigid_compose(cur, I3, T8);
  visit(std::integral_constant<int, 8>{}, l8);
  const float RH[9] = {SH, SH, 0, -SH, SH, 0, 0, 0, 1};
  const float Z3[3] = {0.0f, 0.0f, 0.0f};
  Rigid hand = rigid_compose(l8, RH, Z3);
  visit(std::integral_constant<int, 9>{}, hand);
  const float TL[3] = {0.0f, finger, 0.0584f};
  const float TR[3] = {0.0f, -finger, 0.0584f};
  Rigid lf = rigid_compose(hand, I3, TL);
  Rigid rf = rigid_compose(hand, I3, TR);
  visit(std::integral_constant<int, 10>{}, lf);
  visit(std::integral_constant<int, 11>{}, rf);
  const float TT[3] = {0.0f, 0.0f, 0.045f};
  visit(std::integral_constant<int, 12>{}, rigid_compose(lf, I3, TT));
  visit(std::integral_constant<int, 13>{}, rigid_compose(rf, I3, TT));
  const float RG[9] = {-SH, -SH, 0, SH, -SH, 0, 0, 0, 1};
  const float TG[3] = {0.0f, 0.0f, 0.1f};
  visit(std::integral_constant<int, 14>{}, rigid_compose(l8, RG, TG));
}

// Writes the 15 frames x 12 floats to `out` (any address space the caller indexes with a plain pointer: LDS or global).
__device__ __forceinline__ void franka_fk_frames(const float *q7, float finger, float *out) {
  franka_fk_visit(q7, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
    constexpr int id = decltype(ID)::value;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[12 * id + k] = g.r[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[12 * id + 9 + k] = g.t[k];
  });
}

// ---- the self-collision model ---------------------------------------------------------------------------------------------
// The in-repo Geometric-Fabrics model (config/franka_fabric_config.yaml:120-140; franka_tables.FABRIC_BODY_CYLINDER /
// FABRIC_SELF_SPHERES): spheres at the origins of link7, the hand and the fingertips against the body cylinder around the
// base segment.  tests/test_franka_tables.py reads these constants; the comparison's literal appears nowhere else.
constexpr float FRANKA_SELF_SEGMENT_Z0 = -0.3f;   // the base segment (0, 0, Z0) - (0, 0, Z1)
constexpr float FRANKA_SELF_SEGMENT_Z1 = 0.333f;
constexpr float FRANKA_SELF_BODY_RADIUS = 0.15f;
constexpr int FRANKA_SELF_SPHERES = 4;
constexpr int FRANKA_SELF_FRAME[FRANKA_SELF_SPHERES] = {7, 9, 12, 13};
constexpr float FRANKA_SELF_RADIUS[FRANKA_SELF_SPHERES] = {0.1f, 0.01f, 0.01f, 0.01f};

// frame id -> its sphere of the self model, -1: none
constexpr int franka_self_sphere(int frame) {
  for (int s = 0; s < FRANKA_SELF_SPHERES; ++s)
    if (FRANKA_SELF_FRAME[s] == frame) return s;
  return -1;
}

// distance of a frame origin to the base segment
__device__ __forceinline__ float franka_self_distance(float x, float y, float z) {
  const float zc = fminf(fmaxf(z, FRANKA_SELF_SEGMENT_Z0), FRANKA_SELF_SEGMENT_Z1);
  const float dz = z - zc;
  return sqrtf(mpx_fma(dz, dz, mpx_fma(y, y, x * x)));
}
// the verdict for a sphere of `radius` at that origin; with a margin, (body + radius) + margin
__device__ __forceinline__ bool franka_self_hit(float x, float y, float z, float radius) {
  return franka_self_distance(x, y, z) < FRANKA_SELF_BODY_RADIUS + radius;
}
__device__ __forceinline__ bool franka_self_hit(float x, float y, float z, float radius, float margin) {
  return franka_self_distance(x, y, z) < FRANKA_SELF_BODY_RADIUS + radius + margin;
}
// on frame `id` of franka_fk_visit (one of FRANKA_SELF_FRAME)
template <int id>
__device__ __forceinline__ bool franka_self_hit(const Rigid &g, float margin) {
  constexpr int s = franka_self_sphere(id);
  static_assert(s >= 0, "the self model's frames");
  constexpr float radius = FRANKA_SELF_RADIUS[s];
  return franka_self_hit(g.t[0], g.t[1], g.t[2], radius, margin);
}
