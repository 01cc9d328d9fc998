// gripper_device.h -- the free-flying gripper as the two gripper roadmap kernels take it (gripper_roadmap.hip against
// primitives, gripper_roadmap_cloud.hip against a distance field), the two shortcut kernels behind them (gripper_shortcut.hip,
// gripper_shortcut_cloud.hip) and, for its validity against primitives, task_candidates.hip: a node (position, unit quaternion x y z w) from a pose
// and back, the SE(3) metric, the nlerp edge pose and the self half of a pose's validity.  One text for both; what differs
// between them (the LDS layout, the environment half of the validity, the host entry) stays in each .hip, and the statement
// blocks they share are gripper_spheres.inc, gripper_nodes.inc, gripper_tail.inc and gripper_poses.inc.  The contract is stated in
// include/mpinets_hip.h (mpx_gripper_roadmap).
#pragma once
#include "common.h"
#include "plan_device.h"
#include "plan_prims_device.h"

enum { STREAM_GRIPPER_ROADMAP = 17 };
enum { GRM_MAX_SPHERES = 64 };

// rows 0..2 of a row-major 4x4 pose -> position, unit quaternion (x, y, z, w) by Shepperd's method: the branch is the
// largest of (trace, r00, r11, r22), the first of equal ones in that order; the result is divided by its norm
__device__ __forceinline__ void gripper_pose_node(const float *m, float *node) {
  const float r00 = m[0], r01 = m[1], r02 = m[2], r10 = m[4], r11 = m[5], r12 = m[6], r20 = m[8], r21 = m[9], r22 = m[10];
  const float tr = r00 + r11 + r22;
  float x, y, z, w;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    const float s = 2.0f * sqrtf(1.0f + tr);
    w = 0.25f * s, x = (r21 - r12) / s, y = (r02 - r20) / s, z = (r10 - r01) / s;
  } else if (r00 >= r11 && r00 >= r22) {
    const float s = 2.0f * sqrtf(1.0f + r00 - r11 - r22);
    x = 0.25f * s, w = (r21 - r12) / s, y = (r01 + r10) / s, z = (r02 + r20) / s;
  } else if (r11 >= r22) {
    const float s = 2.0f * sqrtf(1.0f + r11 - r00 - r22);
    y = 0.25f * s, w = (r02 - r20) / s, x = (r01 + r10) / s, z = (r12 + r21) / s;
  } else {
    const float s = 2.0f * sqrtf(1.0f + r22 - r00 - r11);
    z = 0.25f * s, w = (r10 - r01) / s, x = (r02 + r20) / s, y = (r12 + r21) / s;
  }
  const float n = sqrtf(mpx_fma(w, w, mpx_fma(z, z, mpx_fma(y, y, x * x))));
  node[0] = m[3], node[1] = m[7], node[2] = m[11];
  node[3] = x / n, node[4] = y / n, node[5] = z / n, node[6] = w / n;
}

// unit quaternion (x, y, z, w) and position -> the frame
__device__ __forceinline__ Rigid gripper_frame(const float *node) {
  const float x = node[3], y = node[4], z = node[5], w = node[6];
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  Rigid g;
  g.r[0] = 1.0f - 2.0f * (yy + zz), g.r[1] = 2.0f * (xy - wz), g.r[2] = 2.0f * (xz + wy);
  g.r[3] = 2.0f * (xy + wz), g.r[4] = 1.0f - 2.0f * (xx + zz), g.r[5] = 2.0f * (yz - wx);
  g.r[6] = 2.0f * (xz - wy), g.r[7] = 2.0f * (yz + wx), g.r[8] = 1.0f - 2.0f * (xx + yy);
  g.t[0] = node[0], g.t[1] = node[1], g.t[2] = node[2];
  return g;
}

// rows 0-2 of the row-major 4x4 pose [R | p] of a frame (12 floats)
__device__ __forceinline__ void gripper_frame_rows(const Rigid &g, float *o) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[4 * r + 0] = g.r[3 * r + 0], o[4 * r + 1] = g.r[3 * r + 1], o[4 * r + 2] = g.r[3 * r + 2], o[4 * r + 3] = g.t[r];
}

__device__ __forceinline__ float gripper_dot4(const float *a, const float *b) {
  return mpx_fma(a[3], b[3], mpx_fma(a[2], b[2], mpx_fma(a[1], b[1], a[0] * b[0])));
}

// a caller's vertex (mpx_gripper_shortcut): its quaternion's squared norm is not within 2^-10 of 1 (NaN: bad)
__device__ __forceinline__ bool gripper_vertex_bad(const float *node) {
  return !(fabsf(gripper_dot4(node + 3, node + 3) - 1.0f) <= 0x1p-10f);
}

// w_ab: k ascending, the first square rounded on its own, the others fused; positions first, then (2 rot_weight)^2 times
// the squared quaternion chord.  Every term is the same bits for (b,a): products commute, (x - y)^2 = (y - x)^2, and with
// sigma = -1 the chord is a sum.
__device__ __forceinline__ float gripper_length(const float *na, const float *nb, float rot_k) {
  float acc = 0.0f, rq = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = nb[k] - na[k];
    acc = k == 0 ? d * d : mpx_fma(d, d, acc);
  }
  const bool same = gripper_dot4(na + 3, nb + 3) >= 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d = same ? nb[3 + k] - na[3 + k] : nb[3 + k] + na[3 + k];
    rq = k == 0 ? d * d : mpx_fma(d, d, rq);
  }
  return sqrtf(mpx_fma(rot_k, rq, acc));
}

// the pose at fraction f of the edge from na to nb: positions by fma, orientations by nlerp toward sigma q_b
__device__ __forceinline__ void gripper_edge_pose(const float *na, const float *nb, float f, float *out) {
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = mpx_fma(f, nb[k] - na[k], na[k]);
  const bool same = gripper_dot4(na + 3, nb + 3) >= 0.0f;
  float raw[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) raw[k] = mpx_fma(f, (same ? nb[3 + k] : -nb[3 + k]) - na[3 + k], na[3 + k]);
  const float n = sqrtf(mpx_fma(raw[3], raw[3], mpx_fma(raw[2], raw[2], mpx_fma(raw[1], raw[1], raw[0] * raw[0]))));
#pragma unroll
  for (int k = 0; k < 4; ++k) out[3 + k] = raw[k] / n;
}

// the self half of a pose's validity: the origin of the hand or of a fingertip frame inside the body column (the origins
// of frames 9, 12, 13 in the right_gripper frame: the offsets of the sphere rows of gripper_spheres.inc)
__device__ __forceinline__ bool gripper_self_hit(const Rigid &g, float finger, float self_margin) {
  const float tip = (0.0584f + 0.045f) - 0.1f;
  bool hit = false;
  Rigid o = g;
  rigid_apply(g, 0.0f, 0.0f, -0.1f, o.t[0], o.t[1], o.t[2]);
  hit |= franka_self_hit<9>(o, self_margin);
  rigid_apply(g, 0.0f, -finger, tip, o.t[0], o.t[1], o.t[2]);
  hit |= franka_self_hit<12>(o, self_margin);
  rigid_apply(g, 0.0f, finger, tip, o.t[0], o.t[1], o.t[2]);
  hit |= franka_self_hit<13>(o, self_margin);
  return hit;
}

// the planner's validity clause on the gripper alone, against a problem's live primitives (the LDS rows of
// franka_live_rows.inc, the gripper's sphere rows of gripper_spheres.inc): a sphere with sdf <= r_s + reach, or (test_self)
// the origin of the hand or a fingertip frame inside the body column.  gripper_roadmap.hip judges its nodes and edge poses
// by it, task_candidates.hip its drawn poses (which are frames already: gripper_frame_hit).
__device__ __forceinline__ bool gripper_frame_hit(const Rigid &g, float finger, const float *gsph, int n_g,
                                                  const float *prim_rows, int n_cub, int n_cyl, float reach, bool test_self,
                                                  float self_margin) {
  bool hit = false;
  if (n_cub + n_cyl > 0) {
    for (int s = 0; s < n_g; ++s) {
      float x, y, z;
      rigid_apply(g, gsph[4 * s + 0], gsph[4 * s + 1], gsph[4 * s + 2], x, y, z);
      int arg;
      const float best = plan_min_sdf(prim_rows, n_cub, n_cyl, x, y, z, arg);
      hit |= best <= gsph[4 * s + 3] + reach;
    }
  }
  if (test_self) hit |= gripper_self_hit(g, finger, self_margin);
  return hit;
}
__device__ __forceinline__ bool gripper_pose_hit(const float *node, float finger, const float *gsph, int n_g,
                                                 const float *prim_rows, int n_cub, int n_cyl, float reach, bool test_self,
                                                 float self_margin) {
  return gripper_frame_hit(gripper_frame(node), finger, gsph, n_g, prim_rows, n_cub, n_cyl, reach, test_self, self_margin);
}
