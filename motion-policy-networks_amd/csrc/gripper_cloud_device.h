// gripper_cloud_device.h -- the validity of a pose of the free-flying gripper against a point cloud's distance field, as
// gripper_roadmap_cloud.hip judges its nodes and edge poses and gripper_shortcut_cloud.hip its chord poses.  One text for both;
// the clause is stated in include/mpinets_hip.h (mpx_gripper_roadmap_cloud).
#pragma once
#include "field_device.h"
#include "gripper_device.h"

// roadmap_cloud_bits' rule on the gripper alone: a sphere whose centre is inside the grid, where the field is not saturated
// and d = ((D - point_radius) - r_s) - clearance <= slack_margin (= check_margin + field_slack, summed once on the host), or
// (test_self) the origin of the hand or a fingertip frame inside the body column.  `f` is ONE environment's nodes, nullptr:
// no environment test.  (A NaN centre is outside the grid: it reads no memory.)
__device__ __forceinline__ bool gripper_cloud_pose_hit(const float *node, float finger, const float *gsph, int n_g,
                                                       const float *__restrict__ f, const FieldGrid &G, float point_radius,
                                                       float clearance, float slack_margin, bool test_self,
                                                       float self_margin) {
  const Rigid g = gripper_frame(node);
  bool hit = false;
  if (f) {
    for (int s = 0; s < n_g; ++s) {
      float x, y, z, D, gx, gy, gz;
      rigid_apply(g, gsph[4 * s + 0], gsph[4 * s + 1], gsph[4 * s + 2], x, y, z);
      const bool inside = field_sample<false>(f, G, x, y, z, D, gx, gy, gz);
      const float d = ((D - point_radius) - gsph[4 * s + 3]) - clearance;
      hit |= inside && D < G.trunc && d <= slack_margin;
    }
  }
  if (test_self) hit |= gripper_self_hit(g, finger, self_margin);
  return hit;
}
