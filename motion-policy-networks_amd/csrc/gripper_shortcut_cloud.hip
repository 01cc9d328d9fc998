// gripper_shortcut_cloud.hip -- gripper_shortcut.hip's shortcutting of the gripper's SE(3) polyline against a POINT CLOUD:
// behind gripper_roadmap_cloud.hip, in front of the cloud follower.  What makes a pose invalid is read off the truncated
// distance field by gripper_roadmap_cloud.hip's rule (gripper_cloud_device.h: 8 cached global loads and 7 lerps per gripper
// sphere); the field APPROXIMATES the distance, so a guide pose may graze the cloud and the follower's trajectory is still
// judged by the exact swept-sphere test.  The passes, the densification, the greedy walk, the outputs and the guide poses are
// mpx_gripper_shortcut's, by the same text (shortcut_kernel.inc, gripper_device.h, gripper_spheres.inc, gripper_poses.inc);
// the contract is stated in include/mpinets_hip.h.
//
// gripper_shortcut_kernel's structure: one workgroup of 256 threads per problem, everything but the field in LDS, no scratch
// memory and no global atomics; thread = vertex, thread = interior pose of a probe level's chords, thread = output pose.
// Every branch around a barrier is workgroup-uniform: it reads a value from LDS behind a barrier, a kernel argument, or a
// barrier's own reduction.
#include "common.h"
#include "franka_host.h"
#include "plan_device.h"
#include "field_device.h"
#include "roadmap_device.h"
#include "gripper_device.h"
#include "gripper_cloud_device.h"

// LDS, in 4-byte words: gripper_shortcut.hip's layout without the primitive rows: [gripper spheres 64 x 4 | sphere count |
// shortcut_lds_words(P, 0)]
__host__ __device__ static inline size_t gripper_shortcut_cloud_lds_words(int P) {
  return (size_t)GRM_MAX_SPHERES * 4 + 1 + shortcut_lds_words(P, 0);
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    gripper_shortcut_cloud_kernel(const float *__restrict__ points, const int32_t *__restrict__ count, int Pin, int W,
                                  const float *__restrict__ goal_pose, float finger, const float *__restrict__ sc,
                                  const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                  const float *__restrict__ field, FieldGrid G, float point_radius, float slack_margin,
                                  mpx_gripper_shortcut_options opt, float *__restrict__ poses, int32_t *__restrict__ status,
                                  float *__restrict__ points_out, int32_t *__restrict__ count_out,
                                  float *__restrict__ length, int32_t *__restrict__ chords_out,
                                  int32_t *__restrict__ configs_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *gsph = lds;
  int *ng_lds = reinterpret_cast<int *>(gsph + GRM_MAX_SPHERES * 4);
  SHORTCUT_LDS_CARVE_T(gsph + GRM_MAX_SPHERES * 4 + 1, opt.points, 0)
  (void)tbuf;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
#include "gripper_spheres.inc"
  const bool test_self = opt.check_self != 0;
  const float two_rw = 2.0f * opt.rot_weight, rot_k = two_rw * two_rw;
  const float *fenv = field != nullptr ? field + (size_t)b * ((size_t)G.nx * G.ny * G.nz) : nullptr;
  // (the body's first barrier publishes the gripper spheres and their count)
#define SHORTCUT_VERTEX_BAD(v) gripper_vertex_bad(v)
#define SHORTCUT_LENGTH(a, e) gripper_length(a, e, rot_k)
#define SHORTCUT_POINT(a, e, f, q) gripper_edge_pose(a, e, f, q);
#define SHORTCUT_HIT(q)                                                                                                 \
  gripper_cloud_pose_hit(q, finger, gsph, *ng_lds, fenv, G, point_radius, opt.clearance, slack_margin, test_self, \
                         opt.check_margin)
#include "shortcut_kernel.inc"
#undef SHORTCUT_VERTEX_BAD
#undef SHORTCUT_LENGTH
#undef SHORTCUT_POINT
#undef SHORTCUT_HIT

  // ---- the guide poses over the returned polyline (vertex i is nodes[path[i]], path[i] = i) ----------------------------------------
  const int V = P, hops = n - 1;
  const float *nodes = cur;
#define GRIPPER_POSES_GOAL(o)                                                    \
  if (goal_pose) {                                                               \
    _Pragma("unroll") for (int i = 0; i < 12; ++i) o[i] = goal_pose[(size_t)b * 16 + i]; \
  } else {                                                                       \
    gripper_frame_rows(gripper_frame(nodes + path[hops] * 7), o);                \
  }
#include "gripper_poses.inc"
#undef GRIPPER_POSES_GOAL
}

MPX_EXPORT int mpx_gripper_shortcut_cloud(const float *points, const int32_t *count, int B, int Pin, int W,
                                          const float *goal_pose, float finger, const float *sph_centers,
                                          const float *sph_radii, const int32_t *sph_link, int S, const float *field,
                                          const mpx_field_grid *grid, float point_radius, float field_slack,
                                          const mpx_gripper_shortcut_options *options, float *poses, int32_t *status,
                                          float *points_out, int32_t *count_out, float *length, int32_t *chords,
                                          int32_t *configs, mpx_stream_t stream) {
  const char *who = "mpx_gripper_shortcut_cloud";
  const mpx_gripper_shortcut_options opt = options ? *options : gripper_shortcut_defaults();
  const float big = __builtin_huge_valf();
  MPX_REQUIRE(B >= 0 && S >= 0, "%s: negative size", who);
  if (gripper_shortcut_options_check(who, W, Pin, opt) || franka_counts_check(who, S) ||
      franka_rows_check(who, B, W * 16, "B x W x 16 pose entries") ||
      franka_rows_check(who, B, opt.points * 7, "B x P x 7 polyline entries"))
    return 1;
  MPX_REQUIRE(point_radius >= 0.0f && point_radius < big, "%s: point_radius must be finite and >= 0", who);
  MPX_REQUIRE(field_slack >= 0.0f && field_slack < big, "%s: field_slack must be finite and >= 0", who);
  FieldGrid G = {};
  const float slack_margin = opt.check_margin + field_slack;  // (float32, summed once: the kernel's right-hand side)
  if (field) {  // (mpx_gripper_roadmap_cloud's refusals, in its words)
    if (field_grid_check(who, grid, G)) return 1;
    MPX_REQUIRE(S > 0, "%s: a field without collision spheres to test it with", who);
    const float need = MPX_FRANKA_MAX_SPHERE_RADIUS + point_radius + (opt.clearance > 0.0f ? opt.clearance : 0.0f) + slack_margin;
    MPX_REQUIRE(G.trunc > need,
                "%s: grid trunc = %g, need more than %g = largest sphere radius %g + point_radius + max(clearance, 0) + "
                "check_margin + field_slack (an obstacle in between would be missed)",
                who, (double)G.trunc, (double)need, (double)MPX_FRANKA_MAX_SPHERE_RADIUS);
  }
  if (B == 0) return 0;
  MPX_REQUIRE(poses && status && points_out && count_out && length,
              "%s: NULL output (poses, status, points_out, count_out, length)", who);
  MPX_REQUIRE(points && count, "%s: NULL operand (points, count)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  const size_t lds = 4 * gripper_shortcut_cloud_lds_words(opt.points);  // 24 604 B at 256 points
  hipLaunchKernelGGL(gripper_shortcut_cloud_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), points, count,
                     Pin, W, goal_pose, finger, sph_centers, sph_radii, sph_link, S, field, G, point_radius, slack_margin, opt,
                     poses, status, points_out, count_out, length, chords, configs);
  MPX_LAUNCH_CHECK(who);
}
