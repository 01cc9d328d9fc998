// gripper_shortcut.hip -- shortcutting of an SE(3) polyline of the free-flying gripper per problem, between gripper_roadmap.hip
// and the follower: the dog-leg path through a few random nodes is shortened before it is resampled to guide poses.  Part of
// the same STAND-IN for the reference's end-effector planner (data_pipeline/gen_data.py:156-189), NOT a port of it.  The
// algorithm is the joint-space shortcut's by the same text (shortcut_kernel.inc: densify, the greedy furthest-free-chord walk
// with a K-ary search, alternating directions) with the gripper's metric, edge pose and validity as its hooks
// (gripper_device.h); the guide poses are the roadmap's by the same text (gripper_poses.inc).  The contract is stated in
// include/mpinets_hip.h (mpx_gripper_shortcut).
//
// One workgroup of 256 threads per problem, everything in LDS, no scratch memory and no global atomics.  The mappings are
// shortcut_kernel.inc's: thread = vertex (load, reverse, densify, copy), thread = interior pose across the concatenated
// chords of one probe level, thread = output pose (W <= 64).  Every branch around a barrier is workgroup-uniform: it reads a
// value from LDS behind a barrier, a kernel argument, or a barrier's own reduction.
#include "common.h"
#include "franka_host.h"
#include "plan_prims_device.h"
#include "roadmap_device.h"
#include "gripper_device.h"

// LDS, in 4-byte words: [128 primitive rows x 16 | gripper spheres 64 x 4 (point in the right_gripper frame, radius) |
// sphere count | shortcut_lds_words(P, 0): no trajectory buffer, dist holds the tail's cumulative and edge lengths]
__host__ __device__ static inline size_t gripper_shortcut_lds_words(int P) {
  return (size_t)128 * 16 + (size_t)GRM_MAX_SPHERES * 4 + 1 + shortcut_lds_words(P, 0);
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    gripper_shortcut_kernel(const float *__restrict__ points, const int32_t *__restrict__ count, int Pin, int W,
                            const float *__restrict__ goal_pose, float finger, const float *__restrict__ sc,
                            const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                            const float *__restrict__ cub_f, const float *__restrict__ cub_d, int M1,
                            const float *__restrict__ cyl_f, const float *__restrict__ cyl_r,
                            const float *__restrict__ cyl_h, int M2, mpx_gripper_shortcut_options opt,
                            float *__restrict__ poses, int32_t *__restrict__ status, float *__restrict__ points_out,
                            int32_t *__restrict__ count_out, float *__restrict__ length, int32_t *__restrict__ chords_out,
                            int32_t *__restrict__ configs_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *prim_rows = lds;
  float *gsph = prim_rows + 128 * 16;
  int *ng_lds = reinterpret_cast<int *>(gsph + GRM_MAX_SPHERES * 4);
  SHORTCUT_LDS_CARVE_T(gsph + GRM_MAX_SPHERES * 4 + 1, opt.points, 0)
  (void)tbuf;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
#include "gripper_spheres.inc"
  const bool test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;
  const float two_rw = 2.0f * opt.rot_weight, rot_k = two_rw * two_rw;
  // (the body's first barrier publishes the primitive rows, the gripper spheres and their count)
#define SHORTCUT_VERTEX_BAD(v) gripper_vertex_bad(v)
#define SHORTCUT_LENGTH(a, e) gripper_length(a, e, rot_k)
#define SHORTCUT_POINT(a, e, f, q) gripper_edge_pose(a, e, f, q);
#define SHORTCUT_HIT(q) \
  gripper_pose_hit(q, finger, gsph, *ng_lds, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin)
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

MPX_EXPORT int mpx_gripper_shortcut(const float *points, const int32_t *count, int B, int Pin, int W, const float *goal_pose,
                                    float finger, const float *sph_centers, const float *sph_radii, const int32_t *sph_link,
                                    int S, const float *cub_inv_frames, const float *cub_dims, int M1,
                                    const float *cyl_inv_frames, const float *cyl_radii, const float *cyl_heights, int M2,
                                    const mpx_gripper_shortcut_options *options, float *poses, int32_t *status,
                                    float *points_out, int32_t *count_out, float *length, int32_t *chords, int32_t *configs,
                                    mpx_stream_t stream) {
  const char *who = "mpx_gripper_shortcut";
  const mpx_gripper_shortcut_options opt = options ? *options : gripper_shortcut_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (gripper_shortcut_options_check(who, W, Pin, opt) || franka_counts_check(who, S, M1, M2) ||
      franka_rows_check(who, B, W * 16, "B x W x 16 pose entries") ||
      franka_rows_check(who, B, opt.points * 7, "B x P x 7 polyline entries"))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(poses && status && points_out && count_out && length,
              "%s: NULL output (poses, status, points_out, count_out, length)", who);
  MPX_REQUIRE(points && count, "%s: NULL operand (points, count)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const size_t lds = 4 * gripper_shortcut_lds_words(opt.points);  // 32 796 B at 256 points
  hipLaunchKernelGGL(gripper_shortcut_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), points, count, Pin,
                     W, goal_pose, finger, sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames,
                     cyl_radii, cyl_heights, M2, opt, poses, status, points_out, count_out, length, chords, configs);
  MPX_LAUNCH_CHECK(who);
}
