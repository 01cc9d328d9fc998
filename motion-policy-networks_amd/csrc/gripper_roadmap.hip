// gripper_roadmap.hip -- a lazy probabilistic roadmap per problem for the FREE-FLYING GRIPPER in SE(3): where the reference's
// data generator plans the end effector through the scene with OMPL before it hands the pose path to the fabric
// (data_pipeline/gen_data.py:156-189, plan_end_effector).  A STAND-IN for that planner, NOT a port of it and without any claim
// of parity with AIT*; "valid" means free by this engine's sphere model (the hand and fingertip spheres of the table), not by
// PyBullet's meshes.  V poses (start, goal, V - 2 Philox draws: positions in the problem's box, orientations scattered
// about the start-goal arc) are judged by the planner's own clause (plan_min_sdf on the live rows, franka_self_hit); the
// search is mpx_franka_roadmap's, statement for statement, over the SE(3) metric below; the surviving polyline is resampled
// to W guide poses for mpx_franka_follow.  The contract is stated in include/mpinets_hip.h.
//
// One workgroup of 256 threads per problem, everything in LDS, no scratch memory and no global atomics.  The mappings are
// roadmap.hip's: thread = node (draw, validity, one Jacobi sweep: V <= 256), thread = interior pose across the concatenated
// untested edges of the round's path (passes of 256), thread = output pose (W <= 64).  Every branch around a barrier is
// workgroup-uniform: it reads a value from LDS behind a barrier, or a barrier's own reduction.  The search is the statement
// block both kernels include (roadmap_search.inc), with the gripper's metric and edge pose (gripper_device.h) and this
// file's validity (gripper_pose_hit, which gripper_device.h states for this kernel and task_candidates.hip).  The sphere set, the node draw and the tail are the statement blocks gripper_roadmap_cloud.hip runs too
// (gripper_spheres.inc, gripper_nodes.inc, gripper_tail.inc).
#include "common.h"
#include "franka_host.h"
#include "plan_prims_device.h"
#include "roadmap_device.h"
#include "gripper_device.h"

// LDS, in 4-byte words: [128 primitive rows x 16 | gripper spheres 64 x 4 (point in the right_gripper frame, radius) |
// nodes V x 7 | dist 2 x V (later: cumulative and edge lengths) | pred, path, rev, pieces, blocked, valid: V ints each |
// first V + 1 | hops | sphere count | edge bits]
__host__ __device__ static inline size_t gripper_roadmap_lds_words(int V) {
  return (size_t)128 * 16 + (size_t)GRM_MAX_SPHERES * 4 + (size_t)V * 7 + 2 * (size_t)V + 6 * (size_t)V + (size_t)V + 1 + 1 +
         1 + ((size_t)V * V + 15) / 16;
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    gripper_roadmap_kernel(const float *__restrict__ start_pose, const float *__restrict__ goal_pose, int W,
                           const float *__restrict__ bounds, float finger, const float *__restrict__ sc,
                           const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                           const float *__restrict__ cub_f, const float *__restrict__ cub_d, int M1,
                           const float *__restrict__ cyl_f, const float *__restrict__ cyl_r,
                           const float *__restrict__ cyl_h, int M2, mpx_gripper_roadmap_options opt, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t env0, float *__restrict__ poses, int32_t *__restrict__ status,
                           int32_t *__restrict__ path_out, int32_t *__restrict__ hops_out, float *__restrict__ nodes_out,
                           uint8_t *__restrict__ edge_out, int32_t *__restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int V = opt.nodes;
  float *prim_rows = lds;
  float *gsph = prim_rows + 128 * 16;
  float *nodes = gsph + GRM_MAX_SPHERES * 4;
  float *dist = nodes + V * 7;
  int *pred = reinterpret_cast<int *>(dist + 2 * V);
  int *path = pred + V, *rev = path + V, *pieces = rev + V, *blocked = pieces + V, *valid = blocked + V;
  int *first = valid + V;  // first[i]: index of edge i's first interior pose among the round's tests
  int *hops_lds = first + V + 1;
  int *ng_lds = hops_lds + 1;
  unsigned *ebits = reinterpret_cast<unsigned *>(ng_lds + 1);
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const float *sp = start_pose + (size_t)b * 16, *gp = goal_pose + (size_t)b * 16;

#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  for (int i = tid; i < (V * V + 15) / 16; i += ROADMAP_THREADS) ebits[i] = 0u;

#include "gripper_spheres.inc"

  // ---- nodes: thread = node ------------------------------------------------------------------------------------------------------
#include "gripper_nodes.inc"
  __syncthreads();  // (the primitive rows, the gripper spheres, the nodes, the cleared edge bits)

  const int n_g = *ng_lds;
  const bool test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;
  const float two_rw = 2.0f * opt.rot_weight, rot_k = two_rw * two_rw;
  if (tid < V)
    valid[tid] = inside && !gripper_pose_hit(mine, finger, gsph, n_g, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin);
  __syncthreads();

  // ---- the lazy search: roadmap.hip's, over the SE(3) metric and the gripper's validity ----------------------------------------------
#define ROADMAP_SEARCH_LENGTH(a, b) gripper_length(a, b, rot_k)
#define ROADMAP_SEARCH_POINT(a, e, f, q) gripper_edge_pose(nodes + a * 7, nodes + e * 7, f, q);
#define ROADMAP_SEARCH_HIT(q) \
  gripper_pose_hit(q, finger, gsph, n_g, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin)
#include "roadmap_search.inc"
#undef ROADMAP_SEARCH_LENGTH
#undef ROADMAP_SEARCH_POINT
#undef ROADMAP_SEARCH_HIT

#include "gripper_tail.inc"
}

MPX_EXPORT int mpx_gripper_roadmap(const float *start_pose, const float *goal_pose, int B, int W, const float *bounds,
                                   float finger, const float *sph_centers, const float *sph_radii, const int32_t *sph_link,
                                   int S, const float *cub_inv_frames, const float *cub_dims, int M1,
                                   const float *cyl_inv_frames, const float *cyl_radii, const float *cyl_heights, int M2,
                                   const mpx_gripper_roadmap_options *options, uint64_t seed, int64_t env_offset, float *poses,
                                   int32_t *status, int32_t *path, int32_t *hops, float *nodes, uint8_t *edge_state,
                                   int32_t *rounds, mpx_stream_t stream) {
  const char *who = "mpx_gripper_roadmap";
  const mpx_gripper_roadmap_options opt = options ? *options : gripper_roadmap_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (gripper_roadmap_options_check(who, W, opt) || franka_counts_check(who, S, M1, M2) ||
      franka_env_offset_check(who, env_offset, B) || franka_rows_check(who, B, W * 16, "B x W x 16 pose entries"))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(poses && status && path && hops, "%s: NULL output (poses, status, path, hops)", who);
  MPX_REQUIRE(start_pose && goal_pose && bounds, "%s: NULL operand (start_pose, goal_pose, bounds)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const size_t lds = 4 * gripper_roadmap_lds_words(opt.nodes);  // 41 996 B at 256 nodes
  hipLaunchKernelGGL(gripper_roadmap_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), start_pose, goal_pose,
                     W, bounds, finger, sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames,
                     cyl_radii, cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, poses,
                     status, path, hops, nodes, edge_state, rounds);
  MPX_LAUNCH_CHECK(who);
}
