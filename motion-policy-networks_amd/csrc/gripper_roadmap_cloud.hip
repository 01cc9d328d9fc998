// gripper_roadmap_cloud.hip -- gripper_roadmap.hip's lazy SE(3) roadmap for the free-flying gripper against a POINT CLOUD:
// the guide of mpx_franka_follow_cloud where a captured cloud has no primitives.  Still the STAND-IN for the reference's OMPL
// end-effector planner (data_pipeline/gen_data.py:156-189, plan_end_effector), NOT a port of it.  What makes a pose invalid
// is read off the truncated distance field that already steers the cloud planner and the cloud follower (field_device.h: 8
// cached global loads and 7 lerps per gripper sphere) by roadmap_cloud.hip's rule; the self test is the parent's.  The field
// APPROXIMATES the distance (within (sqrt(3)/2) h of it), so a guide pose may graze the cloud: what the follower returns is
// still judged by the exact swept-sphere test.  The sphere set, the nodes, the metric, the edges, the search, the statuses
// and the guide poses are mpx_gripper_roadmap's, by the same text (gripper_device.h, gripper_spheres.inc, gripper_nodes.inc,
// roadmap_search.inc, gripper_tail.inc); the contract is stated in include/mpinets_hip.h.
//
// gripper_roadmap_kernel's structure: one workgroup of 256 threads per problem, everything but the field in LDS, no scratch
// memory and no global atomics; thread = node, thread = interior pose of the round's untested edges, thread = output pose.
// Every branch around a barrier is workgroup-uniform: it reads a value from LDS behind a barrier, or a barrier's own
// reduction.
#include "common.h"
#include "franka_host.h"
#include "plan_device.h"
#include "field_device.h"
#include "roadmap_device.h"
#include "gripper_device.h"
#include "gripper_cloud_device.h"

// LDS, in 4-byte words: gripper_roadmap.hip's layout without the primitive rows: [gripper spheres 64 x 4 (point in the
// right_gripper frame, radius) | nodes V x 7 | dist 2 x V (later: cumulative and edge lengths) | pred, path, rev, pieces,
// blocked, valid: V ints each | first V + 1 | hops | sphere count | edge bits]
__host__ __device__ static inline size_t gripper_roadmap_cloud_lds_words(int V) {
  return (size_t)GRM_MAX_SPHERES * 4 + (size_t)V * 7 + 2 * (size_t)V + 6 * (size_t)V + (size_t)V + 1 + 1 + 1 +
         ((size_t)V * V + 15) / 16;
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    gripper_roadmap_cloud_kernel(const float *__restrict__ start_pose, const float *__restrict__ goal_pose, int W,
                                 const float *__restrict__ bounds, float finger, const float *__restrict__ sc,
                                 const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                 const float *__restrict__ field, FieldGrid G, float point_radius, float slack_margin,
                                 mpx_gripper_roadmap_options opt, uint32_t seed_lo, uint32_t seed_hi, uint32_t env0,
                                 float *__restrict__ poses, int32_t *__restrict__ status, int32_t *__restrict__ path_out,
                                 int32_t *__restrict__ hops_out, float *__restrict__ nodes_out,
                                 uint8_t *__restrict__ edge_out, int32_t *__restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int V = opt.nodes;
  float *gsph = lds;
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

  for (int i = tid; i < (V * V + 15) / 16; i += ROADMAP_THREADS) ebits[i] = 0u;

#include "gripper_spheres.inc"

  // ---- nodes: thread = node (mpx_gripper_roadmap's draw: the same seed gives the same nodes) ---------------------------------------
#include "gripper_nodes.inc"
  __syncthreads();  // (the gripper spheres, the nodes, the cleared edge bits)

  const int n_g = *ng_lds;
  const bool test_self = opt.check_self != 0;
  const float two_rw = 2.0f * opt.rot_weight, rot_k = two_rw * two_rw;
  const float *fenv = field != nullptr ? field + (size_t)b * ((size_t)G.nx * G.ny * G.nz) : nullptr;
  if (tid < V)
    valid[tid] = inside && !gripper_cloud_pose_hit(mine, finger, gsph, n_g, fenv, G, point_radius, opt.clearance, slack_margin,
                                                   test_self, opt.check_margin);
  __syncthreads();

  // ---- the lazy search: roadmap.hip's, over the SE(3) metric, with the field as the environment test -----------------------------------
#define ROADMAP_SEARCH_LENGTH(a, b) gripper_length(a, b, rot_k)
#define ROADMAP_SEARCH_POINT(a, e, f, q) gripper_edge_pose(nodes + a * 7, nodes + e * 7, f, q);
#define ROADMAP_SEARCH_HIT(q) \
  gripper_cloud_pose_hit(q, finger, gsph, n_g, fenv, G, point_radius, opt.clearance, slack_margin, test_self, opt.check_margin)
#include "roadmap_search.inc"
#undef ROADMAP_SEARCH_LENGTH
#undef ROADMAP_SEARCH_POINT
#undef ROADMAP_SEARCH_HIT

#include "gripper_tail.inc"
}

MPX_EXPORT int mpx_gripper_roadmap_cloud(const float *start_pose, const float *goal_pose, int B, int W, const float *bounds,
                                         float finger, const float *sph_centers, const float *sph_radii,
                                         const int32_t *sph_link, int S, const float *field, const mpx_field_grid *grid,
                                         float point_radius, float field_slack, const mpx_gripper_roadmap_options *options,
                                         uint64_t seed, int64_t env_offset, float *poses, int32_t *status, int32_t *path,
                                         int32_t *hops, float *nodes, uint8_t *edge_state, int32_t *rounds,
                                         mpx_stream_t stream) {
  const char *who = "mpx_gripper_roadmap_cloud";
  const mpx_gripper_roadmap_options opt = options ? *options : gripper_roadmap_defaults();
  const float big = __builtin_huge_valf();
  MPX_REQUIRE(B >= 0 && S >= 0, "%s: negative size", who);
  if (gripper_roadmap_options_check(who, W, opt) || franka_counts_check(who, S) ||
      franka_env_offset_check(who, env_offset, B) || franka_rows_check(who, B, W * 16, "B x W x 16 pose entries"))
    return 1;
  MPX_REQUIRE(point_radius >= 0.0f && point_radius < big, "%s: point_radius must be finite and >= 0", who);
  MPX_REQUIRE(field_slack >= 0.0f && field_slack < big, "%s: field_slack must be finite and >= 0", who);
  FieldGrid G = {};
  const float slack_margin = opt.check_margin + field_slack;  // (float32, summed once: the kernel's right-hand side)
  if (field) {
    if (field_grid_check(who, grid, G)) return 1;
    MPX_REQUIRE(S > 0, "%s: a field without collision spheres to test it with", who);
    // The joint roadmap's bound, although the gripper's largest sphere is smaller: one rule for every reader of a field.
    const float need = MPX_FRANKA_MAX_SPHERE_RADIUS + point_radius + (opt.clearance > 0.0f ? opt.clearance : 0.0f) + slack_margin;
    MPX_REQUIRE(G.trunc > need,
                "%s: grid trunc = %g, need more than %g = largest sphere radius %g + point_radius + max(clearance, 0) + "
                "check_margin + field_slack (an obstacle in between would be missed)",
                who, (double)G.trunc, (double)need, (double)MPX_FRANKA_MAX_SPHERE_RADIUS);
  }
  if (B == 0) return 0;
  MPX_REQUIRE(poses && status && path && hops, "%s: NULL output (poses, status, path, hops)", who);
  MPX_REQUIRE(start_pose && goal_pose && bounds, "%s: NULL operand (start_pose, goal_pose, bounds)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  const size_t lds = 4 * gripper_roadmap_cloud_lds_words(opt.nodes);  // 33 804 B at 256 nodes
  hipLaunchKernelGGL(gripper_roadmap_cloud_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), start_pose,
                     goal_pose, W, bounds, finger, sph_centers, sph_radii, sph_link, S, field, G, point_radius, slack_margin,
                     opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, poses, status, path, hops, nodes,
                     edge_state, rounds);
  MPX_LAUNCH_CHECK(who);
}
