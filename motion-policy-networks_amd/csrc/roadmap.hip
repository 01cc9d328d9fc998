// roadmap.hip -- a lazy probabilistic roadmap per problem: the global half of what the reference's data generator asks of
// OMPL (data_pipeline/gen_data.py:106-153), in front of plan.hip's local optimiser.  V configurations (start, goal, V - 2
// Philox draws inside the limits) are judged by the planner's own validity test (plan_prims_device.h); the shortest path from
// start to goal over the complete graph is searched with every untested edge counted as free, the untested edges of that path
// are then tested in full, and the search repeats without the blocked ones until a path survives.  The surviving polyline,
// resampled to T waypoints and rounded at its corners, is a candidate for mpx_franka_plan_seeded.  The contract (draws, edge
// pieces, sweeps, resampling) is stated in include/mpinets_hip.h.
//
// One workgroup of 256 threads per problem, everything in LDS, no scratch memory and no global atomics.  Three mappings:
// thread = node (the node draw, node validity, one Bellman-Ford sweep: V <= 256), thread = interior configuration across the
// concatenated untested edges of the round's path (the planner's validity-sweep mapping, in passes of 256), thread = waypoint
// (resampling and the corner filter: T <= 64).  The path walk and the prefix sums over its <= V - 1 edges are serial on
// thread 0.  Every branch around a barrier is workgroup-uniform: it reads a value from LDS behind a barrier, or a barrier's
// own reduction.  The search itself is roadmap_search.inc, shared with gripper_roadmap.hip (the gripper's roadmap in SE(3)) and
// roadmap_cloud.hip (this roadmap against a point cloud's distance field), which also shares what follows it, roadmap_tail.inc.
// Behind the roadmap, franka_shortcut_kernel shortens a polyline (the roadmap's path, or any caller's) with the same validity
// test: its body is shortcut_kernel.inc, shared with roadmap_cloud.hip's form and with the gripper's shortcut kernels
// (gripper_shortcut.hip), and it ends with the seed trajectory's statements (roadmap_traj.inc, which roadmap_tail.inc ends with).
#include "common.h"
#include "franka_host.h"
#include "plan_prims_device.h"
#include "roadmap_device.h"

// LDS, in 4-byte words: [128 primitive rows x 16 | nodes V x 7 | dist 2 x V (later: cumulative and edge lengths) |
// two trajectories 64 x 7 | pred, path, rev, pieces, blocked, valid: V ints each | first V + 1 | hops | edge bits]
__host__ __device__ static inline size_t roadmap_lds_words(int V) {
  return (size_t)128 * 16 + (size_t)V * 7 + 2 * (size_t)V + 2 * 64 * 7 + 6 * (size_t)V + (size_t)V + 1 + 1 +
         ((size_t)V * V + 15) / 16;
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    franka_roadmap_kernel(const float *__restrict__ q_start, const float *__restrict__ q_goal, int T, float finger,
                          const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,
                          const int32_t *__restrict__ sl, int S, const float *__restrict__ cub_f,
                          const float *__restrict__ cub_d, int M1, const float *__restrict__ cyl_f,
                          const float *__restrict__ cyl_r, const float *__restrict__ cyl_h, int M2, mpx_roadmap_options opt,
                          uint32_t seed_lo, uint32_t seed_hi, uint32_t env0, float *__restrict__ traj,
                          int32_t *__restrict__ status, int32_t *__restrict__ path_out, int32_t *__restrict__ hops_out,
                          float *__restrict__ nodes_out, uint8_t *__restrict__ edge_out, int32_t *__restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int V = opt.nodes;
  float *prim_rows = lds;
  float *nodes = prim_rows + 128 * 16;
  float *dist = nodes + V * 7;
  float *tbuf = dist + 2 * V;
  int *pred = reinterpret_cast<int *>(tbuf + 2 * 64 * 7);
  int *path = pred + V, *rev = path + V, *pieces = rev + V, *blocked = pieces + V, *valid = blocked + V;
  int *first = valid + V;  // first[i]: index of edge i's first interior configuration among the round's tests
  int *hops_lds = first + V + 1;
  unsigned *ebits = reinterpret_cast<unsigned *>(hops_lds + 1);
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");

  float lo[7], hi[7], qs[7], qg[7];
  plan_endpoints(limits, q_start, q_goal, b, lo, hi, qs, qg);

#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  for (int i = tid; i < (V * V + 15) / 16; i += ROADMAP_THREADS) ebits[i] = 0u;

  // ---- nodes: thread = node ------------------------------------------------------------------------------------------------------
  float mine[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool inside = true;
  if (tid < V) {
    const Philox p0 = philox4x32(2u * (uint32_t)tid, env0 + (uint32_t)b, STREAM_ROADMAP, 0u, seed_lo, seed_hi);
    const Philox p1 = philox4x32(2u * (uint32_t)tid + 1u, env0 + (uint32_t)b, STREAM_ROADMAP, 0u, seed_lo, seed_hi);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float drawn = mpx_fma(u01(j < 4 ? p0.c[j] : p1.c[j - 4]), hi[j] - lo[j], lo[j]);
      mine[j] = tid == 0 ? qs[j] : tid == 1 ? qg[j] : drawn;
      inside &= (mine[j] >= lo[j]) & (mine[j] <= hi[j]);  // (an endpoint: NaN fails)
      nodes[tid * 7 + j] = mine[j];
      if (nodes_out) nodes_out[((size_t)b * V + tid) * 7 + j] = mine[j];
    }
  }
  __syncthreads();  // (the primitive rows, the nodes, the cleared edge bits)

  const bool test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;
  if (tid < V)
    valid[tid] = inside && plan_config_bits(mine, finger, sc, sr, sl, S, prim_rows, n_cub, n_cyl, reach, test_self,
                                            opt.check_margin) == 0;
  __syncthreads();

  // ---- the lazy search -----------------------------------------------------------------------------------------------------------
#define ROADMAP_SEARCH_LENGTH(a, b) roadmap_length(a, b)
#define ROADMAP_SEARCH_POINT(a, e, f, q) \
  _Pragma("unroll") for (int j = 0; j < 7; ++j) q[j] = mpx_fma(f, nodes[e * 7 + j] - nodes[a * 7 + j], nodes[a * 7 + j]);
#define ROADMAP_SEARCH_HIT(q) \
  plan_config_bits(q, finger, sc, sr, sl, S, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin)
#include "roadmap_search.inc"
#undef ROADMAP_SEARCH_LENGTH
#undef ROADMAP_SEARCH_POINT
#undef ROADMAP_SEARCH_HIT

#include "roadmap_tail.inc"
}

MPX_EXPORT int mpx_franka_roadmap(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                                  const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                  const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                                  const float *cyl_radii, const float *cyl_heights, int M2, const mpx_roadmap_options *options,
                                  uint64_t seed, int64_t env_offset, float *traj, int32_t *status, int32_t *path,
                                  int32_t *hops, float *nodes, uint8_t *edge_state, int32_t *rounds, mpx_stream_t stream) {
  const char *who = "mpx_franka_roadmap";
  const mpx_roadmap_options opt = options ? *options : franka_roadmap_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (franka_roadmap_options_check(who, T, opt) || franka_counts_check(who, S, M1, M2) || franka_env_offset_check(who, env_offset, B))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status && path && hops, "%s: NULL output (traj, status, path, hops)", who);
  MPX_REQUIRE(q_start && q_goal && limits, "%s: NULL operand (q_start, q_goal, limits)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const size_t lds = 4 * roadmap_lds_words(opt.nodes);  // 44 552 B at 256 nodes
  hipLaunchKernelGGL(franka_roadmap_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), q_start, q_goal, T,
                     finger, limits, sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames,
                     cyl_radii, cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, traj,
                     status, path, hops, nodes, edge_state, rounds);
  MPX_LAUNCH_CHECK(who);
}

// ---- shortcutting a polyline: shortcut_kernel.inc with the planner's validity test --------------------------------------------------
// LDS: [128 primitive rows x 16 | shortcut_lds_words(P)]
__global__ void __launch_bounds__(ROADMAP_THREADS)
    franka_shortcut_kernel(const float *__restrict__ points, const int32_t *__restrict__ count, int Pin, int T, float finger,
                           const float *__restrict__ sc, const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                           const float *__restrict__ cub_f, const float *__restrict__ cub_d, int M1,
                           const float *__restrict__ cyl_f, const float *__restrict__ cyl_r, const float *__restrict__ cyl_h,
                           int M2, mpx_shortcut_options opt, float *__restrict__ traj, int32_t *__restrict__ status,
                           float *__restrict__ points_out, int32_t *__restrict__ count_out, float *__restrict__ length,
                           int32_t *__restrict__ chords_out, int32_t *__restrict__ configs_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *prim_rows = lds;
  SHORTCUT_LDS_CARVE(prim_rows + 128 * 16, opt.points)
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  const bool test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;
  // (the body's first barrier publishes the primitive rows)
#define SHORTCUT_HIT(q) \
  plan_config_bits(q, finger, sc, sr, sl, S, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin)
#define SHORTCUT_LENGTH(a, e) roadmap_length(a, e)
#define SHORTCUT_POINT(a, e, f, q) \
  _Pragma("unroll") for (int j = 0; j < 7; ++j) q[j] = mpx_fma(f, e[j] - a[j], a[j]);
#include "shortcut_kernel.inc"
#undef SHORTCUT_HIT
#undef SHORTCUT_LENGTH
#undef SHORTCUT_POINT
  // ---- the seed trajectory over the returned polyline (vertex i is nodes[path[i]], path[i] = i) --------------------------------------
  const int V = P, hops = n - 1;
  const float *nodes = cur;
  float qs[7], qg[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) qs[j] = st == 0 ? cur[j] : nan, qg[j] = st == 0 ? cur[(n - 1) * 7 + j] : nan;
#include "roadmap_traj.inc"
}

MPX_EXPORT int mpx_franka_shortcut(const float *points, const int32_t *count, int B, int Pin, int T, float finger,
                                   const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                   const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                                   const float *cyl_radii, const float *cyl_heights, int M2,
                                   const mpx_shortcut_options *options, float *traj, int32_t *status, float *points_out,
                                   int32_t *count_out, float *length, int32_t *chords, int32_t *configs, mpx_stream_t stream) {
  const char *who = "mpx_franka_shortcut";
  const mpx_shortcut_options opt = options ? *options : franka_shortcut_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (franka_shortcut_options_check(who, T, Pin, opt) || franka_counts_check(who, S, M1, M2)) return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status && points_out && count_out && length,
              "%s: NULL output (traj, status, points_out, count_out, length)", who);
  MPX_REQUIRE(points && count, "%s: NULL operand (points, count)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const size_t lds = 4 * ((size_t)128 * 16 + shortcut_lds_words(opt.points));  // 35 352 B at 256 points
  hipLaunchKernelGGL(franka_shortcut_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), points, count, Pin,
                     T, finger, sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii,
                     cyl_heights, M2, opt, traj, status, points_out, count_out, length, chords, configs);
  MPX_LAUNCH_CHECK(who);
}
