// roadmap_cloud.hip -- roadmap.hip's lazy roadmap against a POINT CLOUD: the global half in front of cloud_field.hip's local
// optimiser.  What makes a configuration invalid is read off the truncated distance field that already steers that planner
// (field_device.h: 8 cached global loads and 7 lerps per collision sphere) instead of a walk over the cloud's N points; the
// self test is the planner's.  The field APPROXIMATES the distance (within (sqrt(3)/2) h of it), so the roadmap's verdicts
// are a guide: what mpx_franka_plan_cloud_seeded returns is still judged by the exact swept-sphere test.  Nodes, edges, the
// search, the statuses and the seed trajectory are mpx_franka_roadmap's, by the same text (roadmap_search.inc,
// roadmap_tail.inc); the contract is stated in include/mpinets_hip.h.
// Behind it, franka_shortcut_cloud_kernel is roadmap.hip's franka_shortcut_kernel with this file's validity test (one body,
// shortcut_kernel.inc).
//
// franka_roadmap_kernel's structure: one workgroup of 256 threads per problem, everything but the field in LDS, no scratch
// memory and no global atomics; thread = node, thread = interior configuration of the round's untested edges, thread =
// waypoint.  Every branch around a barrier is workgroup-uniform: it reads a value from LDS behind a barrier, or a barrier's
// own reduction.
#include "common.h"
#include "franka_host.h"
#include "plan_device.h"
#include "field_device.h"
#include "roadmap_device.h"

// LDS, in 4-byte words: roadmap.hip's layout without the primitive rows: [nodes V x 7 | dist 2 x V (later: cumulative and
// edge lengths) | two trajectories 64 x 7 | pred, path, rev, pieces, blocked, valid: V ints each | first V + 1 | hops | edge bits]
__host__ __device__ static inline size_t roadmap_cloud_lds_words(int V) {
  return (size_t)V * 7 + 2 * (size_t)V + 2 * 64 * 7 + 6 * (size_t)V + (size_t)V + 1 + 1 + ((size_t)V * V + 15) / 16;
}

// bits PLAN_BIT_ENV / PLAN_BIT_SELF of one configuration.  A sphere is blocked when its centre is inside the grid, the
// field is not saturated there and d = ((D - point_radius) - r_s) - clearance <= slack_margin (= check_margin + field_slack,
// summed once on the host); `f` is ONE environment's nodes, nullptr: no environment test.  (A NaN centre is outside the
// grid: it reads no memory.)
__device__ __forceinline__ int roadmap_cloud_bits(const float *q, float finger, const float *__restrict__ sc,
                                                  const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                                  const float *__restrict__ f, const FieldGrid &G, float point_radius,
                                                  float clearance, float slack_margin, bool test_self, float self_margin) {
  int bits = 0;
  franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
    constexpr int id = decltype(ID)::value;
    if (f) {
      for (int s = 0; s < S; ++s) {
        if (sl[s] != id) continue;  // (wave-uniform)
        float x, y, z, D, gx, gy, gz;
        rigid_apply(g, sc[3 * s + 0], sc[3 * s + 1], sc[3 * s + 2], x, y, z);
        const bool inside = field_sample<false>(f, G, x, y, z, D, gx, gy, gz);
        const float d = ((D - point_radius) - sr[s]) - clearance;
        if (inside && D < G.trunc && d <= slack_margin) bits |= PLAN_BIT_ENV;
      }
    }
    if constexpr (franka_self_sphere(id) >= 0) {
      if (test_self && franka_self_hit<id>(g, self_margin)) bits |= PLAN_BIT_SELF;
    }
  });
  return bits;
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    franka_roadmap_cloud_kernel(const float *__restrict__ q_start, const float *__restrict__ q_goal, int T, float finger,
                                const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,
                                const int32_t *__restrict__ sl, int S, const float *__restrict__ field, FieldGrid G,
                                float point_radius, float slack_margin, mpx_roadmap_options opt, uint32_t seed_lo,
                                uint32_t seed_hi, uint32_t env0, float *__restrict__ traj, int32_t *__restrict__ status,
                                int32_t *__restrict__ path_out, int32_t *__restrict__ hops_out, float *__restrict__ nodes_out,
                                uint8_t *__restrict__ edge_out, int32_t *__restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int V = opt.nodes;
  float *nodes = lds;
  float *dist = nodes + V * 7;
  float *tbuf = dist + 2 * V;
  int *pred = reinterpret_cast<int *>(tbuf + 2 * 64 * 7);
  int *path = pred + V, *rev = path + V, *pieces = rev + V, *blocked = pieces + V, *valid = blocked + V;
  int *first = valid + V;  // first[i]: index of edge i's first interior configuration among the round's tests
  int *hops_lds = first + V + 1;
  unsigned *ebits = reinterpret_cast<unsigned *>(hops_lds + 1);
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float inf = __builtin_inff(), nan = __builtin_nanf("");

  float lo[7], hi[7], qs[7], qg[7];
  plan_endpoints(limits, q_start, q_goal, b, lo, hi, qs, qg);
  for (int i = tid; i < (V * V + 15) / 16; i += ROADMAP_THREADS) ebits[i] = 0u;

  // ---- nodes: thread = node (mpx_franka_roadmap's draw: the same seed gives the same nodes) ---------------------------------------
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
  __syncthreads();  // (the nodes, the cleared edge bits)

  const bool test_self = opt.check_self != 0;
  const float *fenv = (field != nullptr && S > 0) ? field + (size_t)b * ((size_t)G.nx * G.ny * G.nz) : nullptr;
  if (tid < V)
    valid[tid] = inside && roadmap_cloud_bits(mine, finger, sc, sr, sl, S, fenv, G, point_radius, opt.clearance, slack_margin,
                                              test_self, opt.check_margin) == 0;
  __syncthreads();

  // ---- the lazy search: roadmap.hip's, with the field as the validity test ---------------------------------------------------------
#define ROADMAP_SEARCH_LENGTH(a, b) roadmap_length(a, b)
#define ROADMAP_SEARCH_POINT(a, e, f, q) \
  _Pragma("unroll") for (int j = 0; j < 7; ++j) q[j] = mpx_fma(f, nodes[e * 7 + j] - nodes[a * 7 + j], nodes[a * 7 + j]);
#define ROADMAP_SEARCH_HIT(q) \
  roadmap_cloud_bits(q, finger, sc, sr, sl, S, fenv, G, point_radius, opt.clearance, slack_margin, test_self, opt.check_margin)
#include "roadmap_search.inc"
#undef ROADMAP_SEARCH_LENGTH
#undef ROADMAP_SEARCH_POINT
#undef ROADMAP_SEARCH_HIT

#include "roadmap_tail.inc"
}

MPX_EXPORT int mpx_franka_roadmap_cloud(const float *q_start, const float *q_goal, int B, int T, float finger,
                                        const float *limits, const float *sph_centers, const float *sph_radii,
                                        const int32_t *sph_link, int S, const float *field, const mpx_field_grid *grid,
                                        float point_radius, float field_slack, const mpx_roadmap_options *options,
                                        uint64_t seed, int64_t env_offset, float *traj, int32_t *status, int32_t *path,
                                        int32_t *hops, float *nodes, uint8_t *edge_state, int32_t *rounds, mpx_stream_t stream) {
  const char *who = "mpx_franka_roadmap_cloud";
  const mpx_roadmap_options opt = options ? *options : franka_roadmap_defaults();
  const float big = __builtin_huge_valf();
  MPX_REQUIRE(B >= 0 && S >= 0, "%s: negative size", who);
  if (franka_roadmap_options_check(who, T, opt) || franka_counts_check(who, S) || franka_env_offset_check(who, env_offset, B))
    return 1;
  MPX_REQUIRE(point_radius >= 0.0f && point_radius < big, "%s: point_radius must be finite and >= 0", who);
  MPX_REQUIRE(field_slack >= 0.0f && field_slack < big, "%s: field_slack must be finite and >= 0", who);
  FieldGrid G = {};
  const float slack_margin = opt.check_margin + field_slack;  // (float32, summed once: the kernel's right-hand side)
  if (field) {
    if (field_grid_check(who, grid, G)) return 1;
    MPX_REQUIRE(S > 0, "%s: a field without collision spheres to test it with", who);
    // An obstacle farther than trunc from a centre is not seen.  The largest radius is bounded by the table's constant
    // (MPX_FRANKA_MAX_SPHERE_RADIUS: reading sph_radii here would need a device copy).
    const float need = MPX_FRANKA_MAX_SPHERE_RADIUS + point_radius + (opt.clearance > 0.0f ? opt.clearance : 0.0f) + slack_margin;
    MPX_REQUIRE(G.trunc > need,
                "%s: grid trunc = %g, need more than %g = largest sphere radius %g + point_radius + max(clearance, 0) + "
                "check_margin + field_slack (an obstacle in between would be missed)",
                who, (double)G.trunc, (double)need, (double)MPX_FRANKA_MAX_SPHERE_RADIUS);
  }
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status && path && hops, "%s: NULL output (traj, status, path, hops)", who);
  MPX_REQUIRE(q_start && q_goal && limits, "%s: NULL operand (q_start, q_goal, limits)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  const size_t lds = 4 * roadmap_cloud_lds_words(opt.nodes);  // 36 360 B at 256 nodes
  hipLaunchKernelGGL(franka_roadmap_cloud_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), q_start, q_goal,
                     T, finger, limits, sph_centers, sph_radii, sph_link, S, field, G, point_radius, slack_margin, opt,
                     (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, traj, status, path, hops, nodes, edge_state,
                     rounds);
  MPX_LAUNCH_CHECK(who);
}

// ---- shortcutting a polyline: shortcut_kernel.inc with the field as the validity test (roadmap_cloud_bits' rule) ---------------------
// LDS: shortcut_lds_words(P)
__global__ void __launch_bounds__(ROADMAP_THREADS)
    franka_shortcut_cloud_kernel(const float *__restrict__ points, const int32_t *__restrict__ count, int Pin, int T,
                                 float finger, const float *__restrict__ sc, const float *__restrict__ sr,
                                 const int32_t *__restrict__ sl, int S, const float *__restrict__ field, FieldGrid G,
                                 float point_radius, float slack_margin, mpx_shortcut_options opt, float *__restrict__ traj,
                                 int32_t *__restrict__ status, float *__restrict__ points_out, int32_t *__restrict__ count_out,
                                 float *__restrict__ length, int32_t *__restrict__ chords_out,
                                 int32_t *__restrict__ configs_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  SHORTCUT_LDS_CARVE(lds, opt.points)
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const bool test_self = opt.check_self != 0;
  const float *fenv = (field != nullptr && S > 0) ? field + (size_t)b * ((size_t)G.nx * G.ny * G.nz) : nullptr;
#define SHORTCUT_HIT(q) \
  roadmap_cloud_bits(q, finger, sc, sr, sl, S, fenv, G, point_radius, opt.clearance, slack_margin, test_self, opt.check_margin)
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

MPX_EXPORT int mpx_franka_shortcut_cloud(const float *points, const int32_t *count, int B, int Pin, int T, float finger,
                                         const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                         const float *field, const mpx_field_grid *grid, float point_radius, float field_slack,
                                         const mpx_shortcut_options *options, float *traj, int32_t *status, float *points_out,
                                         int32_t *count_out, float *length, int32_t *chords, int32_t *configs,
                                         mpx_stream_t stream) {
  const char *who = "mpx_franka_shortcut_cloud";
  const mpx_shortcut_options opt = options ? *options : franka_shortcut_defaults();
  const float big = __builtin_huge_valf();
  MPX_REQUIRE(B >= 0 && S >= 0, "%s: negative size", who);
  if (franka_shortcut_options_check(who, T, Pin, opt) || franka_counts_check(who, S)) return 1;
  MPX_REQUIRE(point_radius >= 0.0f && point_radius < big, "%s: point_radius must be finite and >= 0", who);
  MPX_REQUIRE(field_slack >= 0.0f && field_slack < big, "%s: field_slack must be finite and >= 0", who);
  FieldGrid G = {};
  const float slack_margin = opt.check_margin + field_slack;  // (float32, summed once: the kernel's right-hand side)
  if (field) {  // (mpx_franka_roadmap_cloud's refusals, in its words)
    if (field_grid_check(who, grid, G)) return 1;
    MPX_REQUIRE(S > 0, "%s: a field without collision spheres to test it with", who);
    const float need = MPX_FRANKA_MAX_SPHERE_RADIUS + point_radius + (opt.clearance > 0.0f ? opt.clearance : 0.0f) + slack_margin;
    MPX_REQUIRE(G.trunc > need,
                "%s: grid trunc = %g, need more than %g = largest sphere radius %g + point_radius + max(clearance, 0) + "
                "check_margin + field_slack (an obstacle in between would be missed)",
                who, (double)G.trunc, (double)need, (double)MPX_FRANKA_MAX_SPHERE_RADIUS);
  }
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status && points_out && count_out && length,
              "%s: NULL output (traj, status, points_out, count_out, length)", who);
  MPX_REQUIRE(points && count, "%s: NULL operand (points, count)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  const size_t lds = 4 * shortcut_lds_words(opt.points);  // 27 160 B at 256 points
  hipLaunchKernelGGL(franka_shortcut_cloud_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), points, count,
                     Pin, T, finger, sph_centers, sph_radii, sph_link, S, field, G, point_radius, slack_margin, opt, traj,
                     status, points_out, count_out, length, chords, configs);
  MPX_LAUNCH_CHECK(who);
}
