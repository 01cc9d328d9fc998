// cloud_collision.hip -- swept-sphere collision check of Franka trajectories against one point cloud per environment.
//
// The primitive check (franka.hip: mpx_franka_collision) needs the scene as cuboids and cylinders.  The policy consumes
// a point cloud, and a depth cloud (depth.hip) or a captured cloud (the reference's ROS planner,
// interactive_demo/mpinets_ros/nodes/planning_node.py:78-151, plans from `obstacle_pc [4096,3]` alone) has no primitives
// behind it.  This file asks the same question of the cloud itself: does any of the robot's S spheres, at any waypoint,
// come within its radius of any point.
//
// Shape (franka_collision_env_kernel's): a workgroup owns ONE environment and a chunk of up to MPX_CLOUD_TC of its
// waypoints.  FK runs once per waypoint on the first lanes, frames parked in LDS; the (waypoint, sphere) pairs of the chunk
// are flattened over the lanes and a thread keeps all its pairs' centres (<= PPT) in registers.  The frames are dead
// from then on and the same LDS becomes a double-buffered tile of MPX_CLOUD_TILE points as 16-byte rows: while the
// workgroup walks tile k its threads hold tile k + 1 in registers (global loads in flight), one barrier per tile.
// The walk is point-outer, pair-inner: one broadcast ds_read_b128 (every lane the same address) feeds PPT independent
// chains of 3 subtractions + mpx_sqdist (1 multiply, 2 fma) + 1 v_min (flags only), or + compare and two selects when the
// nearest index is wanted.  N is unbounded (tiles loop), `counts` trims the walk.
//
// Pinned arithmetic (the contract in include/mpinets_hip.h): centres by franka_fk_frames + rigid_apply exactly as
// mpx_franka_spheres computes them; d2 = mpx_sqdist(c - p); R = (r_s + point_radius) + clearance, hit iff d2 <= R * R;
// best starts at +inf and moves only on d2 < best, points ascending.
//
// Flags-only form with the cull (MPX_VARIANT_CLOUD_CULL, default on): the workgroup first takes the axis-aligned box of
// its centres, inflated by more than the largest R (see `infl` below for why that is conservative in float32), and a
// point strictly outside the box on any axis is dropped while its tile is staged: the survivors of a tile are compacted
// into the LDS rows (ballot + prefix popcount within a wave, one LDS atomic per wave for its slot range -- their order
// does not matter to a minimum).  After each tile the workgroup stops if one of its pairs has hit.
//
// Per-waypoint form (mpx_franka_cloud_collision_each, EACH below): the same walk, one verdict per waypoint instead of one
// flag per environment.  An optional `active` mask [B,T] says which waypoints are tested; the first lanes read it beside
// their FK and wave 0 ballots it into a 64-bit mask of the chunk.  A pair that lands on an inactive waypoint is replaced
// as padding is -- here by sphere 0 of the chunk's FIRST ACTIVE waypoint, so the cull box is that of the active pairs alone
// -- and neither padding nor a replaced pair is ever folded into a verdict.  A thread folds its pairs' hits into a 64-bit
// mask in LDS (one ds_or_b64 when it has any); threads tid < nt store hit[b, t0 + tid] from it: plain vector stores, every
// output written exactly once, no global atomics.  With the cull the fold runs after every tile into one of two masks
// (k & 1: hits only accumulate, so or-ing the thread's whole current set into the mask of two tiles ago gives this tile's;
// the other mask is still being read) and the workgroup stops once every active waypoint of its chunk has a hit -- not
// at the first hit.  A chunk with nothing active writes its zeros and leaves before the walk.
//
// The statements of both kernel templates are ONE text, cloud_collision_walk.inc, included into each: as a __device__
// function the shared body compiled the flag kernels differently (__restrict__ on its parameters is not __restrict__ on a
// kernel's), and their instruction streams are pinned (tools/isa_diff.py, profiles/ik_cloud_timing.md).
#include "common.h"
#include "franka_host.h"
#include "franka_device.h"

constexpr int FRAME_FLOATS = MPX_NUM_FRAMES * 12;  // 180
constexpr int CC_TC = MPX_CLOUD_TC;                // waypoints per workgroup
constexpr int CC_TILE = MPX_CLOUD_TILE;            // points per LDS tile
static_assert(CC_TC >= 1 && CC_TC <= 64 && CC_TC * 64 <= 16 * 256,
              "MPX_CLOUD_TC: FK runs on one thread per waypoint and a thread holds at most 16 (waypoint, sphere) pairs");
static_assert(CC_TILE % 256 == 0, "MPX_CLOUD_TILE: whole rows of the largest workgroup");

template <int BLOCK, int PPT, bool FULL, bool CULL>
__global__ void __launch_bounds__(BLOCK)
    franka_cloud_collision_kernel(const float *__restrict__ q, int T, int chunks, float finger, const float *__restrict__ sc,
                                  const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                  const float *__restrict__ cloud, int64_t cbs, int cps, int N,
                                  const int32_t *__restrict__ counts, float point_radius, float clearance,
                                  int32_t *__restrict__ flags, float *__restrict__ min_dist, int32_t *__restrict__ nearest) {
  constexpr bool EACH = false;
  constexpr const int32_t *active = nullptr;
  constexpr int32_t *hit_out = nullptr;
#include "cloud_collision_walk.inc"
}

template <int BLOCK, int PPT, bool CULL>
__global__ void __launch_bounds__(BLOCK)
    franka_cloud_collision_each_kernel(const float *__restrict__ q, int T, int chunks, float finger,
                                       const float *__restrict__ sc, const float *__restrict__ sr,
                                       const int32_t *__restrict__ sl, int S, const float *__restrict__ cloud, int64_t cbs,
                                       int cps, int N, const int32_t *__restrict__ counts, float point_radius, float clearance,
                                       const int32_t *__restrict__ active, int32_t *__restrict__ hit_out) {
  constexpr bool FULL = false, EACH = true;
  constexpr int32_t *flags = nullptr, *nearest = nullptr;
  constexpr float *min_dist = nullptr;
#include "cloud_collision_walk.inc"
}

MPX_EXPORT int mpx_franka_cloud_collision(const float *q, int B, int T, float finger, const float *sph_centers,
                                          const float *sph_radii, const int32_t *sph_link, int S, const float *cloud,
                                          int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                                          float point_radius, float clearance, int32_t *flags, float *min_dist,
                                          int32_t *nearest, mpx_stream_t stream) {
  const char *who = "mpx_franka_cloud_collision";
  if (franka_cloud_operand_check(who, B, S, N, point_radius, clearance, cloud_point_stride) || franka_rows_check(who, B, T, "B*T") ||
      franka_counts_check(who, S))
    return 1;
  if (B == 0 || T == 0 || S == 0) return 0;
  const bool full = min_dist != nullptr || nearest != nullptr;
  if (N == 0 && !full) return 0;  // no point, no hit
  MPX_REQUIRE(q && sph_centers && sph_radii && sph_link && flags && (cloud || N == 0), "%s: NULL operand", who);
  const int chunks = cdiv(T, CC_TC);
  MPX_REQUIRE((int64_t)B * chunks < (int64_t)1 << 31, "%s: too many workgroups", who);
  const bool cull = !full && mpx_get_variant(MPX_VARIANT_CLOUD_CULL) != 0;
  const int nt = min(T, CC_TC);
  const size_t lds_bytes = sizeof(float) * (size_t)max(nt * FRAME_FLOATS, 2 * CC_TILE * 4);
  franka_cloud_launch_form(nt * S, [&](auto BLOCK, auto PPT) {
    constexpr int block = decltype(BLOCK)::value, ppt = decltype(PPT)::value;
    auto kernel = full   ? franka_cloud_collision_kernel<block, ppt, true, false>
                  : cull ? franka_cloud_collision_kernel<block, ppt, false, true>
                         : franka_cloud_collision_kernel<block, ppt, false, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * chunks)), dim3(block), lds_bytes, mpx_s(stream), q, T, chunks, finger,
                       sph_centers, sph_radii, sph_link, S, cloud, cloud_batch_stride, cloud_point_stride, N, counts,
                       point_radius, clearance, flags, min_dist, nearest);
  });
  MPX_LAUNCH_CHECK(who);
}

__global__ void __launch_bounds__(256) cloud_each_zero_kernel(int32_t *__restrict__ hit, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) hit[i] = 0;
}

MPX_EXPORT int mpx_franka_cloud_collision_each(const float *q, int B, int T, float finger, const float *sph_centers,
                                               const float *sph_radii, const int32_t *sph_link, int S, const float *cloud,
                                               int64_t cloud_batch_stride, int cloud_point_stride, int N,
                                               const int32_t *counts, float point_radius, float clearance,
                                               const int32_t *active, int32_t *hit, mpx_stream_t stream) {
  const char *who = "mpx_franka_cloud_collision_each";
  if (franka_cloud_operand_check(who, B, S, N, point_radius, clearance, cloud_point_stride) || franka_rows_check(who, B, T, "B*T") ||
      franka_counts_check(who, S))
    return 1;
  if (B == 0 || T == 0) return 0;
  MPX_REQUIRE(hit, "%s: NULL output (hit)", who);
  if (S == 0 || N == 0) {  // no sphere or no point: no hit, but every verdict is still written
    const int64_t n = (int64_t)B * T;
    hipLaunchKernelGGL(cloud_each_zero_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, mpx_s(stream), hit, n);
    MPX_LAUNCH_CHECK(who);
  }
  MPX_REQUIRE(q && sph_centers && sph_radii && sph_link && cloud, "%s: NULL operand", who);
  const int chunks = cdiv(T, CC_TC);
  MPX_REQUIRE((int64_t)B * chunks < (int64_t)1 << 31, "%s: too many workgroups", who);
  const bool cull = mpx_get_variant(MPX_VARIANT_CLOUD_CULL) != 0;
  const int nt = min(T, CC_TC);
  const size_t lds_bytes = sizeof(float) * (size_t)max(nt * FRAME_FLOATS, 2 * CC_TILE * 4);
  franka_cloud_launch_form(nt * S, [&](auto BLOCK, auto PPT) {
    constexpr int block = decltype(BLOCK)::value, ppt = decltype(PPT)::value;
    auto kernel = cull ? franka_cloud_collision_each_kernel<block, ppt, true> : franka_cloud_collision_each_kernel<block, ppt, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * chunks)), dim3(block), lds_bytes, mpx_s(stream), q, T, chunks, finger,
                       sph_centers, sph_radii, sph_link, S, cloud, cloud_batch_stride, cloud_point_stride, N, counts,
                       point_radius, clearance, active, hit);
  });
  MPX_LAUNCH_CHECK(who);
}
