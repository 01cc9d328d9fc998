// follow_cloud.hip -- mpx_franka_follow against a POINT CLOUD: the reactive follower of follow.hip (still the stand-in for
// the reference's Geometric Fabrics expert, NOT Lula's fabric, no parity claimed) with the cloud's truncated distance field
// as its obstacle term and mpx_franka_cloud_collision as the judge of its environment bit -- the field steers, the exact
// test judges, as in cloud_field.hip's planner.  The contract is stated in include/mpinets_hip.h.
//
// One wave per problem, as in follow.hip: the state, the joint origins and axes and the 6x6 solve are wave-uniform; in the
// obstacle term the lane is the collision sphere (S <= 64), its centre is sampled with field_sample<true> (8 loads, issued
// together), and the seven sums over spheres are follow.hip's butterfly of __shfl_xor in a fixed order.  There are no
// primitive rows: the only LDS is the 64 x 7 waypoint buffer.  What this file states is what differs from follow.hip: the
// obstacle term, the test of a fresh start, the bad-input return and the verdict.  The state load, steps 1 to 4 and 6 to 7
// of the time loop, the retiming and the miss test are the statement blocks both kernels include (follow_state.inc,
// follow_step_head.inc, follow_step_tail.inc, follow_retime.inc, follow_miss.inc), the pose helpers and the state write-out
// are follow_device.h's; both kernels have the instruction streams they had with a copy each
// (profiles/follow_shared_isa.md).
//
// The entry enqueues, on the caller's stream and without a host synchronisation: a memset of the two flag rows, for a fresh
// rollout a flags call on q_start as [B,1,7], the rollout kernel (steps, retiming, the jerk / self / miss bits, the T
// waypoints and the refined configurations to scratch), one flags call over the refined configurations, and a finish
// kernel that ORs PLAN_BIT_ENV in and writes status, bits, traj and traj_any.
#include "common.h"
#include "franka_host.h"
#include "franka_device.h"
#include "dls_device.h"
#include "field_device.h"
#include "plan_device.h"
#include "follow_device.h"

struct FollowCloudScratch {  // all in 4-byte words, from the start of `scratch`
  size_t refined;            // float [B, R, 7]: what the one flags call over the trajectories reads
  size_t waypoints;          // float [B, T, 7]: the retimed waypoints (traj_any's rows)
  size_t start_flags;        // int32 [B] then traj_flags int32 [B]: zeroed on the stream, OR-ed into by the flag calls
  size_t traj_flags;
  size_t pre_bits;           // int32 [B]: the jerk, self and miss bits (15 on bad input)
  size_t bad;                // int32 [B]: status 2
  size_t total_bytes;
};
static FollowCloudScratch follow_cloud_layout(int B, int T, int substeps) {
  FollowCloudScratch L;
  const size_t R = (size_t)(T - 1) * substeps + 1, b = (size_t)B;
  size_t at = 0;
  L.refined = at, at += b * R * 7;
  L.waypoints = at, at += b * (size_t)T * 7;
  L.start_flags = at, at += b;
  L.traj_flags = at, at += b;
  L.pre_bits = at, at += b;
  L.bad = at, at += b;
  L.total_bytes = (at * 4 + 15) & ~(size_t)15;
  return L;
}

__global__ void __launch_bounds__(64)
    franka_follow_cloud_kernel(const float *__restrict__ q_start, const float *__restrict__ poses, int W, int T, float finger,
                               const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,
                               const int32_t *__restrict__ sl, int S, const float *__restrict__ field, FieldGrid G,
                               float point_radius, const float *__restrict__ v_init,
                               const int32_t *__restrict__ progress_init, mpx_follow_options opt,
                               const int32_t *__restrict__ start_flags, float *__restrict__ path, float *__restrict__ arc,
                               int32_t *__restrict__ steps_out, float *__restrict__ q_end, float *__restrict__ v_end,
                               int32_t *__restrict__ progress_end, float *__restrict__ waypoints,
                               float *__restrict__ refined, int32_t *__restrict__ pre_bits, int32_t *__restrict__ bad_out) {
  __shared__ float buf[64 * 7];  // the T waypoints under judgement
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  float *P = path + (size_t)b * ((size_t)opt.max_steps + 1) * 7;
  float *A = arc + (size_t)b * ((size_t)opt.max_steps + 1);
  const float *my_poses = poses + (size_t)b * W * 16;
  const int R = (T - 1) * opt.substeps + 1;
  float *ref = refined + (size_t)b * (size_t)R * 7;

  // ---- the state as given, and what makes it bad input --------------------------------------------------------------------
#include "follow_state.inc"

  const bool test_env = field != nullptr && S > 0, test_self = opt.check_self != 0;
  if (!bad && !progress_init) {  // (wave-uniform) the start of a FRESH rollout: the entry's flags call on q_start, the self test
    bad = start_flags[b] != 0;
    if (!bad && test_self) bad = plan_self_bits(q, finger, opt.check_margin) != 0;
  }

  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 7; ++j) P[j] = q[j];
    A[0] = 0.0f;
  }
  if (bad) {  // (wave-uniform) status 2: no steps, the state as given
    // (the flags call over `refined` reads every row: a bad row's are zeros, and the finish kernel discards its flag)
    for (int i = lane; i < R * 7; i += 64) ref[i] = 0.0f;
    if (lane == 0) {
      bad_out[b] = 1, pre_bits[b] = FOLLOW_BAD_BITS, steps_out[b] = 0;
      follow_store_state(b, q, v, w, nw, fin, q_end, v_end, progress_end);
    }
    return;
  }

  // ---- this lane's collision sphere ----------------------------------------------------------------------------------------
  const bool my_sphere = test_env && lane < S;
  const int link = my_sphere ? sl[lane] : -1;
  const float cx = my_sphere ? sc[3 * lane + 0] : 0.0f, cy = my_sphere ? sc[3 * lane + 1] : 0.0f,
              cz = my_sphere ? sc[3 * lane + 2] : 0.0f, radius = my_sphere ? sr[lane] : 0.0f;
  const int nj = link < 7 ? link : 7;  // the joints upstream of the sphere's link (link0 does not move: none)
  const float *f = test_env ? field + (size_t)b * ((size_t)G.nx * G.ny * G.nz) : nullptr;

  // ---- the time loop: at most opt.max_steps steps ---------------------------------------------------------------------------
  const float lam2 = opt.lambda * opt.lambda, inv_eps = 1.0f / opt.epsilon;
  float Rt[9], pt[3], total = 0.0f;
  follow_load_pose(my_poses + 16 * w, Rt, pt);
  int n = 0;
  for (int i = 1; i <= opt.max_steps; ++i) {
    if (fin) break;
    // 1. FK, 2. switch, 3. stop (leaves the loop), 4. the attractor u
#include "follow_step_head.inc"
    // 5. the obstacle gradient: lane = sphere reads the field, then the seven sums over lanes in a fixed order
    float g[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (test_env) {
      if (link >= 1) {
        float D, nx, ny, nz;
        field_sample<true>(f, G, sx, sy, sz, D, nx, ny, nz);
        const float d = ((D - point_radius) - radius) - opt.clearance;
        if (D < G.trunc && d < opt.epsilon) {  // (D >= trunc: saturated, or outside the grid)
          const float cp = d < 0.0f ? -1.0f : (d - opt.epsilon) * inv_eps;
          nx *= cp, ny *= cp, nz *= cp;
          float term[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
          plan_joint_terms<7>(o, z, sx, sy, sz, nx, ny, nz, term);
#pragma unroll
          for (int j = 0; j < 7; ++j) g[j] = j < nj ? term[j] : 0.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) g[j] += __shfl_xor(g[j], off);
    }
    // 6. the acceleration, 7. the integration and the clamp, the arc length, the dense path
#include "follow_step_tail.inc"
  }
  __threadfence_block();
  __syncthreads();  // (lane 0's path and arc are read by every lane below)

  // ---- retiming: lane = output waypoint -------------------------------------------------------------------------------------
#include "follow_retime.inc"

  // ---- the jerk, self and miss bits; the refined configurations go to scratch for the entry's flags call -------------------
#pragma unroll
  for (int j = 0; j < 7; ++j) buf[lane * 7 + j] = qt[j];
  __syncthreads();
  int bits = plan_jerk_bits(buf, lane, T, opt.max_jerk);
  for (int r0_ = 0; r0_ < R; r0_ += 64) {
    const int r = r0_ + lane;
    if (r < R) {
      float qq[7];
      plan_refined(buf, r, opt.substeps, qq);
#pragma unroll
      for (int j = 0; j < 7; ++j) ref[(size_t)r * 7 + j] = qq[j];
      if (test_self) bits |= plan_self_bits(qq, finger, opt.check_margin);
    }
  }
#include "follow_miss.inc"
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off);

  // ---- results ----------------------------------------------------------------------------------------------------------------
  if (lane < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) waypoints[((size_t)b * T + lane) * 7 + j] = qt[j];
  }
  if (lane == 0) {
    bad_out[b] = 0, pre_bits[b] = bits, steps_out[b] = n;
    follow_store_state(b, q, v, w, nw, fin, q_end, v_end, progress_end);
  }
}

// status, bits, traj and the optional traj_any of problem b from the rollout kernel's bits and the flags call's flag
__global__ void __launch_bounds__(64)
    franka_follow_cloud_finish_kernel(int T, const float *__restrict__ waypoints, const int32_t *__restrict__ pre_bits,
                                      const int32_t *__restrict__ traj_flags, const int32_t *__restrict__ bad,
                                      int32_t *__restrict__ status, int32_t *__restrict__ bits_out, float *__restrict__ traj,
                                      float *__restrict__ traj_any) {
  const int b = blockIdx.x, lane = (int)threadIdx.x;
  const bool is_bad = bad[b] != 0;  // (block-uniform)
  const int bits = is_bad ? FOLLOW_BAD_BITS : pre_bits[b] | (traj_flags[b] != 0 ? PLAN_BIT_ENV : 0);
  const float nan = __builtin_nanf("");
  const float *src = waypoints + (size_t)b * T * 7;  // (a bad row's waypoints are not written, and not read)
  for (int i = lane; i < T * 7; i += 64) {
    const float x = is_bad ? nan : src[i];
    traj[(size_t)b * T * 7 + i] = bits ? nan : x;
    if (traj_any) traj_any[(size_t)b * T * 7 + i] = x;
  }
  if (lane == 0) status[b] = is_bad ? 2 : bits ? 1 : 0, bits_out[b] = bits;
}

MPX_EXPORT int64_t mpx_franka_follow_cloud_scratch(int B, int T, int substeps) {
  if (B < 0 || !franka_plan_T_ok(T) || !franka_plan_substeps_ok(substeps)) return -1;
  return (int64_t)follow_cloud_layout(B, T, substeps).total_bytes;
}

MPX_EXPORT int mpx_franka_follow_cloud(const float *q_start, const float *poses, int B, int W, int T, float finger,
                                       const float *limits, const float *sph_centers, const float *sph_radii,
                                       const int32_t *sph_link, int S, const float *field, const mpx_field_grid *grid,
                                       const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                                       const int32_t *counts, float point_radius, const float *v_init,
                                       const int32_t *progress_init, const mpx_follow_options *options, float *path,
                                       float *arc, int32_t *status, int32_t *bits, int32_t *steps, float *traj,
                                       float *traj_any, float *q_end, float *v_end, int32_t *progress_end, void *scratch,
                                       int64_t scratch_bytes, mpx_stream_t stream) {
  const char *who = "mpx_franka_follow_cloud";
  const mpx_follow_options opt = options ? *options : franka_follow_defaults();
  if (franka_follow_options_check(who, W, T, opt) || franka_counts_check(who, S) ||
      franka_cloud_operand_check(who, B, S, N, point_radius, opt.clearance, cloud_point_stride, cloud && N > 0))
    return 1;  // (a short stride is tolerated when no point is read)
  FieldGrid G = {};
  if (field && field_grid_check(who, grid, G)) return 1;
  const int R = (T - 1) * opt.substeps + 1;
  if (franka_rows_check(who, B, opt.max_steps + 1, "B * (max_steps + 1)") ||
      franka_rows_check(who, B, R, "B x refined configurations"))
    return 1;
  const FollowCloudScratch L = follow_cloud_layout(B, T, opt.substeps);
  if (franka_scratch_size_check(who, scratch_bytes, (int64_t)L.total_bytes, {B, T, opt.substeps})) return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(path && arc && status && bits && steps && traj, "%s: NULL output (path, arc, status, bits, steps, traj)", who);
  MPX_REQUIRE(q_start && poses && limits, "%s: NULL operand (q_start, poses, limits)", who);
  if (franka_scratch_pointer_check(who, scratch) || franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  MPX_REQUIRE((!field && (!cloud || N == 0)) || S > 0, "%s: a field or a cloud without collision spheres to test them with", who);
  float *w = static_cast<float *>(scratch);
  int32_t *wi = static_cast<int32_t *>(scratch);
  hipStream_t st = mpx_s(stream);
  hipError_t e = hipMemsetAsync(wi + L.start_flags, 0, sizeof(int32_t) * 2 * (size_t)B, st);
  MPX_REQUIRE(e == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(e));
  const bool test_cloud = cloud && N > 0 && S > 0;
  const float reach = opt.clearance + opt.check_margin;  // (float32, as the contract says)
  if (test_cloud && !progress_init &&
      mpx_franka_cloud_collision(q_start, B, 1, finger, sph_centers, sph_radii, sph_link, S, cloud, cloud_batch_stride,
                                 cloud_point_stride, N, counts, point_radius, reach, wi + L.start_flags, nullptr, nullptr, stream))
    return 1;
  hipLaunchKernelGGL(franka_follow_cloud_kernel, dim3((unsigned)B), dim3(64), 0, st, q_start, poses, W, T, finger, limits,
                     sph_centers, sph_radii, sph_link, S, field, G, point_radius, v_init, progress_init, opt,
                     wi + L.start_flags, path, arc, steps, q_end, v_end, progress_end, w + L.waypoints, w + L.refined,
                     wi + L.pre_bits, wi + L.bad);
  e = hipGetLastError();
  MPX_REQUIRE(e == hipSuccess, "%s: launch failed: %s", who, hipGetErrorString(e));
  if (test_cloud && mpx_franka_cloud_collision(w + L.refined, B, R, finger, sph_centers, sph_radii, sph_link, S, cloud,
                                               cloud_batch_stride, cloud_point_stride, N, counts, point_radius, reach,
                                               wi + L.traj_flags, nullptr, nullptr, stream))
    return 1;
  hipLaunchKernelGGL(franka_follow_cloud_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, T, w + L.waypoints, wi + L.pre_bits,
                     wi + L.traj_flags, wi + L.bad, status, bits, traj, traj_any);
  MPX_LAUNCH_CHECK(who);
}
