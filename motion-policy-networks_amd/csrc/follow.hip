// follow.hip -- a reactive follower of an end-effector path for the Franka Panda, the retiming of its dense path to T
// waypoints of constant arc-length spacing, and the verdict on them.
//
// Stands where the reference's data generator runs Geometric Fabrics along the global plan, downsamples and filters with
// verify_trajectory (data_pipeline/gen_data.py:156-307, 433-528: the 'hybrid_solutions' key).  It is NOT Lula's fabric and
// claims no parity with it: a damped second-order joint-space system, a = attract u - repel g + barrier - damping v, with
// u the IK kernel's damped-least-squares direction toward the current guide pose (dls_direction.inc) and g the planner's
// obstacle gradient for one configuration.  The contract (one step, the dense path, retiming, the verdict, continuing a
// rollout from the returned state) is stated in include/mpinets_hip.h.
//
// One wave per problem.  The state (q, v, waypoint, steps on it), the seven joint origins and axes and the 6x6 solve are
// wave-uniform: every lane evaluates them from the same numbers.  In the obstacle term the lane is the collision sphere
// (S <= 64), as in the IK kernel's candidate test: its centre comes from the frame of its link as franka_fk_visit hands it
// over, the live primitives sit in LDS (franka_live_rows.inc), and the seven sums over spheres are a butterfly of
// __shfl_xor in a fixed order, so every lane ends with the same bits whatever the timing.  The time loop runs at most
// opt.max_steps (host-checked) iterations; the dense path and its arc lengths go to the caller's global buffers (28 bytes
// a step: LDS is better spent on occupancy in a latency-bound loop).  Retiming: lane = output waypoint, a bisection of
// fixed length over arc[].  Verdict: plan_jerk_bits, plan_refined and plan_config_bits with lane = refined configuration.
//
// Everything but the obstacle term, the test of a fresh start, the bad-input return and the verdict is stated once for
// this kernel and follow_cloud.hip's: follow_device.h and the statement blocks follow_state.inc, follow_step_head.inc,
// follow_step_tail.inc, follow_retime.inc and follow_miss.inc (profiles/follow_shared_isa.md: the instruction streams did
// not move).
#include "common.h"
#include "franka_host.h"
#include "franka_device.h"
#include "dls_device.h"         // what the follower shares with ik.hip: the rotation vector (and dls_direction.inc)
#include "sdf_grad_device.h"
#include "plan_device.h"        // ... with plan.hip: the joint terms of a sphere's gradient, the jerk test, the refined sweep
#include "plan_prims_device.h"  // ... and the validity test of one configuration
#include "follow_device.h"      // ... with follow_cloud.hip: all but the obstacle term and the verdict

__global__ void __launch_bounds__(64)
    franka_follow_kernel(const float *__restrict__ q_start, const float *__restrict__ poses, int W, int T, float finger,
                         const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,
                         const int32_t *__restrict__ sl, int S, const float *__restrict__ cub_f,
                         const float *__restrict__ cub_d, int M1, const float *__restrict__ cyl_f,
                         const float *__restrict__ cyl_r, const float *__restrict__ cyl_h, int M2,
                         const float *__restrict__ v_init, const int32_t *__restrict__ progress_init, mpx_follow_options opt,
                         float *__restrict__ path, float *__restrict__ arc, int32_t *__restrict__ status,
                         int32_t *__restrict__ bits_out, int32_t *__restrict__ steps_out, float *__restrict__ traj,
                         float *__restrict__ traj_any, float *__restrict__ q_end, float *__restrict__ v_end,
                         int32_t *__restrict__ progress_end) {
  __shared__ __attribute__((aligned(16))) float prim_rows[128 * 16];  // live cuboids from row 0, live cylinders from row 64
  __shared__ float buf[64 * 7];                                       // the T waypoints under judgement
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  float *P = path + (size_t)b * ((size_t)opt.max_steps + 1) * 7;
  float *A = arc + (size_t)b * ((size_t)opt.max_steps + 1);
  const float *my_poses = poses + (size_t)b * W * 16;

  // ---- the state as given, and what makes it bad input --------------------------------------------------------------------
#include "follow_state.inc"

  // ---- the problem's live primitives, compacted into LDS (every lane of the one wave stores) -------------------------------
#define FRANKA_LIVE_ROWS_STORE true
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  __syncthreads();

  const bool test_env = S > 0 && n_cub + n_cyl > 0, test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;
  if (!bad && !progress_init)  // (wave-uniform) the start of a FRESH rollout must pass the planner's configuration test
    bad = plan_config_bits(q, finger, sc, sr, sl, S, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin) != 0;

  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 7; ++j) P[j] = q[j];
    A[0] = 0.0f;
  }
  if (bad) {  // (wave-uniform) status 2: no steps, the state as given
    const float nan = __builtin_nanf("");
    for (int i = lane; i < T * 7; i += 64) {
      traj[(size_t)b * T * 7 + i] = nan;
      if (traj_any) traj_any[(size_t)b * T * 7 + i] = nan;
    }
    if (lane == 0) {
      status[b] = 2, bits_out[b] = FOLLOW_BAD_BITS, steps_out[b] = 0;
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

  // ---- the time loop: at most opt.max_steps steps ---------------------------------------------------------------------------
  const float lam2 = opt.lambda * opt.lambda, inv_eps = 1.0f / opt.epsilon;
  float Rt[9], pt[3], total = 0.0f;
  follow_load_pose(my_poses + 16 * w, Rt, pt);
  int n = 0;
  for (int i = 1; i <= opt.max_steps; ++i) {
    if (fin) break;
    // 1. FK, 2. switch, 3. stop (leaves the loop), 4. the attractor u
#include "follow_step_head.inc"
    // 5. the obstacle gradient: lane = sphere, then the seven sums over lanes in a fixed order
    float g[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (test_env) {
      if (link >= 1) {
        int arg;
        const float best = plan_min_sdf(prim_rows, n_cub, n_cyl, sx, sy, sz, arg);
        const float d = (best - radius) - opt.clearance;
        if (d < opt.epsilon) {  // (d = +inf without a live primitive)
          const float cp = d < 0.0f ? -1.0f : (d - opt.epsilon) * inv_eps;
          const float *row = prim_rows + 16 * arg;
          float px, py, pz, l0, l1, l2, nx, ny, nz;
          mpx_project(row, sx, sy, sz, px, py, pz);
          if (arg < 64)
            cuboid_sdf_grad_local(px, py, pz, row[12], row[13], row[14], l0, l1, l2);
          else
            cylinder_sdf_grad_local(px, py, pz, row[12], row[13], l0, l1, l2);
          sdf_grad_to_world(row, l0, l1, l2, nx, ny, nz);
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

  // ---- the verdict: the planner's tests on the T waypoints, and the miss of the last guide pose ----------------------------
#pragma unroll
  for (int j = 0; j < 7; ++j) buf[lane * 7 + j] = qt[j];
  __syncthreads();
  int bits = plan_jerk_bits(buf, lane, T, opt.max_jerk);
  if (test_env || test_self) {
    const int R = (T - 1) * opt.substeps + 1;
    for (int r0_ = 0; r0_ < R; r0_ += 64) {
      const int r = r0_ + lane;
      if (r < R) {
        float qq[7];
        plan_refined(buf, r, opt.substeps, qq);
        bits |= plan_config_bits(qq, finger, sc, sr, sl, S, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin);
      }
    }
  }
#include "follow_miss.inc"
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off);

  // ---- results ----------------------------------------------------------------------------------------------------------------
  if (lane < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      traj[((size_t)b * T + lane) * 7 + j] = bits ? __builtin_nanf("") : qt[j];
      if (traj_any) traj_any[((size_t)b * T + lane) * 7 + j] = qt[j];
    }
  }
  if (lane == 0) {
    status[b] = bits ? 1 : 0, bits_out[b] = bits, steps_out[b] = n;
    follow_store_state(b, q, v, w, nw, fin, q_end, v_end, progress_end);
  }
}

MPX_EXPORT int mpx_franka_follow(const float *q_start, const float *poses, int B, int W, int T, float finger,
                                 const float *limits, const float *sph_centers, const float *sph_radii,
                                 const int32_t *sph_link, int S, const float *cub_inv_frames, const float *cub_dims, int M1,
                                 const float *cyl_inv_frames, const float *cyl_radii, const float *cyl_heights, int M2,
                                 const float *v_init, const int32_t *progress_init, const mpx_follow_options *options,
                                 float *path, float *arc, int32_t *status, int32_t *bits, int32_t *steps, float *traj,
                                 float *traj_any, float *q_end, float *v_end, int32_t *progress_end, mpx_stream_t stream) {
  const char *who = "mpx_franka_follow";
  const mpx_follow_options opt = options ? *options : franka_follow_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (franka_follow_options_check(who, W, T, opt) || franka_counts_check(who, S, M1, M2) ||
      franka_rows_check(who, B, opt.max_steps + 1, "B * (max_steps + 1)"))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(path && arc && status && bits && steps && traj, "%s: NULL output (path, arc, status, bits, steps, traj)", who);
  MPX_REQUIRE(q_start && poses && limits, "%s: NULL operand (q_start, poses, limits)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  hipLaunchKernelGGL(franka_follow_kernel, dim3((unsigned)B), dim3(64), 0, mpx_s(stream), q_start, poses, W, T, finger, limits,
                     sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights,
                     M2, v_init, progress_init, opt, path, arc, status, bits, steps, traj, traj_any, q_end, v_end,
                     progress_end);
  MPX_LAUNCH_CHECK(who);
}
