// ik.hip -- batched collision-free inverse kinematics of the Franka Panda.
//
// Replaces (reference call sites; the implementation is robofin's ikfast wrapper + a PyBullet test per draw):
//   FrankaRealRobot.collision_free_ik(sim, arm, selfcc, pose, retries=1000)
//                                data_pipeline/environments/tabletop_environment.py:395,
//                                cubby_environment.py:546, dresser_environment.py:496
//   FrankaRobot.ik / FrankaRealRobot.ik (robofin)
//
// Damped least squares with restarts.  One wave per problem, one lane per restart ("seed"), everything a lane iterates on
// in registers, one instruction stream: the iteration count is an argument and there is no early exit, so the 64 lanes
// never diverge.  Per iteration: FK (franka_fk_visit, keeping the seven joint origins, their z axes and right_gripper),
// e = [p_t - p ; rotvec(R_t R^T)], the geometric Jacobian J[:, j] = [z_j x (p - o_j) ; z_j],
// dq = J^T (J J^T + lambda^2 I)^-1 e through an unrolled 6x6 Cholesky (positive definite for lambda > 0: no pivoting),
// the step scaled so that max |dq_j| <= step_clip (dls_direction.inc states these), q clamped into the limits.
// A lane is ACCEPTED when one more FK of its final q -- the code mpx_franka_fk runs -- is within pos_tol / rot_tol of the
// target.  Accepted lanes are then visited in lane order and the WAVE tests one candidate together: lane = collision
// sphere against the problem's live primitives (compacted into LDS once, sdf_device.h forms, `sdf <= radius + clearance`
// is a hit: with clearance 0 exactly mpx_franka_collision's test), then the self model of franka_device.h, the one
// mpx_trajectory_metrics applies.  The first candidate without a hit is the result: "the lowest seed that
// converges and is free".
//
// Against a point cloud (mpx_franka_ik_cloud, at the end of this file): the same kernel without primitives, every start's
// q and bits kept; the per-waypoint cloud check of cloud_collision.hip on the [B,64,7] starts with `active` = converged
// (a self-hit start is tested too: with all_status every converged start carries both bits); then a select kernel, one wave per problem, that folds the verdicts into bit 1 and picks the lowest start
// whose bits equal 1.
#include "common.h"
#include "franka_host.h"
#include "franka_device.h"
#include "dls_device.h"  // what the solver shares with follow.hip: the rotation vector (and dls_direction.inc)
#include "sdf_device.h"
#include "philox.h"

enum { STREAM_IK = 13 };
constexpr int IK_FRAME_FLOATS = MPX_NUM_FRAMES * 12;

__global__ void __launch_bounds__(64)
    franka_ik_kernel(const float *__restrict__ targets, float finger, const float *__restrict__ limits,
                     const float *__restrict__ q_init, const float *__restrict__ sc, const float *__restrict__ sr,
                     const int32_t *__restrict__ sl, int S, const float *__restrict__ cub_f,
                     const float *__restrict__ cub_d, int M1, const float *__restrict__ cyl_f,
                     const float *__restrict__ cyl_r, const float *__restrict__ cyl_h, int M2, mpx_ik_options opt,
                     uint32_t seed_lo, uint32_t seed_hi, uint32_t env0, float *__restrict__ q_out,
                     int32_t *__restrict__ status, float *__restrict__ all_q, int32_t *__restrict__ all_status) {
  __shared__ __attribute__((aligned(16))) float prim_rows[128 * 16];  // live cuboids from row 0, live cylinders from row 64
  __shared__ float frames[IK_FRAME_FLOATS];                           // the candidate under test
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  const float *tg = targets + (size_t)b * 16;  // (wave-uniform: scalar loads)
  const float Rt[9] = {tg[0], tg[1], tg[2], tg[4], tg[5], tg[6], tg[8], tg[9], tg[10]};
  const float pt[3] = {tg[3], tg[7], tg[11]};
  float lo[7], hi[7], q[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) lo[j] = limits[2 * j], hi[j] = limits[2 * j + 1];

  // ---- starts: lane 0 from the caller (or the neutral pose), the others uniform in the limits -----------------------------
  {
    const float neutral[7] = {0.00f, -1.3f, 0.00f, -2.87f, 0.00f, 2.00f, 0.75f};  // franka_tables.DEFAULT_Q
    const Philox r0 = philox4x32(2u * (uint32_t)lane, env0 + (uint32_t)b, STREAM_IK, 0u, seed_lo, seed_hi);
    const Philox r1 = philox4x32(2u * (uint32_t)lane + 1u, env0 + (uint32_t)b, STREAM_IK, 0u, seed_lo, seed_hi);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float u = u01(j < 4 ? r0.c[j] : r1.c[j - 4]);
      const float drawn = lo[j] + u * (hi[j] - lo[j]);
      const float given = q_init ? q_init[(size_t)b * 7 + j] : neutral[j];
      q[j] = fminf(fmaxf(lane == 0 ? given : drawn, lo[j]), hi[j]);
    }
  }

  // ---- damped least squares ----------------------------------------------------------------------------------------------
  const float lam2 = opt.lambda * opt.lambda;
  for (int it = 0; it < opt.iterations; ++it) {
    float o[7][3], z[7][3];
    Rigid eff;
    franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
      constexpr int id = decltype(ID)::value;
      if constexpr (id >= 1 && id <= 7) {
        o[id - 1][0] = g.t[0], o[id - 1][1] = g.t[1], o[id - 1][2] = g.t[2];
        z[id - 1][0] = g.r[2], z[id - 1][1] = g.r[5], z[id - 1][2] = g.r[8];
      }
      if constexpr (id == 14) eff = g;
    });
#define DLS_STEP_CLIP opt.step_clip
#include "dls_direction.inc"
#undef DLS_STEP_CLIP
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = fminf(fmaxf(q[j] + dq[j] * scale, lo[j]), hi[j]);
  }

  // ---- acceptance: one more FK of the final q (the chain mpx_franka_fk evaluates) ------------------------------------------
  bool conv;
  {
    Rigid eff;
    franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
      if constexpr (decltype(ID)::value == 14) eff = g;
    });
    const float dx = pt[0] - eff.t[0], dy = pt[1] - eff.t[1], dz = pt[2] - eff.t[2];
    const float perr = sqrtf(mpx_fma(dz, dz, mpx_fma(dy, dy, dx * dx)));
    float w[3];
    const float theta = ik_rotvec(Rt, eff.r, w);
    // (the margins -- 1e-4 relative, 2e-6 rad: tens of times the float32 rounding of perr and theta -- make the
    // acceptance hold for a caller who re-checks the SAME frame in other arithmetic, e.g. float64)
    conv = perr <= opt.pos_tol * MPX_IK_ACCEPT_SHARE && theta <= opt.rot_tol * MPX_IK_ACCEPT_SHARE - MPX_IK_ACCEPT_ANGLE_MARGIN;
  }

  // ---- the problem's live primitives, compacted into LDS (every lane of the one wave stores) -------------------------------
#define FRANKA_LIVE_ROWS_STORE true
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  __syncthreads();

  // ---- candidates in lane order: the wave tests one at a time, lane = collision sphere ----------------------------------------
  const unsigned long long accepted = __builtin_amdgcn_ballot_w64(conv);
  const bool test_env = S > 0 && n_cub + n_cyl > 0, test_self = opt.check_self != 0;
  const bool test_all = all_status != nullptr;  // every seed's bits are wanted: no stop at the first free one
  int winner = -1;
  bool my_env = false, my_self = false;
  if (!test_env && !test_self) {
    winner = accepted ? (int)__builtin_ctzll(accepted) : -1;
  } else {
    unsigned long long todo = accepted;
    while (todo) {
      const int c = (int)__builtin_ctzll(todo);  // (wave-uniform)
      todo &= todo - 1;
      if (lane == c) franka_fk_frames(q, finger, frames);
      __syncthreads();
      bool hit = false;
      if (test_env && lane < S) {
        float x, y, zz;
        rigid_apply(frames + 12 * sl[lane], sc[3 * lane + 0], sc[3 * lane + 1], sc[3 * lane + 2], x, y, zz);
        float best = __builtin_inff();
        for (int m = 0; m < n_cub; ++m) {
          const float *row = prim_rows + 16 * m;
          best = fminf(best, cuboid_sdf_live(row, row[12], row[13], row[14], x, y, zz));
        }
        for (int m = 0; m < n_cyl; ++m) {
          const float *row = prim_rows + 16 * (64 + m);
          best = fminf(best, cylinder_sdf_live(row, row[12], row[13], x, y, zz));
        }
        hit = best <= sr[lane] + opt.clearance;
      }
      bool self = false;
      if (test_self && lane < FRANKA_SELF_SPHERES) {  // lane = sphere of the self model
        static_assert(FRANKA_SELF_SPHERES == 4, "the two selects below");
        const int link = lane == 0   ? FRANKA_SELF_FRAME[0]
                         : lane == 1 ? FRANKA_SELF_FRAME[1]
                         : lane == 2 ? FRANKA_SELF_FRAME[2]
                                     : FRANKA_SELF_FRAME[3];
        const float radius = lane == 0   ? FRANKA_SELF_RADIUS[0]
                             : lane == 1 ? FRANKA_SELF_RADIUS[1]
                             : lane == 2 ? FRANKA_SELF_RADIUS[2]
                                         : FRANKA_SELF_RADIUS[3];
        const float *p = frames + 12 * link + 9;
        self = franka_self_hit(p[0], p[1], p[2], radius);
      }
      const bool any_env = __any(hit), any_self = __any(self);
      if (lane == c) my_env = any_env, my_self = any_self;
      __syncthreads();  // (the next candidate overwrites `frames`)
      if (!any_env && !any_self && winner < 0) {
        winner = c;
        if (!test_all) break;
      }
    }
  }

  // ---- results ----------------------------------------------------------------------------------------------------------------
  if (all_q) {
#pragma unroll
    for (int j = 0; j < 7; ++j) all_q[((size_t)b * 64 + lane) * 7 + j] = q[j];
  }
  if (all_status) all_status[(size_t)b * 64 + lane] = (conv ? 1 : 0) | (my_env ? 2 : 0) | (my_self ? 4 : 0);
  if (winner >= 0) {
    if (lane == winner) {
#pragma unroll
      for (int j = 0; j < 7; ++j) q_out[(size_t)b * 7 + j] = q[j];
    }
  } else if (lane < 7) {
    q_out[(size_t)b * 7 + lane] = __builtin_nanf("");
  }
  if (lane == 0) status[b] = winner >= 0 ? 0 : accepted ? 1 : 2;
}

MPX_EXPORT int mpx_franka_ik(const float *target_poses, int B, float finger, const float *limits, const float *q_init,
                             const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                             const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                             const float *cyl_radii, const float *cyl_heights, int M2, const mpx_ik_options *options,
                             uint64_t seed, int64_t env_offset, float *q_out, int32_t *status, float *all_q,
                             int32_t *all_status, mpx_stream_t stream) {
  const char *who = "mpx_franka_ik";
  const mpx_ik_options opt = options ? *options : franka_ik_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (franka_counts_check(who, S, M1, M2) || franka_ik_options_check(who, opt) || franka_env_offset_check(who, env_offset, B))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(q_out && status, "%s: NULL output (q_out, status)", who);
  MPX_REQUIRE(target_poses && limits, "%s: NULL operand (target_poses, limits)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  hipLaunchKernelGGL(franka_ik_kernel, dim3((unsigned)B), dim3(64), 0, mpx_s(stream), target_poses, finger, limits, q_init,
                     sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii,
                     cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, q_out, status,
                     all_q, all_status);
  MPX_LAUNCH_CHECK(who);
}

// ---- against a point cloud ------------------------------------------------------------------------------------------------------
// scratch: all_q [B,64,7] float, all_status [B,64], active [B,64], hit [B,64] int32 (the first two unused when the caller
// passes its own)
constexpr int64_t IK_CLOUD_WORDS_PER_PROBLEM = MPX_IK_SEEDS * (7 + 3);

__global__ void __launch_bounds__(256)
    franka_ik_cloud_active_kernel(const int32_t *__restrict__ all_status, int64_t n, int32_t *__restrict__ active) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) active[i] = all_status[i] & 1;  // converged: the starts that carry a cloud verdict
}

// one wave per problem, lane = start: bit 1 from the cloud verdicts, the lowest start with bits == 1, NaN row otherwise
__global__ void __launch_bounds__(256)
    franka_ik_cloud_select_kernel(int B, const float *__restrict__ all_q, const int32_t *__restrict__ bits_in,
                                  const int32_t *__restrict__ hit, float *__restrict__ q_out, int32_t *__restrict__ status,
                                  int32_t *__restrict__ all_status) {
  const int b = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (b >= B) return;  // (wave-uniform)
  const size_t i = (size_t)b * 64 + lane;
  int bits = bits_in[i];
  if (hit && (bits & 1) && hit[i] != 0) bits |= 2;
  if (all_status) all_status[i] = bits;
  const unsigned long long free = __builtin_amdgcn_ballot_w64(bits == 1), conv = __builtin_amdgcn_ballot_w64((bits & 1) != 0);
  const int winner = free ? (int)__builtin_ctzll(free) : -1;
  if (lane < 7) q_out[(size_t)b * 7 + lane] = winner >= 0 ? all_q[((size_t)b * 64 + winner) * 7 + lane] : __builtin_nanf("");
  if (lane == 0) status[b] = winner >= 0 ? 0 : conv ? 1 : 2;
}

MPX_EXPORT int64_t mpx_franka_ik_cloud_scratch(int B) {
  if (B < 0) return -1;
  return (int64_t)B * IK_CLOUD_WORDS_PER_PROBLEM * 4;  // (2560 B: a multiple of 16)
}

MPX_EXPORT int mpx_franka_ik_cloud(const float *target_poses, int B, float finger, const float *limits, const float *q_init,
                                   const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                   const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                                   const int32_t *counts, float point_radius, const mpx_ik_options *options, uint64_t seed,
                                   int64_t env_offset, float *q_out, int32_t *status, float *all_q, int32_t *all_status,
                                   void *scratch, int64_t scratch_bytes, mpx_stream_t stream) {
  const char *who = "mpx_franka_ik_cloud";
  const float clearance = options ? options->clearance : franka_ik_defaults().clearance;
  // what the cloud check would refuse, before anything is launched (the 64 starts are its waypoints)
  if (franka_cloud_operand_check(who, B, S, N, point_radius, clearance, cloud_point_stride) ||
      franka_rows_check(who, B, MPX_IK_SEEDS, "B * 64"))
    return 1;
  const bool test_env = cloud != nullptr && N > 0;
  MPX_REQUIRE(N == 0 || S > 0, "%s: a cloud without collision spheres to test it with", who);
  if (franka_counts_check(who, S) || franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_scratch_size_check(who, scratch_bytes, mpx_franka_ik_cloud_scratch(B), {B}) ||
      (B > 0 && franka_scratch_pointer_check(who, scratch)))
    return 1;
  float *w_q = all_q ? all_q : static_cast<float *>(scratch);
  int32_t *wi = static_cast<int32_t *>(scratch) + (size_t)B * MPX_IK_SEEDS * 7;
  int32_t *w_bits = wi, *w_active = wi + (size_t)B * MPX_IK_SEEDS, *w_hit = wi + (size_t)2 * B * MPX_IK_SEEDS;
  // the solver, no primitives: every start's q, bit 0 and (check_self) bit 2.  (Its q_out / status are written again below.)
  if (mpx_franka_ik(target_poses, B, finger, limits, q_init, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr,
                    nullptr, nullptr, 0, options, seed, env_offset, q_out, status, w_q, w_bits, stream))
    return 1;
  if (B == 0) return 0;
  const int64_t n = (int64_t)B * MPX_IK_SEEDS;
  hipStream_t st = mpx_s(stream);
  if (test_env) {
    hipLaunchKernelGGL(franka_ik_cloud_active_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, w_bits, n, w_active);
    hipError_t e = hipGetLastError();
    MPX_REQUIRE(e == hipSuccess, "%s: launch failed: %s", who, hipGetErrorString(e));
    if (mpx_franka_cloud_collision_each(w_q, B, MPX_IK_SEEDS, finger, sph_centers, sph_radii, sph_link, S, cloud,
                                        cloud_batch_stride, cloud_point_stride, N, counts, point_radius, clearance, w_active,
                                        w_hit, stream))
      return 1;
  }
  hipLaunchKernelGGL(franka_ik_cloud_select_kernel, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, st, B, w_q, w_bits,
                     test_env ? w_hit : nullptr, q_out, status, all_status);
  MPX_LAUNCH_CHECK(who);
}
