// plan.hip -- batched collision-free trajectory planning of the Franka Panda between two configurations.
//
// Stands where the reference's data generator calls OMPL's AIT* and Geometric Fabrics and then filters with
// verify_trajectory (data_pipeline/gen_data.py:106-153, 396-430).  It is NOT that planner: it is a local optimiser,
// covariant gradient descent (CHOMP form) from K starting trajectories, and "valid" means valid by this library's sphere
// model.  The contract (candidates, one iteration, validity, the choice) is stated in include/mpinets_hip.h.
//
// One workgroup per problem, one wave per candidate, lane = waypoint (T <= 64).  FK, the sphere loop and the gradient of
// a waypoint stay in the lane's registers: franka_fk_visit hands over each frame as it exists, the lane then walks the
// sphere table (wave-uniform: scalar loads) for the spheres of that link, tests them against the problem's live primitives
// (compacted into LDS once per workgroup: franka_live_rows.inc) and adds c'(d) n . (z_j x (x - o_j)) for the joints upstream.
// g goes to LDS once per iteration for the M g product (n x 7 FMAs per lane, M in LDS, broadcast reads of g).
// The validity sweep reuses the mapping with lane = refined configuration, in passes of 64.
#include "common.h"
#include "franka_host.h"
#include "sdf_grad_device.h"
#include "plan_device.h"  // what the planner shares with cloud_field.hip: endpoints, candidates, M g, the jerk test

// min over the live primitives (LDS rows [R | Rt (3 x 4 floats) | sizes]; cuboids from row 0, cylinders from row 64) and
// the row that attains it: the first minimum, cuboids before cylinders (-1: no live primitive)
__device__ __forceinline__ float plan_min_sdf(const float *prim_rows, int n_cub, int n_cyl, float x, float y, float z,
                                              int &arg) {
  float best = __builtin_inff();
  arg = -1;
  for (int m = 0; m < n_cub; ++m) {
    const float *row = prim_rows + 16 * m;
    const float v = cuboid_sdf_live(row, row[12], row[13], row[14], x, y, z);
    if (v < best) best = v, arg = m;
  }
  for (int m = 0; m < n_cyl; ++m) {
    const float *row = prim_rows + 16 * (64 + m);
    const float v = cylinder_sdf_live(row, row[12], row[13], x, y, z);
    if (v < best) best = v, arg = 64 + m;
  }
  return best;
}

// bits PLAN_BIT_ENV / PLAN_BIT_SELF of one configuration
__device__ __forceinline__ int plan_config_bits(const float *q, float finger, const float *__restrict__ sc,
                                                const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                                const float *prim_rows, int n_cub, int n_cyl, float reach, bool test_self,
                                                float self_margin) {
  int bits = 0;
  const bool test_env = S > 0 && n_cub + n_cyl > 0;
  franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
    constexpr int id = decltype(ID)::value;
    if (test_env) {
      for (int s = 0; s < S; ++s) {
        if (sl[s] != id) continue;  // (wave-uniform)
        float x, y, z;
        rigid_apply(g, sc[3 * s + 0], sc[3 * s + 1], sc[3 * s + 2], x, y, z);
        int arg;
        const float best = plan_min_sdf(prim_rows, n_cub, n_cyl, x, y, z, arg);
        if (best <= sr[s] + reach) bits |= PLAN_BIT_ENV;
      }
    }
    if constexpr (franka_self_sphere(id) >= 0) {
      if (test_self && franka_self_hit<id>(g, self_margin)) bits |= PLAN_BIT_SELF;
    }
  });
  return bits;
}

// MAXK: the most candidates a launch may carry.  Up to 8 waves per workgroup leave a wave 256 VGPRs (no spills); 16
// leave it 128, where the seven joint frames no longer fit and a few values go to scratch.
template <int MAXK>
__global__ void __launch_bounds__(64 * MAXK)
    franka_plan_kernel(const float *__restrict__ q_start, const float *__restrict__ q_goal, int T, float finger,
                       const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,
                       const int32_t *__restrict__ sl, int S, const float *__restrict__ cub_f,
                       const float *__restrict__ cub_d, int M1, const float *__restrict__ cyl_f,
                       const float *__restrict__ cyl_r, const float *__restrict__ cyl_h, int M2, mpx_plan_options opt,
                       uint32_t seed_lo, uint32_t seed_hi, uint32_t env0, float *__restrict__ traj,
                       int32_t *__restrict__ status, int32_t *__restrict__ choice, float *__restrict__ all_traj,
                       int32_t *__restrict__ all_status) {
  // LDS: [128 primitive rows x 16 | M: T x T | per candidate: 64 waypoints x 7 (g, then the trajectory) | K bits]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *prim_rows = lds;
  float *Mtab = lds + 128 * 16;
  const int K = opt.candidates;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // candidate of this wave
  float *buf = Mtab + T * T + k * 64 * 7;
  int *cand_bits = reinterpret_cast<int *>(Mtab + T * T + K * 64 * 7);
  const int n = T - 2;
  const int t = lane < T ? lane : T - 1;  // (lanes past the trajectory repeat the goal and never store)

  float lo[7], hi[7], qs[7], qg[7];
  bool bad_end = plan_endpoints(limits, q_start, q_goal, b, lo, hi, qs, qg);

  // ---- the problem's live primitives, compacted into LDS: wave 0 stores, every wave gets the counts ---------------------------
#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  plan_fill_metric(Mtab, T, n);
  __syncthreads();

  const bool test_env = S > 0 && n_cub + n_cyl > 0, test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;

  // ---- endpoints: an invalid one ends the problem (block-uniform: every wave computes the same answer) --------------------
  if (!bad_end) {  // (the limits test is wave-uniform)
    int e = 0;
    if (lane < 2)
      e = plan_config_bits(lane == 0 ? qs : qg, finger, sc, sr, sl, S, prim_rows, n_cub, n_cyl, reach, test_self,
                           opt.check_margin);
    bad_end = __any(e != 0);
  }
  if (bad_end) {
    const float nan = __builtin_nanf("");
    if (k == 0) {
      for (int i = lane; i < T * 7; i += 64) traj[(size_t)b * T * 7 + i] = nan;
      if (lane == 0) {
        status[b] = 2;
        if (choice) choice[b] = -1;
      }
    }
    if (all_traj)
      for (int i = lane; i < T * 7; i += 64) all_traj[((size_t)b * K + k) * T * 7 + i] = nan;
    if (all_status && lane == 0) all_status[(size_t)b * K + k] = PLAN_BIT_ENV | PLAN_BIT_SELF | PLAN_BIT_JERK;
    return;
  }

  // ---- this lane's waypoint of candidate k ---------------------------------------------------------------------------------
  float L[7], q[7];
  plan_candidate(k, t, T, env0 + (uint32_t)b, seed_lo, seed_hi, opt.spread, qs, qg, lo, hi, L, q);
  const bool interior = lane >= 1 && lane <= n;

  // ---- covariant gradient descent ------------------------------------------------------------------------------------------
  const float inv_eps = 1.0f / opt.epsilon;
  for (int it = 0; it < opt.iterations; ++it) {
    float g[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (test_env) {
      float o[7][3], z[7][3];
      franka_fk_visit(q, finger, [&](auto ID, const Rigid &fr) __attribute__((always_inline)) {
        constexpr int id = decltype(ID)::value;
        if constexpr (id >= 1 && id <= 7) {
          o[id - 1][0] = fr.t[0], o[id - 1][1] = fr.t[1], o[id - 1][2] = fr.t[2];
          z[id - 1][0] = fr.r[2], z[id - 1][1] = fr.r[5], z[id - 1][2] = fr.r[8];
        }
        if constexpr (id >= 1) {  // (link0 does not move)
          constexpr int nj = id < 7 ? id : 7;
          for (int s = 0; s < S; ++s) {
            if (sl[s] != id) continue;  // (wave-uniform)
            float x, y, zz;
            rigid_apply(fr, sc[3 * s + 0], sc[3 * s + 1], sc[3 * s + 2], x, y, zz);
            int arg;
            const float best = plan_min_sdf(prim_rows, n_cub, n_cyl, x, y, zz, arg);
            const float d = (best - sr[s]) - opt.clearance;
            if (d < opt.epsilon) {  // (d = +inf without a live primitive)
              const float cp = d < 0.0f ? -1.0f : (d - opt.epsilon) * inv_eps;
              const float *row = prim_rows + 16 * arg;
              float px, py, pz, l0, l1, l2, nx, ny, nz;
              mpx_project(row, x, y, zz, px, py, pz);
              if (arg < 64)
                cuboid_sdf_grad_local(px, py, pz, row[12], row[13], row[14], l0, l1, l2);
              else
                cylinder_sdf_grad_local(px, py, pz, row[12], row[13], l0, l1, l2);
              sdf_grad_to_world(row, l0, l1, l2, nx, ny, nz);
              nx *= cp, ny *= cp, nz *= cp;
              plan_joint_terms<nj>(o, z, x, y, zz, nx, ny, nz, g);
            }
          }
        }
      });
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) buf[lane * 7 + j] = g[j];
    // (buf belongs to this wave alone, so a wave-level barrier would do; the workgroup barrier is legal -- every wave runs
    // the same iteration count and the bad-endpoint return is block-uniform -- and couples the candidates' progress, at
    // two barriers per ~20 k instructions of an iteration.  The looser form is unmeasured.)
    __syncthreads();
    float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (test_env) plan_metric_product(Mtab, buf, T, n, t, acc);
    if (interior) plan_update(opt.step, opt.smooth_weight, acc, L, lo, hi, q);
    __syncthreads();  // (the next iteration overwrites buf)
  }

  // ---- validity: jerk of the T waypoints, then the refined configurations, lane = configuration -------------------------------
#pragma unroll
  for (int j = 0; j < 7; ++j) buf[lane * 7 + j] = q[j];
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
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o);
  if (lane == 0) cand_bits[k] = bits;
  __syncthreads();

  // ---- the lowest valid candidate ----------------------------------------------------------------------------------------------
  int winner = -1;
  for (int c = K - 1; c >= 0; --c)
    if (cand_bits[c] == 0) winner = c;
  if (all_traj && lane < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) all_traj[(((size_t)b * K + k) * T + lane) * 7 + j] = q[j];
  }
  if (all_status && lane == 0) all_status[(size_t)b * K + k] = bits;
  if (lane < T && (winner == k || (winner < 0 && k == 0))) {
#pragma unroll
    for (int j = 0; j < 7; ++j) traj[((size_t)b * T + lane) * 7 + j] = winner < 0 ? __builtin_nanf("") : q[j];
  }
  if (k == 0 && lane == 0) {
    status[b] = winner >= 0 ? 0 : 1;
    if (choice) choice[b] = winner;
  }
}

MPX_EXPORT int mpx_franka_plan(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                               const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                               const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                               const float *cyl_radii, const float *cyl_heights, int M2, const mpx_plan_options *options,
                               uint64_t seed, int64_t env_offset, float *traj, int32_t *status, int32_t *choice,
                               float *all_traj, int32_t *all_status, mpx_stream_t stream) {
  const char *who = "mpx_franka_plan";
  const mpx_plan_options opt = options ? *options : franka_plan_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (franka_plan_options_check(who, T, opt) || franka_counts_check(who, S, M1, M2) || franka_env_offset_check(who, env_offset, B))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status, "%s: NULL output (traj, status)", who);
  MPX_REQUIRE(q_start && q_goal && limits, "%s: NULL operand (q_start, q_goal, limits)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const int K = opt.candidates;
  const size_t lds = sizeof(float) * ((size_t)128 * 16 + (size_t)T * T + (size_t)K * 64 * 7) + sizeof(int) * K;  // <= 53 312 B
  auto kernel = K <= 8 ? franka_plan_kernel<8> : franka_plan_kernel<MPX_PLAN_MAX_CANDIDATES>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64 * K), lds, mpx_s(stream), q_start, q_goal, T, finger, limits,
                     sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii,
                     cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, traj, status,
                     choice, all_traj, all_status);
  MPX_LAUNCH_CHECK(who);
}
