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
// mpx_franka_plan_seeded is the same kernel body (plan_kernel.inc) with Ks more waves that start from the caller's
// trajectories, e.g. roadmap.hip's: candidates 0 .. K-1 and everything after the start are the plain planner's.
#include "common.h"
#include "franka_host.h"
#include "sdf_grad_device.h"
#include "plan_device.h"  // what the planner shares with cloud_field.hip: endpoints, candidates, M g, the jerk test
#include "plan_prims_device.h"  // what it shares with roadmap.hip: the validity test of one configuration

#define PLAN_KERNEL_PARAMS                                                                                                  \
  const float *__restrict__ q_start, const float *__restrict__ q_goal, int T, float finger,                                \
      const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,                        \
      const int32_t *__restrict__ sl, int S, const float *__restrict__ cub_f, const float *__restrict__ cub_d, int M1,     \
      const float *__restrict__ cyl_f, const float *__restrict__ cyl_r, const float *__restrict__ cyl_h, int M2,           \
      mpx_plan_options opt, uint32_t seed_lo, uint32_t seed_hi, uint32_t env0, float *__restrict__ traj,                   \
      int32_t *__restrict__ status, int32_t *__restrict__ choice, float *__restrict__ all_traj,                            \
      int32_t *__restrict__ all_status

// MAXK: the most candidates a launch may carry.  Up to 8 waves per workgroup leave a wave 256 VGPRs (no spills); 16
// leave it 128, where the seven joint frames no longer fit and a few values go to scratch.
template <int MAXK>
__global__ void __launch_bounds__(64 * MAXK) franka_plan_kernel(PLAN_KERNEL_PARAMS) {
#define PLAN_KERNEL_SEEDED 0
#define PLAN_KERNEL_WAVES opt.candidates
#include "plan_kernel.inc"
#undef PLAN_KERNEL_SEEDED
#undef PLAN_KERNEL_WAVES
}
// mpx_franka_plan_seeded: waves opt.candidates .. opt.candidates + Ks - 1 start from seeds[b, k - opt.candidates]
template <int MAXK>
__global__ void __launch_bounds__(64 * MAXK)
    franka_plan_seeded_kernel(PLAN_KERNEL_PARAMS, const float *__restrict__ seeds, int Ks) {
#define PLAN_KERNEL_SEEDED 1
#define PLAN_KERNEL_WAVES (opt.candidates + Ks)
#include "plan_kernel.inc"
#undef PLAN_KERNEL_SEEDED
#undef PLAN_KERNEL_WAVES
}

// the checks and the launch of both entries; seeds == nullptr / Ks == 0: mpx_franka_plan's own kernel
static int franka_plan_launch(const char *who, const float *q_start, const float *q_goal, int B, int T, float finger,
                              const float *limits, const float *sph_centers, const float *sph_radii, const int32_t *sph_link,
                              int S, const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                              const float *cyl_radii, const float *cyl_heights, int M2, const mpx_plan_options *options,
                              uint64_t seed, int64_t env_offset, const float *seeds, int Ks, float *traj, int32_t *status,
                              int32_t *choice, float *all_traj, int32_t *all_status, mpx_stream_t stream) {
  const mpx_plan_options opt = options ? *options : franka_plan_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0 && Ks >= 0, "%s: negative size", who);
  if (franka_plan_options_check(who, T, opt) || franka_counts_check(who, S, M1, M2) || franka_env_offset_check(who, env_offset, B))
    return 1;
  MPX_REQUIRE(opt.candidates + Ks <= MPX_PLAN_MAX_CANDIDATES, "%s: candidates + seeds = %d + %d, at most %d (one wave each)", who,
              opt.candidates, Ks, MPX_PLAN_MAX_CANDIDATES);
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status, "%s: NULL output (traj, status)", who);
  MPX_REQUIRE(q_start && q_goal && limits, "%s: NULL operand (q_start, q_goal, limits)", who);
  MPX_REQUIRE(Ks == 0 || seeds, "%s: Ks > 0 without seeds", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const int K = opt.candidates + Ks;
  const size_t lds = sizeof(float) * ((size_t)128 * 16 + (size_t)T * T + (size_t)K * 64 * 7) + sizeof(int) * K;  // <= 53 312 B
  if (Ks == 0) {
    auto kernel = K <= 8 ? franka_plan_kernel<8> : franka_plan_kernel<MPX_PLAN_MAX_CANDIDATES>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64 * K), lds, mpx_s(stream), q_start, q_goal, T, finger, limits,
                       sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii,
                       cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, traj, status,
                       choice, all_traj, all_status);
  } else {
    auto kernel = K <= 8 ? franka_plan_seeded_kernel<8> : franka_plan_seeded_kernel<MPX_PLAN_MAX_CANDIDATES>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64 * K), lds, mpx_s(stream), q_start, q_goal, T, finger, limits,
                       sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii,
                       cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, traj, status,
                       choice, all_traj, all_status, seeds, Ks);
  }
  MPX_LAUNCH_CHECK(who);
}

MPX_EXPORT int mpx_franka_plan(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                               const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                               const float *cub_inv_frames, const float *cub_dims, int M1, const float *cyl_inv_frames,
                               const float *cyl_radii, const float *cyl_heights, int M2, const mpx_plan_options *options,
                               uint64_t seed, int64_t env_offset, float *traj, int32_t *status, int32_t *choice,
                               float *all_traj, int32_t *all_status, mpx_stream_t stream) {
  return franka_plan_launch("mpx_franka_plan", q_start, q_goal, B, T, finger, limits, sph_centers, sph_radii, sph_link, S,
                            cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2, options, seed, env_offset,
                            nullptr, 0, traj, status, choice, all_traj, all_status, stream);
}

MPX_EXPORT int mpx_franka_plan_seeded(const float *q_start, const float *q_goal, int B, int T, float finger,
                                      const float *limits, const float *sph_centers, const float *sph_radii,
                                      const int32_t *sph_link, int S, const float *cub_inv_frames, const float *cub_dims, int M1,
                                      const float *cyl_inv_frames, const float *cyl_radii, const float *cyl_heights, int M2,
                                      const mpx_plan_options *options, uint64_t seed, int64_t env_offset, const float *seeds,
                                      int Ks, float *traj, int32_t *status, int32_t *choice, float *all_traj,
                                      int32_t *all_status, mpx_stream_t stream) {
  return franka_plan_launch("mpx_franka_plan_seeded", q_start, q_goal, B, T, finger, limits, sph_centers, sph_radii, sph_link, S,
                            cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2, options, seed, env_offset,
                            seeds, Ks, traj, status, choice, all_traj, all_status, stream);
}
