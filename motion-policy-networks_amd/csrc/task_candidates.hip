// task_candidates.hip -- task-oriented gripper pose candidates: a start or goal drawn ON a scene's supports (a table top, a
// cubby pocket) the way the reference's scene generators pose their problems (tabletop_environment.py:354-404,
// cubby_environment.py:440-549), kept when the free-flying gripper is clear of the scene.  A restatement of those
// distributions judged by this engine's sphere model (gripper_device.h: the clause the gripper roadmap judges by), not by
// PyBullet's meshes.  The contract, uniform by uniform, is stated in include/mpinets_hip.h (mpx_task_candidates).
//
// One workgroup of 128 threads per problem, thread = draw (N <= 128).  Wave 0 stages the live primitives
// (franka_live_rows.inc), wave 1 the gripper's sphere rows (gripper_spheres.inc); behind one barrier every thread makes its
// draw and judges it; the free draws are compacted IN DRAW ORDER by a ballot per wave and one count per wave through LDS
// (position = free draws of the waves before + popcount of the lower lanes: no atomics, no races).  Every barrier is
// reached by all 128 threads.  LDS: 128 x 16 + 64 x 4 + 4 words, static; no scratch memory.
#include "common.h"
#include "franka_host.h"
#include "philox.h"
#include "gripper_device.h"

enum { STREAM_TASK_CANDIDATES = 18 };
enum { TASK_THREADS = 128 };
static_assert(MPX_TASK_MAX_DRAWS == TASK_THREADS, "one thread per draw");
static_assert(MPX_TASK_MAX_CANDIDATES <= TASK_THREADS, "the tail rows are written one per thread");

__global__ void __launch_bounds__(TASK_THREADS)
    task_candidates_kernel(const float *__restrict__ boxes, const int32_t *__restrict__ kinds, int NS,
                           const int32_t *__restrict__ exclude, int C, float finger, const float *__restrict__ sc,
                           const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                           const float *__restrict__ cub_f, const float *__restrict__ cub_d, int M1,
                           const float *__restrict__ cyl_f, const float *__restrict__ cyl_r,
                           const float *__restrict__ cyl_h, int M2, mpx_task_candidates_options opt, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t env0, float *__restrict__ poses, int32_t *__restrict__ draw_out,
                           int32_t *__restrict__ support_out, int32_t *__restrict__ count_out) {
  __shared__ __attribute__((aligned(16))) float prim_rows[128 * 16];
  __shared__ float gsph[GRM_MAX_SPHERES * 4];
  __shared__ int ng_lds[1];
  __shared__ int wave_free[TASK_THREADS / 64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");

#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
#include "gripper_spheres.inc"
  __syncthreads();  // (the primitive rows, the gripper spheres)
  const int n_g = *ng_lds;

  // ---- the draw: thread = draw -------------------------------------------------------------------------------------------
  const float *box = boxes + (size_t)b * NS * 12;
  const int32_t *kind = kinds + (size_t)b * NS;
  const int skip = exclude ? exclude[b] : -1;
  Rigid g = {{nan, nan, nan, nan, nan, nan, nan, nan, nan}, {nan, nan, nan}};
  int pick = -1;
  bool is_free = false;
  if (tid < opt.draws) {
    const Philox p0 = philox4x32(2u * (uint32_t)tid, env0 + (uint32_t)b, STREAM_TASK_CANDIDATES, (uint32_t)opt.role, seed_lo, seed_hi);
    const Philox p1 = philox4x32(2u * (uint32_t)tid + 1u, env0 + (uint32_t)b, STREAM_TASK_CANDIDATES, (uint32_t)opt.role, seed_lo, seed_hi);
    // 1 support: the first whose inclusive cumulative weight exceeds u_0 total
    float total = 0.0f;
    for (int s = 0; s < NS; ++s) {
      const float w = box[12 * s + 11];
      total += (kind[s] != 0 && s != skip && w > 0.0f) ? w : 0.0f;
    }
    const float t = u01(p0.c[0]) * total;
    float cum = 0.0f;
    for (int s = 0; s < NS && pick < 0; ++s) {
      const float w = box[12 * s + 11];
      cum += (kind[s] != 0 && s != skip && w > 0.0f) ? w : 0.0f;
      if (cum > t) pick = s;
    }
    if (pick >= 0) {
      const float *row = box + 12 * pick;
      const bool surface = kind[pick] == 1;
      // 2 position: a point of the top face (surface) or of the box (volume), in the support's frame
      const float sup[7] = {row[0], row[1], row[2], row[7], row[8], row[9], row[6]};  // (centre, quaternion x y z w)
      const Rigid f = gripper_frame(sup);
      const float lx = (u01(p0.c[1]) - 0.5f) * row[3], ly = (u01(p0.c[2]) - 0.5f) * row[4];
      const float u3 = u01(p0.c[3]);
      const float lz = surface ? 0.5f * row[5] : (u3 - 0.5f) * row[5];
      float px, py, pz;
      rigid_apply(f, lx, ly, lz, px, py, pz);
      const float u4 = u01(p1.c[0]);
      if (surface) {
        // lifted onto every primitive it lies on, in index order, each against the already lifted point
        for (int m = 0; m < n_cub; ++m) {
          const float *r = prim_rows + 16 * m;
          if (cuboid_sdf_live(r, r[12], r[13], r[14], px, py, pz) <= 0.01f) pz = -r[11] + r[14] / 2.0f;
        }
        for (int m = 0; m < n_cyl; ++m) {
          const float *r = prim_rows + 16 * (64 + m);
          if (cylinder_sdf_live(r, r[12], r[13], px, py, pz) <= 0.01f) pz = -r[11] + r[13] / 2.0f;
        }
        pz += mpx_fma(1.0f - sqrtf(u3), 0.11f, 0.01f);
        // 3 orientation: R = Rz(yaw) Ry(pitch) Rx(roll), the gripper pointing down
        float sro, cro, sp, cp, sy, cy;
        mpx_sincos(mpx_fma(u4, 1.57079632679489661923f, 2.35619449019234492885f), sro, cro);
        mpx_sincos(mpx_fma(u01(p1.c[1]), 0.78539816339744830962f, -0.39269908169872415481f), sp, cp);
        mpx_sincos(mpx_fma(u01(p1.c[2]), 3.14159265358979323846f, -1.57079632679489661923f), sy, cy);
        g.r[0] = cy * cp, g.r[1] = cy * sp * sro - sy * cro, g.r[2] = cy * sp * cro + sy * sro;
        g.r[3] = sy * cp, g.r[4] = sy * sp * sro + cy * cro, g.r[5] = sy * sp * cro - cy * sro;
        g.r[6] = -sp, g.r[7] = cp * sro, g.r[8] = cp * cro;
      } else {
        // 3 orientation: z along approach + theta, x down, y = z x x
        float sa, ca;
        mpx_sincos(row[10] + mpx_fma(u4, 1.57079632679489661923f, -0.78539816339744830962f), sa, ca);
        g.r[0] = 0.0f, g.r[1] = -sa, g.r[2] = ca;
        g.r[3] = 0.0f, g.r[4] = ca, g.r[5] = sa;
        g.r[6] = -1.0f, g.r[7] = 0.0f, g.r[8] = 0.0f;
      }
      g.t[0] = px, g.t[1] = py, g.t[2] = pz;
      // 4 verdict
      bool finite = true;
#pragma unroll
      for (int i = 0; i < 9; ++i) finite &= __builtin_fabsf(g.r[i]) < inf;  // (NaN fails)
#pragma unroll
      for (int i = 0; i < 3; ++i) finite &= __builtin_fabsf(g.t[i]) < inf;
      is_free = finite && !gripper_frame_hit(g, finger, gsph, n_g, prim_rows, n_cub, n_cyl, opt.clearance, opt.test_self != 0,
                                             opt.self_margin);
    }
  }

  // ---- the first C free draws, in draw order ------------------------------------------------------------------------------
  const unsigned long long fmask = __builtin_amdgcn_ballot_w64(is_free);
  if (lane == 0) wave_free[k] = __builtin_popcountll(fmask);
  __syncthreads();
  const int n_free = wave_free[0] + wave_free[1];
  const int kept = n_free < C ? n_free : C;
  const int at = (k == 0 ? 0 : wave_free[0]) + __builtin_popcountll(fmask & below);
  if (is_free && at < C) {
    float *m = poses + ((size_t)b * C + at) * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      m[4 * i + 0] = g.r[3 * i + 0], m[4 * i + 1] = g.r[3 * i + 1], m[4 * i + 2] = g.r[3 * i + 2], m[4 * i + 3] = g.t[i];
    }
    m[12] = 0.0f, m[13] = 0.0f, m[14] = 0.0f, m[15] = 1.0f;
    draw_out[(size_t)b * C + at] = tid;
    support_out[(size_t)b * C + at] = pick;
  }
  if (tid >= kept && tid < C) {  // (C <= 16: one row per thread)
    float *m = poses + ((size_t)b * C + tid) * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = nan;
    draw_out[(size_t)b * C + tid] = -1;
    support_out[(size_t)b * C + tid] = -1;
  }
  if (tid == 0) count_out[b] = kept;
}

MPX_EXPORT int mpx_task_candidates(const float *support_boxes, const int32_t *support_kind, int B, int NS, const int32_t *exclude,
                                   int C, float finger, const float *sph_centers, const float *sph_radii,
                                   const int32_t *sph_link, int S, const float *cub_inv_frames, const float *cub_dims, int M1,
                                   const float *cyl_inv_frames, const float *cyl_radii, const float *cyl_heights, int M2,
                                   const mpx_task_candidates_options *options, uint64_t seed, int64_t env_offset, float *poses,
                                   int32_t *draw, int32_t *support, int32_t *count, mpx_stream_t stream) {
  const char *who = "mpx_task_candidates";
  const mpx_task_candidates_options opt = options ? *options : task_candidates_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (task_candidates_options_check(who, NS, C, opt) || franka_counts_check(who, S, M1, M2) ||
      franka_env_offset_check(who, env_offset, B) || franka_rows_check(who, B, C * 16, "B x C x 16 pose entries"))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(poses && draw && support && count, "%s: NULL output (poses, draw, support, count)", who);
  MPX_REQUIRE(support_boxes && support_kind, "%s: NULL operand (support_boxes, support_kind)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  hipLaunchKernelGGL(task_candidates_kernel, dim3((unsigned)B), dim3(TASK_THREADS), 0, mpx_s(stream), support_boxes,
                     support_kind, NS, exclude, C, finger, sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1,
                     cyl_inv_frames, cyl_radii, cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)env_offset, poses, draw, support, count);
  MPX_LAUNCH_CHECK(who);
}
