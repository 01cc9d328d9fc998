// follow_cloud.hip -- mpx_franka_follow against a POINT CLOUD: the reactive follower of follow.hip (still the stand-in for
// the reference's Geometric Fabrics expert, NOT Lula's fabric, no parity claimed) with the cloud's truncated distance field
// as its obstacle term and mpx_franka_cloud_collision as the judge of its environment bit -- the field steers, the exact
// test judges, as in cloud_field.hip's planner.  The contract is stated in include/mpinets_hip.h.
//
// One wave per problem, as in follow.hip: the state, the joint origins and axes and the 6x6 solve are wave-uniform; in the
// obstacle term the lane is the collision sphere (S <= 64), its centre is sampled with field_sample<true> (8 loads, issued
// together), and the seven sums over spheres are follow.hip's butterfly of __shfl_xor in a fixed order.  There are no
// primitive rows: the only LDS is the 64 x 7 waypoint buffer.  The time loop is this kernel's OWN COPY of follow.hip's
// (as plan_cloud_kernel.inc is of the planner's): franka_follow_kernel keeps its instruction stream
// (profiles/follow_cloud_timing.md has the comparison).
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

constexpr int FOLLOW_CLOUD_BISECT_ROUNDS = 13;  // 2^13 > MPX_FOLLOW_MAX_STEPS, as in follow.hip
static_assert((1 << FOLLOW_CLOUD_BISECT_ROUNDS) > MPX_FOLLOW_MAX_STEPS, "the retiming search");
static_assert(MPX_FOLLOW_MAX_POSES <= 64 && MPX_PLAN_MAX_T <= 64, "one lane per guide pose / per waypoint");
constexpr int FOLLOW_CLOUD_BAD_BITS = PLAN_BIT_ENV | PLAN_BIT_SELF | PLAN_BIT_JERK | MPX_FOLLOW_BIT_MISS;

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

__device__ __forceinline__ void follow_cloud_load_pose(const float *__restrict__ tg, float (&Rt)[9], float (&pt)[3]) {
  Rt[0] = tg[0], Rt[1] = tg[1], Rt[2] = tg[2], Rt[3] = tg[4], Rt[4] = tg[5], Rt[5] = tg[6], Rt[6] = tg[8], Rt[7] = tg[9],
  Rt[8] = tg[10];
  pt[0] = tg[3], pt[1] = tg[7], pt[2] = tg[11];
}
__device__ __forceinline__ float follow_cloud_distance(const float (&pt)[3], const Rigid &eff) {
  const float dx = pt[0] - eff.t[0], dy = pt[1] - eff.t[1], dz = pt[2] - eff.t[2];
  return sqrtf(mpx_fma(dz, dz, mpx_fma(dy, dy, dx * dx)));
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
  float lo[7], hi[7], q[7], v[7];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    lo[j] = limits[2 * j], hi[j] = limits[2 * j + 1];
    q[j] = q_start[(size_t)b * 7 + j];
    v[j] = v_init ? v_init[(size_t)b * 7 + j] : 0.0f;
    bad |= !((q[j] >= lo[j]) & (q[j] <= hi[j])) | !(__builtin_fabsf(v[j]) < __builtin_inff());  // (NaN fails)
  }
  int w = progress_init ? progress_init[(size_t)b * 3 + 0] : 0;
  int nw = progress_init ? progress_init[(size_t)b * 3 + 1] : 0;
  int fin = progress_init ? (progress_init[(size_t)b * 3 + 2] != 0) : 0;
  bad |= (w < 0) | (w >= W) | (nw < 0);
  {
    bool pose_bad = false;
    if (lane < W) {  // lane = guide pose: its first three rows
#pragma unroll
      for (int i = 0; i < 12; ++i) pose_bad |= !(__builtin_fabsf(my_poses[16 * lane + i]) < __builtin_inff());
    }
    bad |= __any(pose_bad) != 0;
  }

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
      bad_out[b] = 1, pre_bits[b] = FOLLOW_CLOUD_BAD_BITS, steps_out[b] = 0;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        if (q_end) q_end[(size_t)b * 7 + j] = q[j];
        if (v_end) v_end[(size_t)b * 7 + j] = v[j];
      }
      if (progress_end)
        progress_end[(size_t)b * 3 + 0] = w, progress_end[(size_t)b * 3 + 1] = nw, progress_end[(size_t)b * 3 + 2] = fin;
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
  follow_cloud_load_pose(my_poses + 16 * w, Rt, pt);
  int n = 0;
  for (int i = 1; i <= opt.max_steps; ++i) {
    if (fin) break;
    // 1. FK: the joint origins and axes, right_gripper, and this lane's sphere centre from the frame of its link
    float o[7][3], z[7][3], sx = 0.0f, sy = 0.0f, sz = 0.0f;  // (sx, sy, sz: the sphere centre)
    Rigid eff;
    franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
      constexpr int id = decltype(ID)::value;
      if constexpr (id >= 1 && id <= 7) {
        o[id - 1][0] = g.t[0], o[id - 1][1] = g.t[1], o[id - 1][2] = g.t[2];
        z[id - 1][0] = g.r[2], z[id - 1][1] = g.r[5], z[id - 1][2] = g.r[8];
      }
      if constexpr (id == 14) eff = g;
      if constexpr (id >= 1) {
        if (link == id) rigid_apply(g, cx, cy, cz, sx, sy, sz);
      }
    });
    float dist = follow_cloud_distance(pt, eff);
    // 2. switch (at most one advance), 3. stop (only where the last pose was the target on entry)
    const bool last_on_entry = w == W - 1;
    if (!last_on_entry && (dist <= opt.switch_radius || nw >= opt.switch_steps)) {
      ++w, nw = 0;
      follow_cloud_load_pose(my_poses + 16 * w, Rt, pt);
      dist = follow_cloud_distance(pt, eff);
    }
    if (last_on_entry && (dist < opt.final_radius || nw >= opt.final_steps)) {
      fin = 1;
      break;
    }
    // 4. the attractor: mpx_franka_ik's dq
#define DLS_STEP_CLIP opt.step_clip
#include "dls_direction.inc"
#undef DLS_STEP_CLIP
    float u[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) u[j] = dq[j] * scale;
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
    // 6. the acceleration, 7. position first, then the velocity; the clamp into the limits stops a joint
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const float barrier = fmaxf(0.0f, (lo[j] + opt.limit_band) - q[j]) - fmaxf(0.0f, q[j] - (hi[j] - opt.limit_band));
      const float a = ((opt.attract * u[j] - opt.repel * g[j]) + opt.limit_gain * barrier) - opt.damping * v[j];
      const float moved = q[j] + opt.dt * v[j];
      float vn = fminf(fmaxf(v[j] + opt.dt * a, -opt.speed_limit), opt.speed_limit);
      const float qn = fminf(fmaxf(moved, lo[j]), hi[j]);
      if (qn != moved) vn = 0.0f;
      const float dj = qn - q[j];
      ss = j == 0 ? dj * dj : mpx_fma(dj, dj, ss);
      q[j] = qn, v[j] = vn;
    }
    total += sqrtf(ss);
    ++nw;
    n = i;
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 7; ++j) P[(size_t)i * 7 + j] = q[j];
      A[i] = total;
    }
  }
  __threadfence_block();
  __syncthreads();  // (lane 0's path and arc are read by every lane below)

  // ---- retiming: lane = output waypoint -------------------------------------------------------------------------------------
  const int t = lane < T ? lane : T - 1;  // (lanes past the trajectory repeat the last waypoint and never store)
  float qt[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) qt[j] = q[j];  // waypoint T-1 is path[n], the state itself; with n = 0 every waypoint is
  if (n > 0 && t < T - 1) {
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < 7; ++j) qt[j] = P[j];
    } else {
      const float st = ((float)t / (float)(T - 1)) * total;
      int i0 = 0, i1 = n - 1;  // arc[i0] <= st (arc[0] = 0); the answer lies in i0 .. i1
      for (int r = 0; r < FOLLOW_CLOUD_BISECT_ROUNDS; ++r) {
        if (i0 < i1) {
          const int mid = (i0 + i1 + 1) >> 1;
          if (A[mid] <= st)
            i0 = mid;
          else
            i1 = mid - 1;
        }
      }
      const float a0 = A[i0], den = A[i0 + 1] - a0;
      const float fr = den > 0.0f ? fminf(fmaxf((st - a0) / den, 0.0f), 1.0f) : 0.0f;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const float p0 = P[(size_t)i0 * 7 + j];
        qt[j] = mpx_fma(fr, P[(size_t)(i0 + 1) * 7 + j] - p0, p0);
      }
    }
  }

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
  {
    Rigid eff;
    franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
      if constexpr (decltype(ID)::value == 14) eff = g;
    });
    float Rl[9], pl[3];
    follow_cloud_load_pose(my_poses + 16 * (W - 1), Rl, pl);
    if (!(follow_cloud_distance(pl, eff) <= opt.miss_tol * MPX_FOLLOW_MISS_SHARE)) bits |= MPX_FOLLOW_BIT_MISS;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off);

  // ---- results ----------------------------------------------------------------------------------------------------------------
  if (lane < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) waypoints[((size_t)b * T + lane) * 7 + j] = qt[j];
  }
  if (lane == 0) {
    bad_out[b] = 0, pre_bits[b] = bits, steps_out[b] = n;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      if (q_end) q_end[(size_t)b * 7 + j] = q[j];
      if (v_end) v_end[(size_t)b * 7 + j] = v[j];
    }
    if (progress_end)
      progress_end[(size_t)b * 3 + 0] = w, progress_end[(size_t)b * 3 + 1] = nw, progress_end[(size_t)b * 3 + 2] = fin;
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
  const int bits = is_bad ? FOLLOW_CLOUD_BAD_BITS : pre_bits[b] | (traj_flags[b] != 0 ? PLAN_BIT_ENV : 0);
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
