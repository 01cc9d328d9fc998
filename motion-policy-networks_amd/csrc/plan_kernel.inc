// plan_kernel.inc -- the body of the primitive planner's kernel, included by plan.hip as a statement block once per kernel
// (franka_live_rows.inc's idiom: as one inline function for both, franka_plan_kernel<8> / <16> came out with ~430 other
// instruction lines of 21 300; included, the compiler sees the lines it saw when the kernel stood alone).
//   in scope: the kernel's parameters (PLAN_KERNEL_PARAMS of plan.hip)
//   PLAN_KERNEL_SEEDED: 1 adds mpx_franka_plan_seeded's clauses (in scope: seeds, Ks), 0 is mpx_franka_plan's kernel
//   PLAN_KERNEL_WAVES:  the workgroup's waves, one per candidate, the seeded ones last
  // LDS: [128 primitive rows x 16 | M: T x T | per candidate: 64 waypoints x 7 (g, then the trajectory) | K bits]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *prim_rows = lds;
  float *Mtab = lds + 128 * 16;
  const int K = PLAN_KERNEL_WAVES;
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
#if PLAN_KERNEL_SEEDED
  bool dead_seed = false;  // (wave-uniform) a seed with a non-finite entry: the wave keeps the barriers, on the line
  if (k >= opt.candidates) {
    plan_candidate(0, t, T, env0 + (uint32_t)b, seed_lo, seed_hi, opt.spread, qs, qg, lo, hi, L, q);  // (L; q = L)
    const float *row = seeds + (((size_t)b * Ks + (k - opt.candidates)) * T + t) * 7;
    float sq[7];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 7; ++j) sq[j] = row[j], finite &= __builtin_fabsf(sq[j]) < __builtin_inff();  // (NaN fails)
    dead_seed = __any(!finite);
    if (lane >= 1 && lane <= n && !dead_seed) {
#pragma unroll
      for (int j = 0; j < 7; ++j) q[j] = fminf(fmaxf(sq[j], lo[j]), hi[j]);
    }
  } else
#endif
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
#if PLAN_KERNEL_SEEDED
  if (dead_seed) {
    bits = PLAN_BIT_ENV | PLAN_BIT_SELF | PLAN_BIT_JERK;
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = __builtin_nanf("");
  }
#endif
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
