// plan_cloud_kernel.inc -- the body of the cloud planner's optimise kernel, included by cloud_field.hip as a statement block once
// per kernel (plan_kernel.inc's idiom: the compiler sees the lines it saw when franka_plan_cloud_kernel stood alone;
// profiles/roadmap_cloud_timing.md has the instruction-stream comparison).
//   in scope: the kernel's parameters (PLAN_CLOUD_KERNEL_PARAMS of cloud_field.hip)
//   PLAN_KERNEL_SEEDED: 1 adds mpx_franka_plan_cloud_seeded's clauses (in scope: seeds, Ks), 0 is mpx_franka_plan_cloud's kernel
//   PLAN_KERNEL_WAVES:  the workgroup's waves, one per candidate, the seeded ones last
  // LDS: [M: T x T | per candidate: 64 waypoints x 7 (g, then the trajectory)]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *Mtab = lds;
  const int K = PLAN_KERNEL_WAVES;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // candidate of this wave
  float *buf = Mtab + T * T + k * 64 * 7;
  const int n = T - 2;
  const int t = lane < T ? lane : T - 1;  // (lanes past the trajectory repeat the goal and never store)

  float lo[7], hi[7], qs[7], qg[7];
  bool bad_end = plan_endpoints(limits, q_start, q_goal, b, lo, hi, qs, qg);
  plan_fill_metric(Mtab, T, n);
  __syncthreads();

  const bool test_env = field != nullptr && S > 0, test_self = opt.check_self != 0;
  // ---- endpoints: limits and the self test here; the cloud test is the entry's flag call on `ends`.  A bad endpoint does
  // not end the workgroup: the select kernel discards what it computes (no row of scratch is left unwritten for the flag
  // calls to read), and arithmetic on a NaN endpoint touches no memory (a NaN centre is outside the grid).
  if (k == 0) {
    if (!bad_end && test_self) {  // (the limits test is wave-uniform)
      int e = 0;
      float qe[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) qe[j] = lane == 0 ? qs[j] : qg[j];
      if (lane < 2) e = plan_self_bits(qe, finger, opt.check_margin);
      bad_end = __any(e != 0);
    }
    if (lane < 14) ends[(size_t)b * 14 + lane] = lane < 7 ? q_start[(size_t)b * 7 + lane] : q_goal[(size_t)b * 7 + lane - 7];
    if (lane == 0) bad_end_out[b] = bad_end ? 1 : 0;
  }

  // ---- this lane's waypoint of candidate k ---------------------------------------------------------------------------------
  float L[7], q[7];
#if PLAN_KERNEL_SEEDED
  bool dead_seed = false;  // (wave-uniform) a seed with a non-finite entry: the wave runs on, from the line, and its result is discarded
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

  // ---- covariant gradient descent: franka_plan_kernel's loop with the field as its environment term.  (Its own copy:
  // one shared loop made this kernel 1.5 % slower, profiles/franka_device_timing.md) --------------------------------------------
  const float inv_eps = 1.0f / opt.epsilon;
  const float *f = test_env ? field + (size_t)b * ((size_t)G.nx * G.ny * G.nz) : nullptr;
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
            float x, y, zz, D, nx, ny, nz;
            rigid_apply(fr, sc[3 * s + 0], sc[3 * s + 1], sc[3 * s + 2], x, y, zz);
            field_sample<true>(f, G, x, y, zz, D, nx, ny, nz);
            const float d = ((D - point_radius) - sr[s]) - opt.clearance;
            if (D < G.trunc && d < opt.epsilon) {  // (D >= trunc: saturated, or outside the grid)
              const float cp = d < 0.0f ? -1.0f : (d - opt.epsilon) * inv_eps;
              nx *= cp, ny *= cp, nz *= cp;
              plan_joint_terms<nj>(o, z, x, y, zz, nx, ny, nz, g);
            }
          }
        }
      });
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) buf[lane * 7 + j] = g[j];
    __syncthreads();  // (as in franka_plan_kernel: every wave runs the same iteration count)
    float acc[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (test_env) plan_metric_product(Mtab, buf, T, n, t, acc);
    if (interior) plan_update(opt.step, opt.smooth_weight, acc, L, lo, hi, q);
    __syncthreads();  // (the next iteration overwrites buf)
  }

  // ---- jerk of the T waypoints; the refined configurations go to scratch (and through the self test), lane = configuration ---
#pragma unroll
  for (int j = 0; j < 7; ++j) buf[lane * 7 + j] = q[j];
  __syncthreads();
  int bits = plan_jerk_bits(buf, lane, T, opt.max_jerk);
  const int R = (T - 1) * opt.substeps + 1;
  float *ref = refined + ((size_t)k * B + b) * (size_t)R * 7;
  for (int r0 = 0; r0 < R; r0 += 64) {
    const int r = r0 + lane;
    if (r < R) {
      float qq[7];
      plan_refined(buf, r, opt.substeps, qq);
#pragma unroll
      for (int j = 0; j < 7; ++j) ref[(size_t)r * 7 + j] = qq[j];
      if (test_self) bits |= plan_self_bits(qq, finger, opt.check_margin);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o);
#if PLAN_KERNEL_SEEDED
  if (dead_seed) {  // (its refined rows come from the line: finite, so the flag calls read numbers; the verdict is fixed here)
    bits = PLAN_BIT_ENV | PLAN_BIT_SELF | PLAN_BIT_JERK;
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = __builtin_nanf("");
  }
#endif
  if (lane == 0) cand_bits_out[(size_t)b * K + k] = bits;
  if (lane < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) ctraj[(((size_t)b * K + k) * T + lane) * 7 + j] = q[j];
  }
