// cloud_field.hip -- planning against a point cloud: a truncated distance field of the cloud, its trilinear sampler, and the
// covariant-gradient planner of plan.hip with the field as its environment term.
//
// plan.hip needs the scene as cuboids and cylinders; a depth cloud or a captured cloud (the reference's real-robot planner,
// interactive_demo/mpinets_ros/nodes/planning_node.py:78-151) has none.  The standard answer of gradient planners is a
// distance field: built once per scene, read at every sphere centre of every iteration.  The field only STEERS: whether a
// candidate is valid is decided by mpx_franka_cloud_collision on its refined configurations, the exact test, unchanged.
// The contracts (pinned arithmetic, what each result depends on) are in include/mpinets_hip.h.
//
// Build (a gather in the mould of franka_cloud_collision_kernel): a workgroup of 256 threads owns one brick of 8 x 8 x 8
// nodes of one environment, two nodes per thread (same x and y: the inner part of the squared distance is shared).  It
// walks the cloud in MPX_CLOUD_TILE-point tiles through double-buffered 16-byte LDS rows, drops the points outside the
// brick's box inflated by more than `trunc` while staging (ballot + prefix popcount, one LDS atomic per wave), and every
// thread takes its minimum over the survivors.  No global atomics, no initialisation pass, no scratch.
//
// Planner: franka_plan_kernel's mapping (workgroup = problem, wave = candidate, lane = waypoint).  The per-sphere work is
// 8 cached global loads and 7 + 4 lerps instead of the loop over live primitives; no primitive rows in LDS.  The kernel
// leaves every candidate's refined configurations candidate-major in scratch; the entry then asks
// mpx_franka_cloud_collision once per candidate (flags only: its bounding-box cull applies) and once for the endpoints,
// and a select kernel forms status, choice and traj.  mpx_franka_plan_cloud_seeded is the same kernel body
// (plan_cloud_kernel.inc) with Ks more waves that start from the caller's trajectories, e.g. roadmap_cloud.hip's.
#include "common.h"
#include "franka_host.h"
#include "plan_device.h"
#include "field_device.h"  // the grid, its check and the sampler: shared with roadmap_cloud.hip

constexpr int FB = MPX_FIELD_BRICK;
constexpr int FIELD_BLOCK = 256;
constexpr int FIELD_NPT = FB * FB * FB / FIELD_BLOCK;  // nodes per thread, stacked along z
constexpr int FIELD_TILE = MPX_CLOUD_TILE;
static_assert(FB == 8 && FIELD_NPT == 2, "the thread -> node map below is written for 8 x 8 x (4 x 2)");
static_assert(FIELD_TILE % FIELD_BLOCK == 0, "MPX_CLOUD_TILE: whole rows of the workgroup");

__global__ void __launch_bounds__(FIELD_BLOCK)
    cloud_field_build_kernel(const float *__restrict__ cloud, int64_t cbs, int cps, int N, const int32_t *__restrict__ counts,
                             FieldGrid G, int bricks_x, int bricks_y, int bricks_env, float *__restrict__ field) {
  constexpr int ROWS = FIELD_TILE / FIELD_BLOCK;
  __shared__ float4 tile[2 * FIELD_TILE];
  __shared__ int cnt[3];  // survivors of tile k in cnt[k % 3]
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x / bricks_env;  // (block-uniform)
  int brick = blockIdx.x - b * bricks_env;
  const int bz = brick / (bricks_x * bricks_y);
  brick -= bz * bricks_x * bricks_y;
  const int by = brick / bricks_x, bx = brick - by * bricks_x;
  const int i0 = bx * FB, j0 = by * FB, k0 = bz * FB;
  if (tid < 3) cnt[tid] = 0;

  // this thread's nodes: (ix, iy, iz + 4 m), m < FIELD_NPT.  A node past the grid (a partial brick) computes and does not store.
  const int ix = i0 + (tid & 7), iy = j0 + ((tid >> 3) & 7), iz = k0 + (tid >> 6);
  const float x = mpx_fma((float)ix, G.h, G.lox), y = mpx_fma((float)iy, G.h, G.loy);
  float z[FIELD_NPT], best[FIELD_NPT];
#pragma unroll
  for (int m = 0; m < FIELD_NPT; ++m) z[m] = mpx_fma((float)(iz + 4 * m), G.h, G.loz), best[m] = __builtin_inff();

  // The box of the brick's nodes that exist (h > 0: the corner nodes bound the rest), inflated.  A point with p.x < bx0 =
  // fl(xa - infl) is dropped.  Then for every node x >= xa of the brick x - p.x > xa - bx0 >= infl - 2^-24 (amax + infl) >
  // trunc (1 + 1e-5): the relative part of `infl` covers trunc, its second part is 16 x the rounding of bx0 itself.  The
  // device's dx = fl(x - p.x) >= trunc (1 + 1e-5)(1 - 2^-24), and mpx_sqdist is monotone in |dx| with non-negative other
  // terms, so d2 >= fl(dx dx) >= trunc^2 (1 + 1e-5)^2 (1 - 2^-24)^3 > trunc^2 (1 + 2^-23) and sqrtf(d2) >= trunc: the point
  // could only have produced a value that fminf(., trunc) replaces by trunc, which is also what a node without any
  // nearer point gets.  The same on the other five faces (cloud_collision.hip's argument with R = trunc).
  const float xa = mpx_fma((float)i0, G.h, G.lox), xb = mpx_fma((float)min(i0 + FB - 1, G.nx - 1), G.h, G.lox);
  const float ya = mpx_fma((float)j0, G.h, G.loy), yb = mpx_fma((float)min(j0 + FB - 1, G.ny - 1), G.h, G.loy);
  const float za = mpx_fma((float)k0, G.h, G.loz), zb = mpx_fma((float)min(k0 + FB - 1, G.nz - 1), G.h, G.loz);
  const float amax = fmaxf(fmaxf(fmaxf(fabsf(xa), fabsf(xb)), fmaxf(fabsf(ya), fabsf(yb))), fmaxf(fabsf(za), fabsf(zb)));
  const float infl = (G.trunc * 1.00001f + 1e-6f * (amax + G.trunc)) + 1e-12f;
  const float bx0 = xa - infl, by0 = ya - infl, bz0 = za - infl, bx1 = xb + infl, by1 = yb + infl, bz1 = zb + infl;

  int n = N;
  if (counts) n = min(max(counts[b], 0), N);
  const int ntiles = (n + FIELD_TILE - 1) / FIELD_TILE;
  const float *cb = cloud + (int64_t)b * cbs;
  float px[ROWS], py[ROWS], pz[ROWS];
  auto fetch = [&](int k) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int i = k * FIELD_TILE + r * FIELD_BLOCK + tid;
      px[r] = py[r] = pz[r] = 0.0f;
      if (i < n) {
        const float *p = cb + (int64_t)i * cps;
        px[r] = p[0], py[r] = p[1], pz[r] = p[2];
      }
    }
  };
  auto stage = [&](int k) __attribute__((always_inline)) {
    float4 *dst = tile + (k & 1) * FIELD_TILE;
    const float inf = __builtin_inff();
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const bool ok = k * FIELD_TILE + r * FIELD_BLOCK + tid < n;
      const bool finite = fabsf(px[r]) < inf && fabsf(py[r]) < inf && fabsf(pz[r]) < inf;  // (false for NaN)
      const bool keep = ok && finite && !(px[r] < bx0 || px[r] > bx1 || py[r] < by0 || py[r] > by1 || pz[r] < bz0 || pz[r] > bz1);
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
      int slot = 0;
      if (lane == 0 && mask) slot = atomicAdd(&cnt[k % 3], __builtin_popcountll(mask));
      slot = __builtin_amdgcn_readfirstlane(slot);
      // (slot + rank < the points staged so far of this tile <= FIELD_TILE: inside the buffer)
      if (keep) dst[slot + __builtin_popcountll(mask & (((unsigned long long)1 << lane) - 1))] = make_float4(px[r], py[r], pz[r], 0.0f);
    }
  };
  __syncthreads();  // cnt is zero
  if (ntiles > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  for (int k = 0; k < ntiles; ++k) {
    if (k + 1 < ntiles) fetch(k + 1);
    // (slot k + 2's counter: last read while tile k - 1 was walked, next added to after this tile's barrier)
    if (tid == 0) cnt[(k + 2) % 3] = 0;
    const int m = __builtin_amdgcn_readfirstlane(cnt[k % 3]);
    const float4 *src = tile + (k & 1) * FIELD_TILE;
#pragma unroll 2
    for (int j = 0; j < m; ++j) {
      const float4 p = src[j];  // (every lane the same address: a broadcast read)
      const float dx = x - p.x, dy = y - p.y;
#pragma unroll
      for (int u = 0; u < FIELD_NPT; ++u) best[u] = fminf(best[u], mpx_sqdist(dx, dy, z[u] - p.z));
    }
    if (k + 1 < ntiles) stage(k + 1);
    __syncthreads();
  }
  if (ix < G.nx && iy < G.ny) {
    float *out = field + (size_t)b * ((size_t)G.nx * G.ny * G.nz);
#pragma unroll
    for (int u = 0; u < FIELD_NPT; ++u) {
      const int kz = iz + 4 * u;
      if (kz < G.nz) out[((size_t)kz * G.ny + iy) * G.nx + ix] = fminf(sqrtf(best[u]), G.trunc);
    }
  }
}

__global__ void __launch_bounds__(256)
    cloud_field_sample_kernel(const float *__restrict__ field, FieldGrid G, int64_t total, int P, const float *__restrict__ points,
                              int64_t pbs, int pps, float *__restrict__ dist, float *__restrict__ grad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / P, p = i - b * P;
  const float *pt = points + b * pbs + p * pps;
  const float *f = field + (size_t)b * ((size_t)G.nx * G.ny * G.nz);
  float D, gx, gy, gz;
  if (grad) {
    field_sample<true>(f, G, pt[0], pt[1], pt[2], D, gx, gy, gz);
    grad[3 * i + 0] = gx, grad[3 * i + 1] = gy, grad[3 * i + 2] = gz;
  } else {
    field_sample<false>(f, G, pt[0], pt[1], pt[2], D, gx, gy, gz);
  }
  dist[i] = D;
}

MPX_EXPORT int mpx_cloud_field_build(const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                                     const int32_t *counts, int B, const mpx_field_grid *grid, float *field,
                                     mpx_stream_t stream) {
  MPX_REQUIRE(B >= 0 && N >= 0, "mpx_cloud_field_build: negative size");
  MPX_REQUIRE(cloud_point_stride >= 3, "mpx_cloud_field_build: cloud_point_stride < 3");
  FieldGrid G;
  if (field_grid_check("mpx_cloud_field_build", grid, G)) return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(field && (cloud || N == 0), "mpx_cloud_field_build: NULL operand (field, cloud)");
  const int bricks_x = cdiv(G.nx, FB), bricks_y = cdiv(G.ny, FB), bricks_z = cdiv(G.nz, FB);
  const int64_t bricks_env = (int64_t)bricks_x * bricks_y * bricks_z;
  MPX_REQUIRE(bricks_env * B < (int64_t)1 << 31, "mpx_cloud_field_build: too many workgroups (%lld bricks x %d)", (long long)bricks_env, B);
  hipLaunchKernelGGL(cloud_field_build_kernel, dim3((unsigned)(bricks_env * B)), dim3(FIELD_BLOCK), 0, mpx_s(stream), cloud,
                     cloud_batch_stride, cloud_point_stride, N, counts, G, bricks_x, bricks_y, (int)bricks_env, field);
  MPX_LAUNCH_CHECK("mpx_cloud_field_build");
}

MPX_EXPORT int mpx_cloud_field_sample(const float *field, const mpx_field_grid *grid, int B, const float *points,
                                      int64_t points_batch_stride, int points_point_stride, int P, float *dist, float *grad,
                                      mpx_stream_t stream) {
  MPX_REQUIRE(B >= 0 && P >= 0, "mpx_cloud_field_sample: negative size");
  MPX_REQUIRE(points_point_stride >= 3, "mpx_cloud_field_sample: points_point_stride < 3");
  FieldGrid G;
  if (field_grid_check("mpx_cloud_field_sample", grid, G)) return 1;
  if (B == 0 || P == 0) return 0;
  MPX_REQUIRE(field && points && dist, "mpx_cloud_field_sample: NULL operand (field, points, dist)");
  const int64_t total = (int64_t)B * P;
  MPX_REQUIRE((total + 255) / 256 < (int64_t)1 << 31, "mpx_cloud_field_sample: too many workgroups");
  hipLaunchKernelGGL(cloud_field_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, mpx_s(stream), field, G,
                     total, P, points, points_batch_stride, points_point_stride, dist, grad);
  MPX_LAUNCH_CHECK("mpx_cloud_field_sample");
}

// ---- the planner ---------------------------------------------------------------------------------------------------------------

struct PlanCloudScratch {  // all in 4-byte words, from the start of `scratch`
  size_t refined;          // float [K, B, R, 7]: candidate-major, what one flags call per candidate reads
  size_t ctraj;            // float [B, K, T, 7]: every candidate's final trajectory
  size_t ends;             // float [B, 2, 7]
  size_t cand_flags;       // int32 [K, B] then end_flags int32 [B]: zeroed on the stream, OR-ed into by the flag calls
  size_t end_flags;
  size_t cand_bits;        // int32 [B, K]: jerk and self bits
  size_t bad_end;          // int32 [B]: an endpoint is not finite, outside the limits or fails the self test
  size_t total_bytes;
};
static PlanCloudScratch plan_cloud_layout(int B, int T, int K, int substeps) {
  PlanCloudScratch L;
  const size_t R = (size_t)(T - 1) * substeps + 1, b = (size_t)B, k = (size_t)K;
  size_t at = 0;
  L.refined = at, at += k * b * R * 7;
  L.ctraj = at, at += b * k * (size_t)T * 7;
  L.ends = at, at += b * 14;
  L.cand_flags = at, at += k * b;
  L.end_flags = at, at += b;
  L.cand_bits = at, at += b * k;
  L.bad_end = at, at += b;
  L.total_bytes = (at * 4 + 15) & ~(size_t)15;
  return L;
}

#define PLAN_CLOUD_KERNEL_PARAMS                                                                                            \
  const float *__restrict__ q_start, const float *__restrict__ q_goal, int B, int T, float finger,                         \
      const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,                        \
      const int32_t *__restrict__ sl, int S, const float *__restrict__ field, FieldGrid G, float point_radius,             \
      mpx_plan_options opt, uint32_t seed_lo, uint32_t seed_hi, uint32_t env0, float *__restrict__ refined,                \
      float *__restrict__ ctraj, float *__restrict__ ends, int32_t *__restrict__ cand_bits_out,                            \
      int32_t *__restrict__ bad_end_out

// MAXK as for franka_plan_kernel: up to 8 waves per workgroup leave a wave 256 VGPRs.
template <int MAXK>
__global__ void __launch_bounds__(64 * MAXK) franka_plan_cloud_kernel(PLAN_CLOUD_KERNEL_PARAMS) {
#define PLAN_KERNEL_SEEDED 0
#define PLAN_KERNEL_WAVES opt.candidates
#include "plan_cloud_kernel.inc"
#undef PLAN_KERNEL_SEEDED
#undef PLAN_KERNEL_WAVES
}
// mpx_franka_plan_cloud_seeded: waves opt.candidates .. opt.candidates + Ks - 1 start from seeds[b, k - opt.candidates]
template <int MAXK>
__global__ void __launch_bounds__(64 * MAXK)
    franka_plan_cloud_seeded_kernel(PLAN_CLOUD_KERNEL_PARAMS, const float *__restrict__ seeds, int Ks) {
#define PLAN_KERNEL_SEEDED 1
#define PLAN_KERNEL_WAVES (opt.candidates + Ks)
#include "plan_cloud_kernel.inc"
#undef PLAN_KERNEL_SEEDED
#undef PLAN_KERNEL_WAVES
}

// status, choice, traj and the optional all_* of problem b from the optimise kernel's bits and the flag calls' flags
__global__ void __launch_bounds__(256)
    franka_plan_cloud_select_kernel(int B, int T, int K, const float *__restrict__ ctraj, const int32_t *__restrict__ cand_bits,
                                    const int32_t *__restrict__ cand_flags, const int32_t *__restrict__ end_flags,
                                    const int32_t *__restrict__ bad_end, float *__restrict__ traj, int32_t *__restrict__ status,
                                    int32_t *__restrict__ choice, float *__restrict__ all_traj, int32_t *__restrict__ all_status) {
  const int b = blockIdx.x, tid = (int)threadIdx.x;
  const bool bad = bad_end[b] != 0 || end_flags[b] != 0;  // (block-uniform)
  int winner = -1;
  for (int c = K - 1; c >= 0; --c) {
    const int bits = cand_bits[(size_t)b * K + c] | (cand_flags[(size_t)c * B + b] != 0 ? PLAN_BIT_ENV : 0);
    if (bits == 0) winner = c;
    if (all_status && tid == 0) all_status[(size_t)b * K + c] = bad ? (PLAN_BIT_ENV | PLAN_BIT_SELF | PLAN_BIT_JERK) : bits;
  }
  if (bad) winner = -1;
  const float nan = __builtin_nanf("");
  const float *src = ctraj + (size_t)b * K * T * 7;
  if (all_traj)
    for (int i = tid; i < K * T * 7; i += 256) all_traj[(size_t)b * K * T * 7 + i] = bad ? nan : src[i];
  for (int i = tid; i < T * 7; i += 256) traj[(size_t)b * T * 7 + i] = winner < 0 ? nan : src[(size_t)winner * T * 7 + i];
  if (tid == 0) {
    status[b] = bad ? 2 : winner >= 0 ? 0 : 1;
    if (choice) choice[b] = winner;
  }
}

MPX_EXPORT int64_t mpx_franka_plan_cloud_scratch(int B, int T, int candidates, int substeps) {
  if (B < 0 || !franka_plan_T_ok(T) || !franka_plan_candidates_ok(candidates) || !franka_plan_substeps_ok(substeps)) return -1;
  return (int64_t)plan_cloud_layout(B, T, candidates, substeps).total_bytes;
}

// the checks and the launches of both entries; seeds == nullptr / Ks == 0: mpx_franka_plan_cloud's own kernel
static int franka_plan_cloud_launch(const char *who, const float *q_start, const float *q_goal, int B, int T, float finger,
                                    const float *limits, const float *sph_centers, const float *sph_radii,
                                    const int32_t *sph_link, int S, const float *field, const mpx_field_grid *grid,
                                    const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                                    const int32_t *counts, float point_radius, const mpx_plan_options *options, uint64_t seed,
                                    int64_t env_offset, const float *seeds, int Ks, float *traj, int32_t *status,
                                    int32_t *choice, float *all_traj, int32_t *all_status, void *scratch, int64_t scratch_bytes,
                                    mpx_stream_t stream) {
  const mpx_plan_options opt = options ? *options : franka_plan_defaults();
  if (franka_plan_options_check(who, T, opt) || franka_counts_check(who, S) || franka_env_offset_check(who, env_offset, B) ||
      franka_cloud_operand_check(who, B, S, N, point_radius, opt.clearance, cloud_point_stride, cloud && N > 0))
    return 1;  // (a short stride is tolerated when no point is read)
  MPX_REQUIRE(Ks >= 0, "%s: negative size", who);
  MPX_REQUIRE(opt.candidates + Ks <= MPX_PLAN_MAX_CANDIDATES, "%s: candidates + seeds = %d + %d, at most %d (one wave each)", who,
              opt.candidates, Ks, MPX_PLAN_MAX_CANDIDATES);
  FieldGrid G = {};
  if (field && field_grid_check(who, grid, G)) return 1;
  const int K = opt.candidates + Ks, R = (T - 1) * opt.substeps + 1;
  if (franka_rows_check(who, B, R, "B x refined configurations")) return 1;
  const PlanCloudScratch L = plan_cloud_layout(B, T, K, opt.substeps);
  // (the size query both entries share is named after the plain one: the message names it, with K + Ks candidates)
  if (franka_scratch_size_check("mpx_franka_plan_cloud", scratch_bytes, (int64_t)L.total_bytes, {B, T, K, opt.substeps})) return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status, "%s: NULL output (traj, status)", who);
  MPX_REQUIRE(q_start && q_goal && limits, "%s: NULL operand (q_start, q_goal, limits)", who);
  MPX_REQUIRE(Ks == 0 || seeds, "%s: Ks > 0 without seeds", who);
  if (franka_scratch_pointer_check(who, scratch) || franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  MPX_REQUIRE((!field && (!cloud || N == 0)) || S > 0, "%s: a field or a cloud without collision spheres to test them with", who);
  float *w = static_cast<float *>(scratch);
  int32_t *wi = static_cast<int32_t *>(scratch);
  hipStream_t st = mpx_s(stream);
  hipError_t e = hipMemsetAsync(wi + L.cand_flags, 0, sizeof(int32_t) * ((size_t)K + 1) * B, st);
  MPX_REQUIRE(e == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(e));
  const size_t lds = sizeof(float) * ((size_t)T * T + (size_t)K * 64 * 7);  // <= 45 056 B
  if (Ks == 0) {
    auto kernel = K <= 8 ? franka_plan_cloud_kernel<8> : franka_plan_cloud_kernel<MPX_PLAN_MAX_CANDIDATES>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64 * K), lds, st, q_start, q_goal, B, T, finger, limits, sph_centers,
                       sph_radii, sph_link, S, field, G, point_radius, opt, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)env_offset, w + L.refined, w + L.ctraj, w + L.ends, wi + L.cand_bits, wi + L.bad_end);
  } else {
    auto kernel = K <= 8 ? franka_plan_cloud_seeded_kernel<8> : franka_plan_cloud_seeded_kernel<MPX_PLAN_MAX_CANDIDATES>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64 * K), lds, st, q_start, q_goal, B, T, finger, limits, sph_centers,
                       sph_radii, sph_link, S, field, G, point_radius, opt, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)env_offset, w + L.refined, w + L.ctraj, w + L.ends, wi + L.cand_bits, wi + L.bad_end, seeds, Ks);
  }
  e = hipGetLastError();
  MPX_REQUIRE(e == hipSuccess, "%s: launch failed: %s", who, hipGetErrorString(e));
  if (cloud && N > 0 && S > 0) {
    const float reach = opt.clearance + opt.check_margin;  // (float32, as the contract says)
    for (int k = 0; k < K; ++k)
      if (mpx_franka_cloud_collision(w + L.refined + (size_t)k * B * R * 7, B, R, finger, sph_centers, sph_radii, sph_link, S,
                                     cloud, cloud_batch_stride, cloud_point_stride, N, counts, point_radius, reach,
                                     wi + L.cand_flags + (size_t)k * B, nullptr, nullptr, stream))
        return 1;
    if (mpx_franka_cloud_collision(w + L.ends, B, 2, finger, sph_centers, sph_radii, sph_link, S, cloud, cloud_batch_stride,
                                   cloud_point_stride, N, counts, point_radius, reach, wi + L.end_flags, nullptr, nullptr,
                                   stream))
      return 1;
  }
  hipLaunchKernelGGL(franka_plan_cloud_select_kernel, dim3((unsigned)B), dim3(256), 0, st, B, T, K, w + L.ctraj,
                     wi + L.cand_bits, wi + L.cand_flags, wi + L.end_flags, wi + L.bad_end, traj, status, choice, all_traj,
                     all_status);
  MPX_LAUNCH_CHECK(who);
}

MPX_EXPORT int mpx_franka_plan_cloud(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                                     const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                     const float *field, const mpx_field_grid *grid, const float *cloud,
                                     int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                                     float point_radius, const mpx_plan_options *options, uint64_t seed, int64_t env_offset,
                                     float *traj, int32_t *status, int32_t *choice, float *all_traj, int32_t *all_status,
                                     void *scratch, int64_t scratch_bytes, mpx_stream_t stream) {
  return franka_plan_cloud_launch("mpx_franka_plan_cloud", q_start, q_goal, B, T, finger, limits, sph_centers, sph_radii, sph_link,
                                  S, field, grid, cloud, cloud_batch_stride, cloud_point_stride, N, counts, point_radius, options,
                                  seed, env_offset, nullptr, 0, traj, status, choice, all_traj, all_status, scratch, scratch_bytes,
                                  stream);
}

MPX_EXPORT int mpx_franka_plan_cloud_seeded(const float *q_start, const float *q_goal, int B, int T, float finger,
                                            const float *limits, const float *sph_centers, const float *sph_radii,
                                            const int32_t *sph_link, int S, const float *field, const mpx_field_grid *grid,
                                            const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                                            const int32_t *counts, float point_radius, const mpx_plan_options *options,
                                            uint64_t seed, int64_t env_offset, const float *seeds, int Ks, float *traj,
                                            int32_t *status, int32_t *choice, float *all_traj, int32_t *all_status, void *scratch,
                                            int64_t scratch_bytes, mpx_stream_t stream) {
  return franka_plan_cloud_launch("mpx_franka_plan_cloud_seeded", q_start, q_goal, B, T, finger, limits, sph_centers, sph_radii,
                                  sph_link, S, field, grid, cloud, cloud_batch_stride, cloud_point_stride, N, counts,
                                  point_radius, options, seed, env_offset, seeds, Ks, traj, status, choice, all_traj, all_status,
                                  scratch, scratch_bytes, stream);
}
