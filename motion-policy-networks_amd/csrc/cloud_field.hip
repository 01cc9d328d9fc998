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
// and a select kernel forms status, choice and traj.
#include "common.h"
#include "franka_host.h"
#include "plan_device.h"

constexpr int FB = MPX_FIELD_BRICK;
constexpr int FIELD_BLOCK = 256;
constexpr int FIELD_NPT = FB * FB * FB / FIELD_BLOCK;  // nodes per thread, stacked along z
constexpr int FIELD_TILE = MPX_CLOUD_TILE;
static_assert(FB == 8 && FIELD_NPT == 2, "the thread -> node map below is written for 8 x 8 x (4 x 2)");
static_assert(FIELD_TILE % FIELD_BLOCK == 0, "MPX_CLOUD_TILE: whole rows of the workgroup");

struct FieldGrid {  // mpx_field_grid as the kernels take it (inv_h formed once on the host)
  float lox, loy, loz, h, inv_h, trunc;
  int nx, ny, nz;
};

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

// The sampler of include/mpinets_hip.h; `f` is ONE environment's nodes.  -> inside (false: D = trunc, gradient 0).
template <bool GRAD>
__device__ __forceinline__ bool field_sample(const float *__restrict__ f, const FieldGrid &G, float x, float y, float z,
                                             float &D, float &gx, float &gy, float &gz) {
  const float u = (x - G.lox) * G.inv_h, v = (y - G.loy) * G.inv_h, w = (z - G.loz) * G.inv_h;
  const bool inside = u >= 0.0f && u <= (float)(G.nx - 1) && v >= 0.0f && v <= (float)(G.ny - 1) && w >= 0.0f &&
                      w <= (float)(G.nz - 1);  // (NaN and infinities fail)
  D = G.trunc, gx = gy = gz = 0.0f;
  if (!inside) return false;
  const int i0 = min((int)floorf(u), G.nx - 2), j0 = min((int)floorf(v), G.ny - 2), k0 = min((int)floorf(w), G.nz - 2);
  const float fx = u - (float)i0, fy = v - (float)j0, fz = w - (float)k0;
  const float *c = f + ((size_t)k0 * G.ny + j0) * G.nx + i0;  // (i0 + 1 < nx, j0 + 1 < ny, k0 + 1 < nz: all 8 inside)
  const size_t sy = (size_t)G.nx, sz = (size_t)G.nx * G.ny;
  const float c000 = c[0], c001 = c[1], c010 = c[sy], c011 = c[sy + 1];  // c[z][y][x]
  const float c100 = c[sz], c101 = c[sz + 1], c110 = c[sz + sy], c111 = c[sz + sy + 1];
  const float X00 = c001 - c000, X01 = c011 - c010, X10 = c101 - c100, X11 = c111 - c110;
  const float a00 = mpx_fma(fx, X00, c000), a01 = mpx_fma(fx, X01, c010);
  const float a10 = mpx_fma(fx, X10, c100), a11 = mpx_fma(fx, X11, c110);
  const float Y0 = a01 - a00, Y1 = a11 - a10;
  const float e0 = mpx_fma(fy, Y0, a00), e1 = mpx_fma(fy, Y1, a10);
  const float Z = e1 - e0;
  D = mpx_fma(fz, Z, e0);
  if (GRAD) {
    const float x0 = mpx_fma(fy, X01 - X00, X00), x1 = mpx_fma(fy, X11 - X10, X10);
    gx = G.inv_h * mpx_fma(fz, x1 - x0, x0);
    gy = G.inv_h * mpx_fma(fz, Y1 - Y0, Y0);
    gz = G.inv_h * Z;
  }
  return true;
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

static int field_grid_check(const char *who, const mpx_field_grid *grid, FieldGrid &G) {
  MPX_REQUIRE(grid, "%s: NULL grid", who);
  const float big = __builtin_huge_valf();
  MPX_REQUIRE(__builtin_fabsf(grid->lo[0]) < big && __builtin_fabsf(grid->lo[1]) < big && __builtin_fabsf(grid->lo[2]) < big,
              "%s: grid lo is not finite", who);
  MPX_REQUIRE(grid->h > 0.0f && grid->h < big, "%s: grid spacing h must be finite and > 0", who);
  MPX_REQUIRE(grid->trunc > 0.0f && grid->trunc < big, "%s: grid trunc must be finite and > 0", who);
  MPX_REQUIRE(grid->nx >= 2 && grid->ny >= 2 && grid->nz >= 2 && grid->nx <= MPX_FIELD_MAX_SIDE &&
                  grid->ny <= MPX_FIELD_MAX_SIDE && grid->nz <= MPX_FIELD_MAX_SIDE,
              "%s: grid of %d x %d x %d nodes, need 2 .. %d per axis", who, grid->nx, grid->ny, grid->nz, MPX_FIELD_MAX_SIDE);
  MPX_REQUIRE((int64_t)grid->nx * grid->ny * grid->nz <= (int64_t)MPX_FIELD_MAX_NODES, "%s: grid of %d x %d x %d nodes, at most %d in all",
              who, grid->nx, grid->ny, grid->nz, MPX_FIELD_MAX_NODES);
  G.lox = grid->lo[0], G.loy = grid->lo[1], G.loz = grid->lo[2];
  G.h = grid->h, G.inv_h = 1.0f / grid->h, G.trunc = grid->trunc;
  G.nx = grid->nx, G.ny = grid->ny, G.nz = grid->nz;
  return 0;
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

// PLAN_BIT_SELF of one configuration (the frames of the self model are all the FK the compiler keeps).  (Its own walk: through
// plan.hip's plan_config_bits without an environment this kernel was 0.6 - 1.3 % slower, profiles/franka_device_timing.md)
__device__ __forceinline__ int plan_self_bits(const float *q, float finger, float self_margin) {
  int bits = 0;
  franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
    constexpr int id = decltype(ID)::value;
    if constexpr (franka_self_sphere(id) >= 0) {
      if (franka_self_hit<id>(g, self_margin)) bits |= PLAN_BIT_SELF;
    }
  });
  return bits;
}

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

// MAXK as for franka_plan_kernel: up to 8 waves per workgroup leave a wave 256 VGPRs.
template <int MAXK>
__global__ void __launch_bounds__(64 * MAXK)
    franka_plan_cloud_kernel(const float *__restrict__ q_start, const float *__restrict__ q_goal, int B, int T, float finger,
                             const float *__restrict__ limits, const float *__restrict__ sc, const float *__restrict__ sr,
                             const int32_t *__restrict__ sl, int S, const float *__restrict__ field, FieldGrid G,
                             float point_radius, mpx_plan_options opt, uint32_t seed_lo, uint32_t seed_hi, uint32_t env0,
                             float *__restrict__ refined, float *__restrict__ ctraj, float *__restrict__ ends,
                             int32_t *__restrict__ cand_bits_out, int32_t *__restrict__ bad_end_out) {
  // LDS: [M: T x T | per candidate: 64 waypoints x 7 (g, then the trajectory)]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *Mtab = lds;
  const int K = opt.candidates;
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
  if (lane == 0) cand_bits_out[(size_t)b * K + k] = bits;
  if (lane < T) {
#pragma unroll
    for (int j = 0; j < 7; ++j) ctraj[(((size_t)b * K + k) * T + lane) * 7 + j] = q[j];
  }
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

MPX_EXPORT int mpx_franka_plan_cloud(const float *q_start, const float *q_goal, int B, int T, float finger, const float *limits,
                                     const float *sph_centers, const float *sph_radii, const int32_t *sph_link, int S,
                                     const float *field, const mpx_field_grid *grid, const float *cloud,
                                     int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                                     float point_radius, const mpx_plan_options *options, uint64_t seed, int64_t env_offset,
                                     float *traj, int32_t *status, int32_t *choice, float *all_traj, int32_t *all_status,
                                     void *scratch, int64_t scratch_bytes, mpx_stream_t stream) {
  const char *who = "mpx_franka_plan_cloud";
  const mpx_plan_options opt = options ? *options : franka_plan_defaults();
  if (franka_plan_options_check(who, T, opt) || franka_counts_check(who, S) || franka_env_offset_check(who, env_offset, B) ||
      franka_cloud_operand_check(who, B, S, N, point_radius, opt.clearance, cloud_point_stride, cloud && N > 0))
    return 1;  // (a short stride is tolerated when no point is read)
  FieldGrid G = {};
  if (field && field_grid_check(who, grid, G)) return 1;
  const int K = opt.candidates, R = (T - 1) * opt.substeps + 1;
  if (franka_rows_check(who, B, R, "B x refined configurations")) return 1;
  const PlanCloudScratch L = plan_cloud_layout(B, T, K, opt.substeps);
  if (franka_scratch_size_check(who, scratch_bytes, (int64_t)L.total_bytes, {B, T, K, opt.substeps})) return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(traj && status, "%s: NULL output (traj, status)", who);
  MPX_REQUIRE(q_start && q_goal && limits, "%s: NULL operand (q_start, q_goal, limits)", who);
  if (franka_scratch_pointer_check(who, scratch) || franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link)) return 1;
  MPX_REQUIRE((!field && (!cloud || N == 0)) || S > 0, "%s: a field or a cloud without collision spheres to test them with", who);
  float *w = static_cast<float *>(scratch);
  int32_t *wi = static_cast<int32_t *>(scratch);
  hipStream_t st = mpx_s(stream);
  hipError_t e = hipMemsetAsync(wi + L.cand_flags, 0, sizeof(int32_t) * ((size_t)K + 1) * B, st);
  MPX_REQUIRE(e == hipSuccess, "%s: memset failed: %s", who, hipGetErrorString(e));
  const size_t lds = sizeof(float) * ((size_t)T * T + (size_t)K * 64 * 7);  // <= 45 056 B
  auto kernel = K <= 8 ? franka_plan_cloud_kernel<8> : franka_plan_cloud_kernel<MPX_PLAN_MAX_CANDIDATES>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64 * K), lds, st, q_start, q_goal, B, T, finger, limits, sph_centers,
                     sph_radii, sph_link, S, field, G, point_radius, opt, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)env_offset, w + L.refined, w + L.ctraj, w + L.ends, wi + L.cand_bits, wi + L.bad_end);
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
