// launch_routes.h -- which kernel form each host launcher takes, stated once.
// Plain C++17, no HIP: integers in, a small POD out, nothing launched and no state read.  A launcher computes its route
// first and then dispatches on it; the mpx_*_route queries (include/mpinets_hip.h) hand the same structs to the tests, and
// tests/test_launch_routes_host.py compiles this header on its own with a host compiler.
#pragma once
#include <stdint.h>

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- mpx_fps (pointnet.hip) ---------------------------------------------------------------------------------------------
#ifndef MPX_FPS4_MIN_B
#define MPX_FPS4_MIN_B 768  // from this many environments on, the 4-wave culled FPS (A/B: tools/ab_build.sh)
#endif
constexpr int FPS_MAX_N = 8192;                       // 512 threads x 16 points (include/mpinets_hip.h says the same)
constexpr int FPS_MAX_LDS = 256 + 3 * FPS_MAX_N * 4;  // the cloud copy of the largest supported launch
constexpr int FPSC_CELLS = 4096;
// dynamic LDS of fps_cull_kernel: [0,256) reduction slots, [256,768) scalars (position of point 0, cloud bounding box
// exchange), then the cloud in sorted order sx | sy | sz (3 N floats); the prologue's histogram (16 KB) and position ->
// index map (2 N bytes) live in the same area before the coordinates are written
constexpr int64_t fpsc_lds_bytes(int N, bool nocloud = false) {
  const int64_t cloud = nocloud ? 0 : (int64_t)3 * N * 4, pro = (int64_t)FPSC_CELLS * 4 + (((int64_t)N * 2 + 15) & ~(int64_t)15);
  return 768 + (cloud > pro ? cloud : pro);
}
inline int opt_n_threads_log2(int n) {
  int l = 0;
  while ((2 << l) <= n && (2 << l) <= 512) ++l;
  return l;
}

enum { FPS_PLAIN = 0, FPS_WAVE = 1, FPS_CULL8 = 2, FPS_CULL4 = 3 };
struct FpsRoute {
  int family;   // FPS_*
  int pts;      // points per lane: the instantiation (0: none serves this shape)
  int threads;  // workgroup size
  int lds;      // dynamic LDS, bytes
};
// `fast`: the MPX_VARIANT_FPS switch (0: the plain kernel at every size)
inline FpsRoute fps_route(int B, int N, int fast) {
  if (fast && N <= 512) {  // small cloud: one wave per environment, no LDS, no barrier
    switch ((N + 63) / 64) {
      case 1: return {FPS_WAVE, 1, 64, 0};
      case 2: return {FPS_WAVE, 2, 64, 0};
      case 3: case 4: return {FPS_WAVE, 4, 64, 0};
      default: return {FPS_WAVE, 8, 64, 0};
    }
  }
  if (fast && N > 512) {  // (log2bs == 9 here: the key layout of fps_cull_kernel assumes it)
    // large clouds (the first module's 6272 points): the 4-wave form without the LDS copy of the cloud -- three
    // workgroups per CU instead of two (6.45 -> 6.11 ms at 8192 environments; with the LDS copy, two per CU: 7.10 ms)
    // (a few hundred environments or fewer are latency-bound, not throughput-bound: they keep the 8-wave form, whose pick
    // chain is shorter -- one planning problem: 0.69 vs 0.80 ms per step.  Same indices either way.)
    // (wave counts measured in round 3 at 8192 environments x 6272 points: 16 waves x 7 points per lane 8.31 ms, 8 x 13
    // 6.41 ms, 4 x 25 with the LDS cloud copy 7.10 ms, 4 x 25 without it 6.11 ms: the cross-wave reduction and the
    // barrier get cheaper with fewer waves, the per-wave pass longer; what pays is the third workgroup per CU.)
    const int waves = (N > 16 * 256 && B >= MPX_FPS4_MIN_B) ? 4 : 8;
    const int lds_c = (int)fpsc_lds_bytes(N, waves == 4);
    const int pts_c = (N + 64 * waves - 1) / (64 * waves);
    if (waves == 4) return {FPS_CULL4, pts_c <= 20 ? 20 : pts_c <= 25 ? 25 : 32, 256, lds_c};
    const int p = pts_c <= 2 ? 2 : pts_c <= 4 ? 4 : pts_c <= 6 ? 6 : pts_c <= 8 ? 8 : pts_c <= 10 ? 10 : pts_c <= 13 ? 13 : 16;
    return {FPS_CULL8, p, 512, lds_c};
  }
  int block = ((N + 63) / 64) * 64;
  if (block > 512) block = 512;  // measured: 512 threads x 13 points beat 1024 x 7
  const int pts = (N + block - 1) / block;
  const int lds = 256 + 3 * N * 4;
  switch (pts) {
    case 1: case 2: case 3: case 4: case 5: case 6: case 7: case 8: return {FPS_PLAIN, pts, block, lds};
    case 9: case 10: return {FPS_PLAIN, 10, block, lds};
    case 11: case 12: case 13: return {FPS_PLAIN, 13, block, lds};
    case 14: case 15: case 16: return {FPS_PLAIN, 16, block, lds};
    default: return {FPS_PLAIN, 0, block, lds};
  }
}

// ---- mpx_franka_collision (franka.hip) ----------------------------------------------------------------------------------
constexpr int COL_PPB = 16;  // (environment, waypoint) pairs per workgroup of the general kernel
#ifndef MPX_COL_TC
#define MPX_COL_TC 64  // waypoints per workgroup of the swept-sphere check (A/B: tools/ab_build.sh)
#endif
static_assert(MPX_COL_TC >= 1 && MPX_COL_TC <= 64 && MPX_COL_TC * 64 <= 16 * 256,
              "MPX_COL_TC: FK runs on one thread per waypoint of a chunk and a thread holds at most 16 (waypoint, sphere) pairs");

enum { COL_NONE = 0, COL_GENERAL = 1, COL_WAVE = 2, COL_ENV = 3 };
struct CollisionRoute {
  int form;    // COL_*
  int ppt;     // wave / env: (waypoint, sphere) pairs per thread, the instantiation
  int block;   // workgroup size
  int tc;      // wave / env: waypoints per chunk
  int chunks;  // wave / env: chunks per environment; general: workgroups of the launch
  int last;    // (waypoint, sphere) pairs of the last chunk / of the last workgroup
};
// The flags-only call (min_sdf == NULL) takes the same route.  frames_aligned: both frame pointers are 16-byte aligned
// (the per-environment kernel stages the 4x4 frames as float4 rows; a tensor view with an odd storage offset takes the
// general kernel, which reads them with scalar loads).
inline CollisionRoute collision_route(int B, int T, int S, int M1, int M2, bool frames_aligned) {
  if (B == 0 || T == 0 || S == 0) return {COL_NONE, 0, 0, 0, 0, 0};
  if (M1 <= 64 && M2 <= 64 && S <= 64 && frames_aligned) {  // per-environment form: masks in two scalar words, pairs flattened over the lanes
    // (waypoints per workgroup, measured at 8192 x 50: 64 -> 0.486 ms, 32 -> 0.508, 16 -> 0.570; one- and two-wave
    // workgroups with 16 / 32 waypoints 0.735 / 0.673: FK runs once per chunk on as many lanes as the chunk has waypoints)
    // (round 4, pairs in registers: MPX_COL_TC waypoints x <= 64 spheres over 256 threads = MPX_COL_TC / 4 pairs per thread)
    const bool wave = T * S <= 64;  // one waypoint (the rollout step): one wave per environment, one pair per lane
    const int tc = wave ? 64 : MPX_COL_TC;
    const int chunks = cdiv(T, tc), last = (T - (chunks - 1) * tc) * S;
    if (wave) return {COL_WAVE, 1, 64, tc, chunks, last};
    const int sel = ((T < tc ? T : tc) * S + 511) / 512;  // packed pairs per thread of a full chunk
    return {COL_ENV, sel >= 1 && sel <= 7 ? 2 * sel : 16, 256, tc, chunks, last};
  }
  const int groups = cdiv((int64_t)B * T, COL_PPB);
  return {COL_GENERAL, 0, 256, 0, groups, (int)((int64_t)B * T - (int64_t)(groups - 1) * COL_PPB) * S};
}

// ---- mpx_linear / mpx_linear_ws (dense.hip) -----------------------------------------------------------------------------
constexpr int LINEAR_BM = 128, LINEAR_BN = 128;  // the tile of linear_kernel
// <= 8 rows whose padded copy fits 64 KB of LDS stream the weights once (gemv_kernel)
inline bool gemv_fits(int M, int K) { return M <= 8 && (int64_t)(M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : 8) * K * 4 <= 64 * 1024; }

enum { LINEAR_GEMV = 0, LINEAR_TILE = 1, LINEAR_SPLITK = 2 };
struct LinearRoute {
  int form;    // LINEAR_*
  int S;       // split-K: slices of K (else 1)
  int kslice;  // k per slice (else K)
};
// Split-K for skinny problems: a rollout of ONE problem (or a few hundred) leaves the fc / decoder layers with 1..32 output
// tiles: 4096->2048 at M <= 128 is 16 workgroups walking K = 4096 alone (310 us on 6 % of the CUs).  With a workspace the K
// range is cut into S slices (blockIdx.z), each writing a raw partial tile; splitk_reduce_kernel then adds the S partials
// IN SLICE ORDER (deterministic), the bias and the activation.  (The row-per-lane and DMA forms depend on the operands'
// addresses: dense.hip decides them.)
inline LinearRoute linear_route(int M, int N, int K) {
  if (gemv_fits(M, K)) return {LINEAR_GEMV, 1, K};
  const int64_t tiles = (int64_t)cdiv(M, LINEAR_BM) * cdiv(N, LINEAR_BN);
  // (M > 1024: the partial tiles would cost more HBM traffic than the idle CUs are worth)
  if (tiles >= 128 || K < 256 || M > 1024) return {LINEAR_TILE, 1, K};
  const int slabs = cdiv(K, 16);
  int S = (int)((512 + tiles - 1) / tiles);
  if (S > slabs / 4) S = slabs / 4;  // >= 64 k per slice
  if (S < 2) return {LINEAR_TILE, 1, K};
  const int kslice = cdiv(slabs, S) * 16;
  S = cdiv(K, kslice);
  return {S > 1 ? LINEAR_SPLITK : LINEAR_TILE, S, S > 1 ? kslice : K};
}

// ---- mpx_linear_wgrad (dense_grad.hip), mpx_pool_wgrad (train_ops.hip) --------------------------------------------------
constexpr int WG_BK = 16;  // rows per staged slab of linear_wgrad_kernel
constexpr int PB_KC = 64;  // columns of a wave's task in the sparse pool backward: one per lane
struct WgradRoute {
  int tile;            // 64 or 128: the instantiation
  int splits;          // partial sums over the rows (1: the kernel may write the gradient itself)
  int rows_per_split;  // a multiple of WG_BK
};
inline WgradRoute wgrad_route(int M, int N, int K) {
  const int T = (N <= 64 && K <= 64) ? 64 : 128;
  const int tiles = cdiv(N, T) * cdiv(K, T);
  int S = cdiv(1024, tiles);
  const int maxs = cdiv(M, 4 * WG_BK);
  S = S < 1 ? 1 : (S > maxs ? (maxs < 1 ? 1 : maxs) : S);
  return {T, S, cdiv(cdiv(M, S), WG_BK) * WG_BK};
}
inline int64_t pool_wgrad_splits(int64_t Q, int C, int K) {
  const int64_t blocks = (int64_t)cdiv(C, 64) * cdiv(K, PB_KC);
  int64_t S = cdiv((int64_t)4096, blocks);
  const int64_t maxs = cdiv(Q, (int64_t)8);  // >= 8 queries per split
  if (S > maxs) S = maxs;
  return S < 1 ? 1 : (S > 65535 ? 65535 : S);
}

// ---- the grouped-MLP launchers (sa_mlp.hip: fp32, sa_mlp_bf16.hip: bf16x3) ----------------------------------------------
constexpr int SA_MAX_NSAMPLE = 256;  // slots per neighbourhood the packed kernels index their row map for
// queries per unit of the large launches (A/B builds: narrow module 16 / 32: 10.38 / 10.14 ms -- the tail of a unit's last
// tile is 2.7 instead of 5.5 % of its rows; wide module 8 / 16: 46.6 / 46.8 ms -- its units are already 16 tiles)
constexpr int SA1_Q = 32, SA2_Q = 8;
constexpr int SA_BF16_WAVES = 8;   // lockstep kernel: waves per workgroup
constexpr int SA_BF16_RES_WV = 4;  // weight-resident kernel: waves per workgroup
constexpr int SA_BF16_V2_Q = 8;    // persistent factored kernel: queries per unit
// Which kernel serves mpx_sa_mlp_bf16x3: the weight-resident one for the first module (pack fits LDS) up to 128 slots
// per neighbourhood, the lockstep one otherwise.  ONE predicate for the launcher and for mpx_sa_mlp_bf16x3_wants_order.
inline bool bf16_uses_resident(int C, int c1, int c2, int c3, int nsample) {
  return C == 1 && c1 == 64 && c2 == 64 && c3 == 64 && nsample <= 128;
}

struct SaRoute {
  int packed;      // fp32: the packed kernel (hit counts honoured); 0: sa_mlp_kernel walks every slot
  int Q;           // queries per wave: the instantiation
  int lpool;       // fp32 narrow module: the form with the small row map that pools through LDS
  int64_t units;   // work units (fp32 packed, bf16x3 factored) or workgroups (the other forms) covering the queries
  int epx;         // > 0: whole environments per XCD -- units (fp32: bpe) / workgroups (bf16x3 resident: wpe) per environment
  int persistent;  // one workgroup per wave slot, units from the device-side queue (fp32: if the stream has a queue slot)
  int slots;       // grid of the persistent form
  int resident;    // bf16x3: the weight-resident kernel (else the lockstep one)
  int one_env;     // bf16x3 resident: a wave's queries share their environment
  int xcd_aware;   // bf16x3 factored: every XCD drains its own environments' units first
};
// cus: CUs of the device (the launchers pass mpx_cu_count()).  has_counts: the hit counts are given.  CF: feature channels
// of the module (1: the narrow (1+3, 64, 64, 64) one; else the wide (64+3, 128, 128, 256) one).  bf16x3 / factored: which
// entry point.  out_aligned: out_stride % 4 == 0 and `out` 16-byte aligned.
// fp32 packed plan: units of whole environments per XCD when the grid is regular (bpe; npoint % Q == 0, B % 8 == 0), and
// with many units per wave slot (per_cu one-wave workgroups per CU) the persistent form: one workgroup per slot -- a
// multiple of 8: the hardware deals workgroups to the XCDs round-robin -- and the units from the device-side queue.
inline SaRoute sa_route(int cus, int B, int npoint, int nsample, bool has_counts, int CF, bool bf16x3, bool factored,
                        bool out_aligned) {
  const int64_t nq = (int64_t)B * npoint;
  SaRoute r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (bf16x3 && factored) {  // ONE kernel: persistent, barrier-free, its own unit queue
    r.Q = SA_BF16_V2_Q, r.units = (nq + r.Q - 1) / r.Q, r.persistent = 1, r.slots = cus;
    r.xcd_aware = (B % 8 == 0 && cus % 8 == 0 && npoint % SA_BF16_V2_Q == 0) ? 1 : 0;
    return r;
  }
  if (bf16x3) {
    r.Q = CF == 1 ? 16 : 4;
    r.resident = CF == 1 && nsample <= 128;  // (bf16_uses_resident for the two modules the kernels are built for)
    const int64_t per_wg = (int64_t)(r.resident ? SA_BF16_RES_WV : SA_BF16_WAVES) * r.Q;
    r.units = (nq + per_wg - 1) / per_wg;
    if (r.resident) {
      r.epx = (npoint % per_wg == 0 && B % 8 == 0) ? (int)(npoint / per_wg) : 0;
      r.one_env = npoint % r.Q == 0;
    }
    return r;
  }
  r.packed = factored || (has_counts && nsample <= SA_MAX_NSAMPLE);  // (more slots than the row map holds: every slot is walked -- the same result)
  if (!r.packed) {
    r.Q = 1, r.units = (nq + 3) / 4;  // four one-query waves per workgroup
    return r;
  }
  // queries per wave: 8-16 tiles of work on typical scenes.  A small batch (a single planning problem up to a few
  // dozen) would leave most CUs idle at that size, so it runs fewer queries per wave instead: same rows, same
  // arithmetic per row (bit-identical results), 4x the waves and a quarter of the latency.
  if (factored) r.Q = nq >= 1024 * SA2_Q ? SA2_Q : nq >= 1024 ? 2 : 1;  // (a handful of problems: one query, 1-2 tiles, per wave)
  else if (CF == 1) r.Q = nq >= 1024 * SA1_Q ? SA1_Q : 4;
  else r.Q = nq >= 1024 * 8 ? 8 : 2;
  r.units = (nq + r.Q - 1) / r.Q;
  r.epx = (npoint % r.Q == 0 && B % 8 == 0) ? npoint / r.Q : 0;
  const int64_t slots = ((int64_t)cus * ((CF == 1 && !factored) ? 16 : 8)) & ~(int64_t)7;
  r.persistent = slots > 0 && r.units >= 4 * slots;
  r.slots = (int)slots;
  // (the narrow module with <= 128 slots per neighbourhood and 16-byte aligned output rows)
  r.lpool = !factored && CF == 1 && nsample <= 128 && out_aligned;
  return r;
}
