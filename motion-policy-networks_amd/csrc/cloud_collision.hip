// cloud_collision.hip -- swept-sphere collision check of Franka trajectories against one point cloud per environment.
//
// The primitive check (franka.hip: mpx_franka_collision) needs the scene as cuboids and cylinders.  The policy consumes
// a point cloud, and a depth cloud (depth.hip) or a captured cloud (the reference's ROS planner,
// interactive_demo/mpinets_ros/nodes/planning_node.py:78-151, plans from `obstacle_pc [4096,3]` alone) has no primitives
// behind it.  This file asks the same question of the cloud itself: does any of the robot's S spheres, at any waypoint,
// come within its radius of any point.
//
// Shape (franka_collision_env_kernel's): a workgroup owns ONE environment and a chunk of up to MPX_CLOUD_TC of its
// waypoints.  FK runs once per waypoint on the first lanes, frames parked in LDS; the (waypoint, sphere) pairs of the chunk
// are flattened over the lanes and a thread keeps all its pairs' centres (<= PPT) in registers.  The frames are dead
// from then on and the same LDS becomes a double-buffered tile of MPX_CLOUD_TILE points as 16-byte rows: while the
// workgroup walks tile k its threads hold tile k + 1 in registers (global loads in flight), one barrier per tile.
// The walk is point-outer, pair-inner: one broadcast ds_read_b128 (every lane the same address) feeds PPT independent
// chains of 3 subtractions + mpx_sqdist (1 multiply, 2 fma) + 1 v_min (flags only), or + compare and two selects when the
// nearest index is wanted.  N is unbounded (tiles loop), `counts` trims the walk.
//
// Pinned arithmetic (the contract in include/mpinets_hip.h): centres by franka_fk_frames + rigid_apply exactly as
// mpx_franka_spheres computes them; d2 = mpx_sqdist(c - p); R = (r_s + point_radius) + clearance, hit iff d2 <= R * R;
// best starts at +inf and moves only on d2 < best, points ascending.
//
// Flags-only form with the cull (MPX_VARIANT_CLOUD_CULL, default on): the workgroup first takes the axis-aligned box of
// its centres, inflated by more than the largest R (see `infl` below for why that is conservative in float32), and a
// point strictly outside the box on any axis is dropped while its tile is staged: the survivors of a tile are compacted
// into the LDS rows (ballot + prefix popcount within a wave, one LDS atomic per wave for its slot range -- their order
// does not matter to a minimum).  After each tile the workgroup stops if one of its pairs has hit.
#include "common.h"

constexpr int FRAME_FLOATS = MPX_NUM_FRAMES * 12;  // 180
constexpr int CC_TC = MPX_CLOUD_TC;                // waypoints per workgroup
constexpr int CC_TILE = MPX_CLOUD_TILE;            // points per LDS tile
static_assert(CC_TC >= 1 && CC_TC <= 64 && CC_TC * 64 <= 16 * 256,
              "MPX_CLOUD_TC: FK runs on one thread per waypoint and a thread holds at most 16 (waypoint, sphere) pairs");
static_assert(CC_TILE % 256 == 0, "MPX_CLOUD_TILE: whole rows of the largest workgroup");

template <int BLOCK, int PPT, bool FULL, bool CULL>
__global__ void __launch_bounds__(BLOCK)
    franka_cloud_collision_kernel(const float *__restrict__ q, int T, int chunks, float finger, const float *__restrict__ sc,
                                  const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                  const float *__restrict__ cloud, int64_t cbs, int cps, int N,
                                  const int32_t *__restrict__ counts, float point_radius, float clearance,
                                  int32_t *__restrict__ flags, float *__restrict__ min_dist, int32_t *__restrict__ nearest) {
  static_assert(!(FULL && CULL), "the full form visits every point");
  constexpr int NW = BLOCK / 64, ROWS = CC_TILE / BLOCK;  // waves; points a thread stages per tile
  constexpr int UNROLL = FULL ? 1 : 2;  // points per trip of the walk (what keeps 12 pairs per thread within 128 registers)
  extern __shared__ __attribute__((aligned(16))) float lds[];  // nt x FRAME_FLOATS, THEN 2 x CC_TILE rows of 4 floats
  __shared__ int cnt[3];        // CULL: survivors of tile k in cnt[k % 3]
  __shared__ float red[NW][8];  // CULL: per-wave box of the centres
  float4 *tile = reinterpret_cast<float4 *>(lds);
  const int b = blockIdx.x / chunks, t0 = (blockIdx.x - b * chunks) * CC_TC;  // (block-uniform)
  const int nt = min(CC_TC, T - t0);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  if (tid < nt) {
    float qq[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) qq[j] = q[((size_t)b * T + t0 + tid) * 7 + j];
    franka_fk_frames(qq, finger, lds + tid * FRAME_FLOATS);
  }
  if (CULL && tid < 3) cnt[tid] = 0;
  __syncthreads();
  // pairs of this thread: p = tid + k * BLOCK, k < PPT (the launcher picks PPT for a full chunk; pairs past the end repeat
  // pair 0 -- a real pair of this environment, so its hits are real -- and are not stored)
  const int npairs = nt * S;
  float cx[PPT], cy[PPT], cz[PPT], best[PPT], R2[PPT];
  int idx[FULL ? PPT : 1];
  float bx0 = __builtin_inff(), by0 = bx0, bz0 = bx0, bx1 = -bx0, by1 = -bx0, bz1 = -bx0, amax = 0.0f, rmax = 0.0f;
  {
    const int dq = BLOCK / S, dr = BLOCK - dq * S;  // a step of BLOCK pairs = dq waypoints + dr spheres
    int tt = tid / S, ss = tid - tt * S;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const bool on = tid + k * BLOCK < npairs;
      const int t1 = on ? tt : 0, s1 = on ? ss : 0;
      rigid_apply(lds + t1 * FRAME_FLOATS + 12 * sl[s1], sc[3 * s1 + 0], sc[3 * s1 + 1], sc[3 * s1 + 2], cx[k], cy[k], cz[k]);
      const float R = (sr[s1] + point_radius) + clearance;
      R2[k] = R * R;
      best[k] = __builtin_inff();
      if constexpr (FULL) idx[k] = -1;
      if (CULL) {
        bx0 = fminf(bx0, cx[k]), by0 = fminf(by0, cy[k]), bz0 = fminf(bz0, cz[k]);
        bx1 = fmaxf(bx1, cx[k]), by1 = fmaxf(by1, cy[k]), bz1 = fmaxf(bz1, cz[k]);
        amax = fmaxf(amax, fmaxf(fabsf(cx[k]), fmaxf(fabsf(cy[k]), fabsf(cz[k]))));
        rmax = fmaxf(rmax, fabsf(R));
      }
      tt += dq, ss += dr;
      if (ss >= S) ss -= S, ++tt;
      // (one pair at a time: left alone the compiler issues the frame reads of ALL pairs first and finishes their
      // products afterwards, 12 registers per pair, and that peak -- not the walk below -- sets the kernel's register
      // count and its waves per SIMD.  The empty asm pins the finished centre here, the fence keeps the scheduler from
      // undoing it.)
      asm volatile("" : "+v"(cx[k]), "+v"(cy[k]), "+v"(cz[k]));
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (CULL) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      bx0 = fminf(bx0, __shfl_xor(bx0, o)), by0 = fminf(by0, __shfl_xor(by0, o)), bz0 = fminf(bz0, __shfl_xor(bz0, o));
      bx1 = fmaxf(bx1, __shfl_xor(bx1, o)), by1 = fmaxf(by1, __shfl_xor(by1, o)), bz1 = fmaxf(bz1, __shfl_xor(bz1, o));
      amax = fmaxf(amax, __shfl_xor(amax, o)), rmax = fmaxf(rmax, __shfl_xor(rmax, o));
    }
    if (lane == 0) {
      float *r = red[tid >> 6];
      r[0] = bx0, r[1] = by0, r[2] = bz0, r[3] = bx1, r[4] = by1, r[5] = bz1, r[6] = amax, r[7] = rmax;
    }
  }
  __syncthreads();  // every centre is in registers: the frames' LDS is free for the tiles (and `red` is complete)
  if (CULL) {
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float *r = red[w];
      bx0 = fminf(bx0, r[0]), by0 = fminf(by0, r[1]), bz0 = fminf(bz0, r[2]);
      bx1 = fmaxf(bx1, r[3]), by1 = fmaxf(by1, r[4]), bz1 = fmaxf(bz1, r[5]);
      amax = fmaxf(amax, r[6]), rmax = fmaxf(rmax, r[7]);
    }
    // A point with p.x < lo = fl(min c.x - infl) is dropped.  Then for every centre c.x - p.x > min c.x - lo >= infl -
    // 2^-24 (amax + infl) > rmax (1 + 1e-5): the relative part of `infl` covers R, its second part is 16 x the rounding of
    // `lo` itself.  The device's dx = fl(c.x - p.x) >= rmax (1 + 1e-5)(1 - 2^-24), and mpx_sqdist is monotone in |dx| with
    // non-negative other terms, so d2 >= fl(dx dx) >= rmax^2 (1 + 1e-5)^2 (1 - 2^-24)^3 > rmax^2 (1 + 2^-24) >= fl(R R) for
    // every |R| <= rmax: no dropped point can hit.  (1e-12: keeps dx dx a normal number when rmax and amax are 0.)  The
    // same on the other five faces.  A NaN bound keeps every point (the comparisons below are false).
    const float infl = (rmax * 1.00001f + 1e-6f * (amax + rmax)) + 1e-12f;
    bx0 -= infl, by0 -= infl, bz0 -= infl, bx1 += infl, by1 += infl, bz1 += infl;
  }
  int n = N;
  if (counts) n = min(max(counts[b], 0), N);
  const int ntiles = (n + CC_TILE - 1) / CC_TILE;
  const float *cb = cloud + (int64_t)b * cbs;
  float px[ROWS], py[ROWS], pz[ROWS];
  auto fetch = [&](int k) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int i = k * CC_TILE + r * BLOCK + tid;
      px[r] = py[r] = pz[r] = 0.0f;
      if (i < n) {
        const float *p = cb + (int64_t)i * cps;
        px[r] = p[0], py[r] = p[1], pz[r] = p[2];
      }
    }
  };
  auto stage = [&](int k) __attribute__((always_inline)) {
    float4 *dst = tile + (k & 1) * CC_TILE;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const bool ok = k * CC_TILE + r * BLOCK + tid < n;
      if (!CULL) {
        if (ok) dst[r * BLOCK + tid] = make_float4(px[r], py[r], pz[r], 0.0f);
      } else {
        const bool keep = ok && !(px[r] < bx0 || px[r] > bx1 || py[r] < by0 || py[r] > by1 || pz[r] < bz0 || pz[r] > bz1);
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
        int slot = 0;
        if (lane == 0 && mask) slot = atomicAdd(&cnt[k % 3], __builtin_popcountll(mask));
        slot = __builtin_amdgcn_readfirstlane(slot);
        if (keep) dst[slot + __builtin_popcountll(mask & (((unsigned long long)1 << lane) - 1))] = make_float4(px[r], py[r], pz[r], 0.0f);
      }
    }
  };
  auto any_hit = [&]() __attribute__((always_inline)) {
    bool h = false;
#pragma unroll
    for (int k = 0; k < PPT; ++k) h |= (best[k] <= R2[k]) & (best[k] < __builtin_inff());  // (R = +inf: still no hit without a point)
    return h;
  };
  if (ntiles > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  for (int k = 0; k < ntiles; ++k) {
    if (k + 1 < ntiles) fetch(k + 1);
    // (slot k + 2's counter: last read while tile k - 1 was walked, next added to after this tile's barrier)
    if (CULL && tid == 0) cnt[(k + 2) % 3] = 0;
    const int m = CULL ? __builtin_amdgcn_readfirstlane(cnt[k % 3]) : min(CC_TILE, n - k * CC_TILE);
    const float4 *src = tile + (k & 1) * CC_TILE;
    const int base = k * CC_TILE;
#pragma unroll UNROLL
    for (int j = 0; j < m; ++j) {
      const float4 p = src[j];
#pragma unroll
      for (int u = 0; u < PPT; ++u) {
        const float d2 = mpx_sqdist(cx[u] - p.x, cy[u] - p.y, cz[u] - p.z);
        if constexpr (FULL) {
          const bool nearer = d2 < best[u];
          best[u] = nearer ? d2 : best[u];
          idx[u] = nearer ? base + j : idx[u];
        } else {
          best[u] = fminf(best[u], d2);  // (= the strict compare-and-keep: best is never NaN, a NaN d2 is dropped)
        }
      }
    }
    if (k + 1 < ntiles) stage(k + 1);
    if (CULL) {
      if (__syncthreads_or(any_hit())) break;
    } else {
      __syncthreads();
    }
  }
  bool hit = false;
  if constexpr (FULL) {
    const int dq = BLOCK / S, dr = BLOCK - dq * S;
    int tt = tid / S, ss = tid - tt * S;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      if (tid + k * BLOCK < npairs) {
        const size_t o = ((size_t)b * T + t0 + tt) * S + ss;
        if (min_dist) min_dist[o] = sqrtf(best[k]) - point_radius;
        if (nearest) nearest[o] = idx[k];
        hit |= (best[k] <= R2[k]) & (idx[k] >= 0);
      }
      tt += dq, ss += dr;
      if (ss >= S) ss -= S, ++tt;
    }
  } else {
    hit = any_hit();
  }
  if (__any(hit) && lane == 0) atomicOr(flags + b, 1);
}

MPX_EXPORT int mpx_franka_cloud_collision(const float *q, int B, int T, float finger, const float *sph_centers,
                                          const float *sph_radii, const int32_t *sph_link, int S, const float *cloud,
                                          int64_t cloud_batch_stride, int cloud_point_stride, int N, const int32_t *counts,
                                          float point_radius, float clearance, int32_t *flags, float *min_dist,
                                          int32_t *nearest, mpx_stream_t stream) {
  MPX_REQUIRE(B >= 0 && T >= 0 && S >= 0 && N >= 0, "mpx_franka_cloud_collision: negative size");
  MPX_REQUIRE(S <= 64, "mpx_franka_cloud_collision: S = %d spheres, at most 64", S);
  MPX_REQUIRE(point_radius >= 0.0f, "mpx_franka_cloud_collision: point_radius must be >= 0");
  MPX_REQUIRE(clearance == clearance, "mpx_franka_cloud_collision: clearance is NaN");
  MPX_REQUIRE(cloud_point_stride >= 3, "mpx_franka_cloud_collision: cloud_point_stride < 3");
  MPX_REQUIRE((int64_t)B * T < (int64_t)1 << 31, "mpx_franka_cloud_collision: B*T overflows int32");
  if (B == 0 || T == 0 || S == 0) return 0;
  const bool full = min_dist != nullptr || nearest != nullptr;
  if (N == 0 && !full) return 0;  // no point, no hit
  MPX_REQUIRE(q && sph_centers && sph_radii && sph_link && flags && (cloud || N == 0), "mpx_franka_cloud_collision: NULL operand");
  const int chunks = cdiv(T, CC_TC);
  MPX_REQUIRE((int64_t)B * chunks < (int64_t)1 << 31, "mpx_franka_cloud_collision: too many workgroups");
  const bool cull = !full && mpx_get_variant(MPX_VARIANT_CLOUD_CULL) != 0;
  const int nt = min(T, CC_TC);
  const size_t lds_bytes = sizeof(float) * (size_t)max(nt * FRAME_FLOATS, 2 * CC_TILE * 4);
#define CLOUD_LAUNCH(BLOCK, PPT, FULL, CULL)                                                                            \
  hipLaunchKernelGGL((franka_cloud_collision_kernel<BLOCK, PPT, FULL, CULL>), dim3((unsigned)(B * chunks)), dim3(BLOCK), \
                     lds_bytes, mpx_s(stream), q, T, chunks, finger, sph_centers, sph_radii, sph_link, S, cloud,        \
                     cloud_batch_stride, cloud_point_stride, N, counts, point_radius, clearance, flags, min_dist, nearest)
#define CLOUD_FORM(BLOCK, PPT)                       \
  do {                                               \
    if (full) CLOUD_LAUNCH(BLOCK, PPT, true, false); \
    else if (cull) CLOUD_LAUNCH(BLOCK, PPT, false, true); \
    else CLOUD_LAUNCH(BLOCK, PPT, false, false);     \
  } while (0)
  if (nt * S <= 64) CLOUD_FORM(64, 1);  // one waypoint (a configuration, the rollout step): one wave, one pair per lane
  else {
    switch ((nt * S + 511) / 512) {  // pairs per thread of a full chunk over 256 threads, rounded up to even
      case 1: CLOUD_FORM(256, 2); break;
      case 2: CLOUD_FORM(256, 4); break;
      case 3: CLOUD_FORM(256, 6); break;
      case 4: CLOUD_FORM(256, 8); break;
      case 5: CLOUD_FORM(256, 10); break;
      case 6: CLOUD_FORM(256, 12); break;
      case 7: CLOUD_FORM(256, 14); break;
      default: CLOUD_FORM(256, 16); break;
    }
  }
#undef CLOUD_FORM
#undef CLOUD_LAUNCH
  MPX_LAUNCH_CHECK("mpx_franka_cloud_collision");
}
