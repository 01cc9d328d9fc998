// cloud_collision_walk.inc -- the body of the kernels of cloud_collision.hip: the one walk of a point cloud, included by
// text so that both kernels are compiled from the same statements and the flag kernels' instruction streams do not depend
// on the per-waypoint form's existence.  Expects, in scope: the constants BLOCK, PPT, FULL, CULL, EACH and the operands
//   q, T, chunks, finger, sc, sr, sl, S, cloud, cbs, cps, N, counts, point_radius, clearance   (both forms)
//   flags, min_dist, nearest   (EACH = false: flags [B] OR-ed into, the other two written when FULL)
//   active, hit_out            (EACH = true: hit_out [B,T] written, `active` optional)
  static_assert(!(FULL && CULL), "the full form visits every point");
  static_assert(!(FULL && EACH), "the per-waypoint form returns verdicts only");
  constexpr int NW = BLOCK / 64, ROWS = CC_TILE / BLOCK;  // waves; points a thread stages per tile
  constexpr int UNROLL = FULL ? 1 : 2;  // points per trip of the walk (what keeps 12 pairs per thread within 128 registers)
  extern __shared__ __attribute__((aligned(16))) float lds[];  // nt x FRAME_FLOATS, THEN 2 x CC_TILE rows of 4 floats
  __shared__ int cnt[3];        // CULL: survivors of tile k in cnt[k % 3]
  __shared__ float red[NW][8];  // CULL: per-wave box of the centres
  float4 *tile = reinterpret_cast<float4 *>(lds);
  const int b = blockIdx.x / chunks, t0 = (blockIdx.x - b * chunks) * CC_TC;  // (block-uniform)
  const int nt = min(CC_TC, T - t0);
  const int tid = (int)threadIdx.x, lane = tid & 63;
  __shared__ unsigned long long each_mask[EACH ? 3 : 1];  // EACH: hits of the chunk's waypoints (two slots), [2] = active
  bool act = true;
  if constexpr (EACH) act = tid < nt && (active == nullptr || active[(size_t)b * T + t0 + tid] != 0);
  if (tid < nt && act) {
    float qq[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) qq[j] = q[((size_t)b * T + t0 + tid) * 7 + j];
    franka_fk_frames(qq, finger, lds + tid * FRAME_FLOATS);
  }
  if (CULL && tid < 3) cnt[tid] = 0;
  if constexpr (EACH) {
    if (tid < 64) {  // (wave 0 holds every waypoint of the chunk: nt <= 64)
      const unsigned long long m = __builtin_amdgcn_ballot_w64(act);
      if (tid == 0) each_mask[0] = 0, each_mask[1] = 0, each_mask[2] = m;
    }
  }
  __syncthreads();
  [[maybe_unused]] unsigned long long amask = 0;  // EACH: the chunk's active waypoints (block-uniform)
  int tfirst = 0;                // what padding and replaced pairs repeat: a real, tested pair
  if constexpr (EACH) {
    amask = each_mask[2];
    if (amask == 0) {  // nothing to test: zeros, and no walk
      if (tid < nt) hit_out[(size_t)b * T + t0 + tid] = 0;
      return;
    }
    tfirst = (int)__builtin_ctzll(amask);
  }
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
      bool on = tid + k * BLOCK < npairs;
      if constexpr (EACH) on = on && ((amask >> (tt & 63)) & 1) != 0;
      const int t1 = on ? tt : tfirst, s1 = on ? ss : 0;
      rigid_apply(lds + t1 * FRAME_FLOATS + 12 * sl[s1], sc[3 * s1 + 0], sc[3 * s1 + 1], sc[3 * s1 + 2], cx[k], cy[k], cz[k]);
      const float R = (sr[s1] + point_radius) + clearance;
      R2[k] = R * R;
      if constexpr (EACH) R2[k] = on ? R2[k] : -1.0f;  // (padding and replaced pairs: no d2 is <= -1)
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
  // EACH: this thread's pairs that have hit, as a mask of their waypoints (padding and replaced pairs left out)
  auto each_hits = [&]() __attribute__((always_inline)) {
    unsigned long long m = 0;
    int t = tid;
    asm volatile("" : "+v"(t));  // (the pair -> waypoint walk is redone here: hoisted out of the tile loop, its PPT shifted
                                 // masks would stay live across the walk, two registers per pair)
    const int dq = BLOCK / S, dr = BLOCK - dq * S;
    int tt = t / S, ss = t - tt * S;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const bool h = (best[k] <= R2[k]) & (best[k] < __builtin_inff());
      m |= h ? (unsigned long long)1 << (tt & 63) : 0;
      tt += dq, ss += dr;
      if (ss >= S) ss -= S, ++tt;
    }
    return m & amask;
  };
  [[maybe_unused]] int slot = 0;  // EACH: which of the two masks holds the verdicts when the walk ends
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
    if constexpr (EACH && CULL) {
      slot = k & 1;
      const unsigned long long m = each_hits();
      if (m) atomicOr(&each_mask[slot], m);
      __syncthreads();  // (each_mask[slot] is next written after tile k + 2, behind the barrier of tile k + 1)
      if (each_mask[slot] == amask) break;  // every active waypoint of the chunk has a hit (block-uniform)
    } else if (CULL) {
      if (__syncthreads_or(any_hit())) break;
    } else {
      __syncthreads();
    }
  }
  if constexpr (EACH) {
    if constexpr (!CULL) {
      const unsigned long long m = each_hits();
      if (m) atomicOr(&each_mask[0], m);
      __syncthreads();
    }
    if (tid < nt) hit_out[(size_t)b * T + t0 + tid] = (int32_t)((each_mask[slot] >> tid) & 1);
    return;
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
