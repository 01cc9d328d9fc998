// cloud_clean.hip -- the first stage of the captured-cloud path: crop, robot removal, outlier removal and the draw.
//
// The reference's real-robot planner (interactive_demo/mpinets_ros/nodes/planning_node.py:78-151) asserts that its caller
// has reduced the capture to [4096, 3] ("You must downsample obstacle PC before passing to planner.  While you're at it,
// filter the outliers out as well"); its own clean_point_cloud (:187-228) crops to two workspace boxes and draws with
// np.random.choice, on the host.  Here a batch of captures [B, N, 3 or 4] is cleaned on the device (the contract is in
// include/mpinets_hip.h): every row gets the first stage it fails as its `reason`,
//   1 non-existent / non-finite, 2 outside every crop box, 3 inside a robot sphere, 4 too few neighbours within a radius,
// and n_out of the rows with reason 0 are drawn by Philox keys through mpx_select_smallest (select_device.h).
//
// Launches, all on the caller's stream, scratch caller-owned:
//   classify   one thread per row, boxes and spheres in LDS: stages 1-3.  Streams N * 12 bytes, writes N reasons.  With
//              no crop box it also reduces the box of the surviving rows (`alive1`): per wave in registers, then six
//              integer atomicMax on order-preserving bits per wave.
//   --- only when min_neighbors > 0 ---
//   grid       one workgroup per environment: a uniform grid over the crop boxes' bounding box (or alive1's box) with a
//              cell edge >= 1.01 r on every axis, so the neighbours of a row lie in the 27 cells around it; at most
//              CLEAN_AXIS cells per axis and MPX_CLEAN_MAX_CELLS per environment (the edges grow until that holds: a
//              far-away point makes cells coarse, never wrong).  Zeroes the cell counters it will use.
//   bin<0>     per alive1 row: atomicAdd(cell counter, 1)
//   scan       one workgroup per environment: exclusive scan of the counters, 4096 cells per trip
//   bin<1>     per alive1 row: slot = atomicAdd(cell cursor, 1); packed[slot] = {x, y, z, row}.  The cursor of cell c ends
//              as the END of c's run (= the start of c + 1's).  The order inside a run depends on how the atomics land;
//              the neighbour COUNT does not.
//   neighbours one thread per packed row: x is the fastest cell axis, so the three cells (cx - 1 .. cx + 1) of a (cy, cz)
//              are one contiguous run of 16-byte rows; nine runs per row (their eighteen bounds are loaded first), walked
//              from the row's own run outwards until min_neighbors are found.
//   Survivors are counted with one integer atomicAdd per workgroup (profiles/cloud_clean_timing.md: one per wave on a
//   single counter per environment cost more than the whole classify pass).
//   --- only when n_out > 0 ---
//   draw       one workgroup per environment, as depth.hip's select: keys by Philox stream 15, gather by source row.
//
// Why 1.01: a pair counts when fma(dz,dz, fma(dx,dx, dy*dy)) <= fl(r * r) with float32 differences, which bounds the real
// |dx| by r (1 + 1e-6).  A cell coordinate is floor(fl(fl(p - lo) * fl(1 / h))), monotone in p, with fl(p - lo) * (1 / h) <=
// 1000 (1 + 1e-6) inside the domain, so its rounding error is below 2e-4 cells; two rows at most r (1 + 1e-6) apart are at
// most 0.9902 + 4e-4 < 1 apart in that coordinate and their cells differ by at most one.  Clamping into [0, n - 1] is
// monotone and keeps that; it is also what keeps every index in range whatever the coordinates are.
#include "common.h"
#include "franka_host.h"
#include "philox.h"
#include "select_device.h"

enum { STREAM_CAPTURE = 15 };

constexpr int CLEAN_CELLS = MPX_CLEAN_MAX_CELLS;  // cell counters per environment
constexpr int CLEAN_AXIS = 1000;                  // cells per axis (a coordinate below 2^10 keeps 13 fraction bits)
constexpr int CLEAN_SCAN = 4096;                  // cells per trip of the scan: 1024 threads x 4
static_assert(CLEAN_CELLS % CLEAN_SCAN == 0 && CLEAN_CELLS >= CLEAN_SCAN, "MPX_CLEAN_MAX_CELLS: whole scan trips");
static_assert(MPX_CLEAN_MAX_BOXES * 6 <= 64 && MPX_CLEAN_MAX_SPHERES <= 64, "boxes and spheres are staged by the first wave");

struct CleanGrid {  // one per environment at the head of the scratch, zeroed by the launcher
  unsigned bb[6];   // no crop box: order-preserving bits of alive1's box, [0..2] = ~min, [3..5] = max (0 = no row yet)
  int n_alive1;     // rows that passed stages 1-3
  int nx, ny, nz;
  float lo[3], ih[3];  // cell = clamp(floor((p - lo) * ih), 0, n - 1)
};
static_assert(sizeof(CleanGrid) == 64, "CleanGrid: one 64-byte record per environment");

struct CleanLayout {
  size_t cells, packed, reason, total, np;
};
static CleanLayout clean_layout(int B, int N) {
  CleanLayout L;
  L.np = ((size_t)N + 15) & ~(size_t)15;
  L.cells = ((size_t)B * sizeof(CleanGrid) + 255) & ~(size_t)255;
  L.packed = L.cells + (size_t)B * CLEAN_CELLS * sizeof(int);
  L.reason = L.packed + (size_t)B * L.np * sizeof(float4);
  L.total = L.reason + (size_t)B * L.np;
  return L;
}

__device__ __forceinline__ int clean_axis_cell(float p, float lo, float ih, int n) {
  // (fmaxf drops a NaN: a degenerate axis lands in cell 0)
  return (int)fminf(fmaxf(floorf((p - lo) * ih), 0.0f), (float)(n - 1));
}
__device__ __forceinline__ int clean_cell(const CleanGrid &g, float x, float y, float z, int &cx, int &cy, int &cz) {
  cx = clean_axis_cell(x, g.lo[0], g.ih[0], g.nx);
  cy = clean_axis_cell(y, g.lo[1], g.ih[1], g.ny);
  cz = clean_axis_cell(z, g.lo[2], g.ih[2], g.nz);
  return (cz * g.ny + cy) * g.nx + cx;
}

__global__ void __launch_bounds__(256)
    clean_classify_kernel(const float *__restrict__ cloud, int64_t cbs, int cps, int N, const int32_t *__restrict__ counts,
                          const float *__restrict__ boxes, int n_boxes, const float *__restrict__ sc,
                          const float *__restrict__ sr, int S, float margin, int stage4, uint8_t *__restrict__ rs,
                          CleanGrid *__restrict__ grid, int32_t *__restrict__ count) {
  __shared__ float bx[MPX_CLEAN_MAX_BOXES * 6];
  __shared__ float4 sp[MPX_CLEAN_MAX_SPHERES];
  const int b = blockIdx.y, tid = (int)threadIdx.x;
  if (tid < n_boxes * 6) bx[tid] = boxes[tid];
  if (tid < S) {
    const float *c = sc + ((size_t)b * S + tid) * 3;
    const float R = sr[tid] + margin;
    sp[tid] = make_float4(c[0], c[1], c[2], R * R);
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + tid;
  int n = N;
  if (counts) n = min(max(counts[b], 0), N);
  const float inf = __builtin_inff();
  float x = 0.0f, y = 0.0f, z = 0.0f;
  int reason = 1;
  if (i < n) {
    const float *p = cloud + (int64_t)b * cbs + (int64_t)i * cps;
    x = p[0], y = p[1], z = p[2];
    if (fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf) {
      reason = 0;
      if (n_boxes > 0) {
        bool in = false;
        for (int j = 0; j < n_boxes; ++j) {
          const float *q = bx + 6 * j;
          in |= q[0] < x && x < q[3] && q[1] < y && y < q[4] && q[2] < z && z < q[5];
        }
        if (!in) reason = 2;
      }
      if (reason == 0) {
        bool hit = false;
        for (int s = 0; s < S; ++s) {
          const float4 c = sp[s];
          hit |= mpx_sqdist(x - c.x, y - c.y, z - c.z) <= c.w;
        }
        if (hit) reason = 3;
      }
    }
  }
  if (i < N) rs[(size_t)b * N + i] = (uint8_t)reason;
  const bool alive = reason == 0;
  // (one atomic per workgroup: a 640 x 480 frame would otherwise queue 5000 wave-level adds on one address)
  const int alive_here = __syncthreads_count(alive);
  if (tid == 0 && alive_here > 0) atomicAdd(stage4 ? &grid[b].n_alive1 : count + b, alive_here);
  if (stage4 && n_boxes == 0 && __any(alive)) {  // (wave-uniform branch)
    float lo[3] = {alive ? x : inf, alive ? y : inf, alive ? z : inf};
    float hi[3] = {alive ? x : -inf, alive ? y : -inf, alive ? z : -inf};
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], __shfl_xor(lo[a], o)), hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
    if ((tid & 63) == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMax(&grid[b].bb[a], ~mpx_ordered_bits(lo[a]));
        atomicMax(&grid[b].bb[3 + a], mpx_ordered_bits(hi[a]));
      }
    }
  }
}

// One workgroup per environment: the grid of this call, then zeroes for the counters the scan will read.
__global__ void __launch_bounds__(256)
    clean_grid_kernel(CleanGrid *__restrict__ grid, const float *__restrict__ boxes, int n_boxes, float r,
                      int *__restrict__ cells) {
  __shared__ int ncell;
  const int b = blockIdx.x, tid = (int)threadIdx.x;
  if (tid == 0) {
    CleanGrid g = grid[b];
    const float inf = __builtin_inff();
    float lo[3] = {0.0f, 0.0f, 0.0f}, ext[3] = {0.0f, 0.0f, 0.0f};
    if (n_boxes > 0 || g.n_alive1 > 0) {
      for (int a = 0; a < 3; ++a) {
        float l = inf, h = -inf;
        for (int j = 0; j < n_boxes; ++j) l = fminf(l, boxes[6 * j + a]), h = fmaxf(h, boxes[6 * j + 3 + a]);
        if (n_boxes == 0) l = mpx_ordered_float(~g.bb[a]), h = mpx_ordered_float(g.bb[3 + a]);
        const float e = h - l;
        if (fabsf(l) < inf && e >= 0.0f && e < inf) lo[a] = l, ext[a] = e;  // (anything else: one cell on this axis)
      }
    }
    float h[3];
    int n[3];
    for (int a = 0; a < 3; ++a) h[a] = fmaxf(r * 1.01f, ext[a] / (float)CLEAN_AXIS);
    for (int trip = 0; trip < 256; ++trip) {
      for (int a = 0; a < 3; ++a) {
        const float cells_f = ext[a] / h[a];  // <= CLEAN_AXIS; NaN (0 / 0, inf / inf) -> one cell
        n[a] = cells_f < (float)CLEAN_AXIS ? (int)cells_f + 1 : CLEAN_AXIS + 1;
        if (!(cells_f >= 0.0f)) n[a] = 1;
      }
      if ((long long)n[0] * n[1] * n[2] <= (long long)CLEAN_CELLS) break;
      for (int a = 0; a < 3; ++a) h[a] *= 1.26f;  // (halves the cell count; every axis reaches one cell long before 256 trips)
    }
    if ((long long)n[0] * n[1] * n[2] > (long long)CLEAN_CELLS) n[0] = n[1] = n[2] = 1;
    for (int a = 0; a < 3; ++a) {
      float ih = 1.0f / h[a];
      if (n[a] == 1 || !(ih < inf)) ih = 0.0f, n[a] = 1;
      g.lo[a] = lo[a], g.ih[a] = ih;
    }
    g.nx = n[0], g.ny = n[1], g.nz = n[2];
    grid[b] = g;
    ncell = (g.nx * g.ny * g.nz + CLEAN_SCAN - 1) / CLEAN_SCAN * CLEAN_SCAN;  // <= CLEAN_CELLS
  }
  __syncthreads();
  int4 *cb = reinterpret_cast<int4 *>(cells + (size_t)b * CLEAN_CELLS);
  for (int i = tid; 4 * i < ncell; i += 256) cb[i] = make_int4(0, 0, 0, 0);
}

// SCATTER = false: count the alive1 rows of every cell.  true: place them (cells holds the exclusive scan of the counts).
template <bool SCATTER>
__global__ void __launch_bounds__(256)
    clean_bin_kernel(const float *__restrict__ cloud, int64_t cbs, int cps, int N, const uint8_t *__restrict__ rs,
                     const CleanGrid *__restrict__ grid, int *__restrict__ cells, float4 *__restrict__ packed, size_t np) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= N || rs[(size_t)b * N + i] != 0) return;  // (rows past counts[b] carry reason 1)
  const CleanGrid g = grid[b];
  const float *p = cloud + (int64_t)b * cbs + (int64_t)i * cps;
  const float x = p[0], y = p[1], z = p[2];
  int cx, cy, cz;
  int *c = cells + (size_t)b * CLEAN_CELLS + clean_cell(g, x, y, z, cx, cy, cz);
  if (!SCATTER) {
    atomicAdd(c, 1);
  } else {
    const int at = atomicAdd(c, 1);
    if ((unsigned)at < (unsigned)N) packed[(size_t)b * np + at] = make_float4(x, y, z, __int_as_float(i));
  }
}

__global__ void __launch_bounds__(1024) clean_scan_kernel(const CleanGrid *__restrict__ grid, int *__restrict__ cells) {
  __shared__ int ws[16];
  const int b = blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncell = (grid[b].nx * grid[b].ny * grid[b].nz + CLEAN_SCAN - 1) / CLEAN_SCAN * CLEAN_SCAN;
  int4 *cb = reinterpret_cast<int4 *>(cells + (size_t)b * CLEAN_CELLS);
  int carry = 0;
  for (int t0 = 0; t0 < ncell; t0 += CLEAN_SCAN) {
    const int4 v = cb[(t0 >> 2) + tid];
    const int s = v.x + v.y + v.z + v.w;
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int t = ws[w];
      base += w < wave ? t : 0;
      tot += t;
    }
    const int e = carry + base + inc - s;
    cb[(t0 >> 2) + tid] = make_int4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
    carry += tot;
    __syncthreads();  // ws is rewritten by the next trip
  }
}

__global__ void __launch_bounds__(256)
    clean_neighbors_kernel(const float4 *__restrict__ packed, size_t np, const CleanGrid *__restrict__ grid,
                           const int *__restrict__ cells, float r2, int need, uint8_t *__restrict__ rs, int N,
                           int32_t *__restrict__ count) {
  const int b = blockIdx.y, tid = (int)threadIdx.x, k = blockIdx.x * 256 + tid;
  const CleanGrid g = grid[b];
  const int n1 = min(g.n_alive1, N);
  const float4 *pk = packed + (size_t)b * np;
  const int *ce = cells + (size_t)b * CLEAN_CELLS;  // ce[c] = end of cell c's run, its start = ce[c - 1]
  bool kept = false;
  if (k < n1) {
    const float4 me = pk[k];
    int cx, cy, cz;
    clean_cell(g, me.x, me.y, me.z, cx, cy, cz);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.nx - 1);
    // the bounds of all nine runs first (eighteen independent loads), then the walk
    int start[9], end[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int z = cz + t / 3 - 1, y = cy + t % 3 - 1;
      start[t] = end[t] = 0;
      if (z >= 0 && z < g.nz && y >= 0 && y < g.ny) {
        const int row = (z * g.ny + y) * g.nx;
        const int first = row + x0, last = row + x1;
        start[t] = first > 0 ? max(ce[first - 1], 0) : 0;
        end[t] = min(ce[last], n1);
      }
    }
    int found = 0;
    constexpr int ORDER[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};  // the row's own run first: that is where most neighbours are
#pragma unroll
    for (int o = 0; o < 9; ++o) {
      const int t = ORDER[o];
      for (int j = start[t]; j < end[t] && found < need; ++j) {
        const float4 q = pk[j];
        found += (mpx_sqdist(me.x - q.x, me.y - q.y, me.z - q.z) <= r2) & (j != k);
      }
    }
    kept = found >= need;
    const int i = __float_as_int(me.w);
    if (!kept && (unsigned)i < (unsigned)N) rs[(size_t)b * N + i] = 4;
  }
  const int kept_here = __syncthreads_count(kept);
  if (tid == 0 && kept_here > 0) atomicAdd(count + b, kept_here);
}

// One workgroup per environment: n_out of the rows with reason 0 (smallest Philox keys; ties by row) in key order.
__global__ void __launch_bounds__(SEL_THREADS)
    clean_draw_kernel(const float *__restrict__ cloud, int64_t cbs, int cps, int N, const int32_t *__restrict__ counts,
                      const uint8_t *__restrict__ rs, int n_out, uint32_t k0, uint32_t k1, uint32_t env0,
                      float *__restrict__ out, int64_t obs, int ops, int32_t *__restrict__ src_index) {
  __shared__ unsigned long long sel[SEL_CAP];
  __shared__ int hist[2048];
  __shared__ int s3[3];
  const int b = blockIdx.x, tid = (int)threadIdx.x;
  int n = N;
  if (counts) n = min(max(counts[b], 0), N);
  const uint8_t *rb = rs + (size_t)b * N;
  const int valid = mpx_select_smallest(
      n, n_out,
      [&](int g, uint32_t (&key)[4], bool (&ok)[4]) {  // one Philox block keys four consecutive rows
        const Philox r = philox4x32((uint32_t)g, env0 + (uint32_t)b, STREAM_CAPTURE, 0u, k0, k1);
#pragma unroll
        for (int u = 0; u < 4; ++u) key[u] = r.c[u], ok[u] = 4 * g + u < n && rb[min(4 * g + u, n - 1)] == 0;
      },
      sel, hist, s3);
  if (valid < n_out) return;  // np.random.choice would raise: the host reports it from count[b]
  const float *cb = cloud + (int64_t)b * cbs;
  for (int k = tid; k < n_out; k += SEL_THREADS) {
    const int i = (int)(uint32_t)sel[k];
    const float *p = cb + (int64_t)i * cps;
    float *o = out + (int64_t)b * obs + (int64_t)k * ops;
    o[0] = p[0], o[1] = p[1], o[2] = p[2];
    if (src_index) src_index[(size_t)b * n_out + k] = i;
  }
}

MPX_EXPORT int64_t mpx_cloud_clean_scratch(int B, int N) {
  if (B < 0 || N < 0) return -1;
  return (int64_t)clean_layout(B, N).total;
}

MPX_EXPORT int mpx_cloud_clean(const float *cloud, int64_t cloud_batch_stride, int cloud_point_stride, int N,
                               const int32_t *counts, int B, const float *boxes, int n_boxes, const float *sph_centers,
                               const float *sph_radii, int S, float robot_margin, float outlier_radius, int min_neighbors,
                               int n_out, uint64_t seed, int64_t env_offset, float *out, int64_t out_batch_stride,
                               int out_point_stride, int32_t *src_index, uint8_t *reason, int32_t *count, void *scratch,
                               int64_t scratch_bytes, mpx_stream_t stream) {
  MPX_REQUIRE(B >= 0 && N >= 0 && n_boxes >= 0 && S >= 0 && min_neighbors >= 0 && n_out >= 0, "mpx_cloud_clean: negative size");
  MPX_REQUIRE(B <= MPX_GRID_Y && N <= (1 << 30), "mpx_cloud_clean: at most %d environments of 2^30 rows", MPX_GRID_Y);
  MPX_REQUIRE(n_out <= SEL_MAX_OUT, "mpx_cloud_clean: n_out = %d, at most %d", n_out, SEL_MAX_OUT);
  MPX_REQUIRE(S <= MPX_CLEAN_MAX_SPHERES, "mpx_cloud_clean: S = %d spheres, at most %d", S, MPX_CLEAN_MAX_SPHERES);
  MPX_REQUIRE(n_boxes <= MPX_CLEAN_MAX_BOXES, "mpx_cloud_clean: n_boxes = %d, at most %d", n_boxes, MPX_CLEAN_MAX_BOXES);
  MPX_REQUIRE(robot_margin >= 0.0f, "mpx_cloud_clean: robot_margin must be >= 0");
  MPX_REQUIRE(min_neighbors == 0 || outlier_radius > 0.0f, "mpx_cloud_clean: outlier_radius must be > 0 when min_neighbors > 0");
  MPX_REQUIRE(cloud_point_stride >= 3, "mpx_cloud_clean: cloud_point_stride < 3");
  MPX_REQUIRE(n_out == 0 || out_point_stride >= 3, "mpx_cloud_clean: out_point_stride < 3");
  if (franka_env_offset_check("mpx_cloud_clean", env_offset, B)) return 1;
  const CleanLayout L = clean_layout(B, N);
  if (franka_scratch_size_check("mpx_cloud_clean", scratch_bytes, (int64_t)L.total, {B, N})) return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(count && scratch && (cloud || N == 0) && (boxes || n_boxes == 0) && ((sph_centers && sph_radii) || S == 0) &&
                  (out || n_out == 0),
              "mpx_cloud_clean: NULL operand");
  MPX_REQUIRE(((uintptr_t)scratch & 15) == 0, "mpx_cloud_clean: scratch must be 16-byte aligned");
  hipStream_t st = mpx_s(stream);
  char *sb = static_cast<char *>(scratch);
  CleanGrid *grid = reinterpret_cast<CleanGrid *>(sb);
  int *cells = reinterpret_cast<int *>(sb + L.cells);
  float4 *packed = reinterpret_cast<float4 *>(sb + L.packed);
  uint8_t *rs = reason ? reason : reinterpret_cast<uint8_t *>(sb + L.reason);  // (either one is [B, N] dense)
  if (hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)B, st) != hipSuccess ||
      hipMemsetAsync(grid, 0, sizeof(CleanGrid) * (size_t)B, st) != hipSuccess) {
    mpx_set_error("mpx_cloud_clean: cannot zero the counters: %s", hipGetErrorString(hipGetLastError()));
    return 2;
  }
  if (N == 0) return 0;  // no row: count = 0, nothing drawn
  const dim3 rows((unsigned)cdiv(N, 256), (unsigned)B);
  const int stage4 = min_neighbors > 0;
  hipLaunchKernelGGL(clean_classify_kernel, rows, dim3(256), 0, st, cloud, cloud_batch_stride, cloud_point_stride, N, counts,
                     boxes, n_boxes, sph_centers, sph_radii, S, robot_margin, stage4, rs, grid, count);
  if (stage4) {
    hipLaunchKernelGGL(clean_grid_kernel, dim3((unsigned)B), dim3(256), 0, st, grid, boxes, n_boxes, outlier_radius, cells);
    hipLaunchKernelGGL(clean_bin_kernel<false>, rows, dim3(256), 0, st, cloud, cloud_batch_stride, cloud_point_stride, N, rs,
                       grid, cells, packed, L.np);
    hipLaunchKernelGGL(clean_scan_kernel, dim3((unsigned)B), dim3(1024), 0, st, grid, cells);
    hipLaunchKernelGGL(clean_bin_kernel<true>, rows, dim3(256), 0, st, cloud, cloud_batch_stride, cloud_point_stride, N, rs,
                       grid, cells, packed, L.np);
    hipLaunchKernelGGL(clean_neighbors_kernel, rows, dim3(256), 0, st, packed, L.np, grid, cells,
                       outlier_radius * outlier_radius, min_neighbors, rs, N, count);
  }
  if (n_out > 0)
    hipLaunchKernelGGL(clean_draw_kernel, dim3((unsigned)B), dim3(SEL_THREADS), 0, st, cloud, cloud_batch_stride,
                       cloud_point_stride, N, counts, rs, n_out, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset,
                       out, out_batch_stride, out_point_stride, src_index);
  MPX_LAUNCH_CHECK("mpx_cloud_clean");
}
