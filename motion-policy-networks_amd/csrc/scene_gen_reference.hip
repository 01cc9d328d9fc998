// scene_gen_reference.hip -- the scenes the reference's generators build, drawn on the device: the tabletop of setup_tables +
// place_objects + random_object (kind 3), the cubby of Cubby.__init__ / .cuboids / .support_volumes (kind 4) and the merged
// cubby (kind 5).  The contract, draw by draw and operation by operation, is stated in include/mpinets_hip.h
// (mpx_scene_generate_reference); scene_gen.hip and its kernel are not touched by this file.
//
// One wave per scene, four scenes per workgroup of 256 threads, nothing shared between the waves: no barrier, no LDS.  A lane
// owns row `lane` of every output array.  Tables and plates sit on the lane of their row.  The tabletop's candidates are
// counter-keyed by their index, so every lane draws three of them up front (candidate 64 r + lane in round r); the greedy
// accept walk is the one sequential part: at most 140 steps, each a lane read of the candidate, one footprint distance per
// placed object (object i is held by lane i, at most 14), a ballot for the verdict and, on an accept, four lane exchanges for
// the least distance.  The accepted object stays on lane `placed` and remembers its row; the rows are stored at the end.
#include "common.h"
#include "philox.h"

enum { SREF_STREAM = 19 };
enum { SREF_WAVES = 4, SREF_THREADS = 64 * SREF_WAVES };
enum { SREF_TABLETOP = 3, SREF_CUBBY = 4, SREF_MERGED = 5 };
enum { SREF_SURFACE = 1, SREF_VOLUME = 2 };
enum { SREF_ROUNDS = 3 };  // 140 candidates at most: three per lane

#define SREF_SPAN_15 1.5e-1f  // 0.15: a span or bound of uniform ranges and the footprint cap (the decimal spelling is franka_device.h's body radius alone)
#define SREF_PIO2 1.57079632679489661923f
#define SREF_PI18 0.17453292519943295f
#define SREF_PI9 0.3490658503988659f

__device__ __forceinline__ int sref_draw_int(uint32_t word, uint32_t n) { return (int)(((word >> 8) * n) >> 24); }
__device__ __forceinline__ float sref_lane(float v, int src) {  // (src is wave-uniform)
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

struct SrefBox {  // a cuboid row or a support row: centre, dims, the quaternion (w, 0, 0, z)
  float c[3], d[3], qw, qz;
};

__device__ __forceinline__ void sref_store_cuboid(float *__restrict__ cc, float *__restrict__ cd, float *__restrict__ cq, size_t r,
                                                  const SrefBox &b) {
  cc[3 * r + 0] = b.c[0], cc[3 * r + 1] = b.c[1], cc[3 * r + 2] = b.c[2];
  cd[3 * r + 0] = b.d[0], cd[3 * r + 1] = b.d[1], cd[3 * r + 2] = b.d[2];
  *reinterpret_cast<float4 *>(cq + 4 * r) = make_float4(b.qw, 0.0f, 0.0f, b.qz);
}
__device__ __forceinline__ void sref_store_cylinder(float *__restrict__ yc, float *__restrict__ yr, float *__restrict__ yh,
                                                    float *__restrict__ yq, size_t r, float x, float y, float z, float radius,
                                                    float height) {
  yc[3 * r + 0] = x, yc[3 * r + 1] = y, yc[3 * r + 2] = z;
  yr[r] = radius, yh[r] = height;
  *reinterpret_cast<float4 *>(yq + 4 * r) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(SREF_THREADS)
    scene_reference_kernel(const int32_t *__restrict__ scene_kind, const int64_t *__restrict__ scene_ids,
                           const int32_t *__restrict__ merge_pockets, int B, int M1, int M2, int S, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t id0, float *__restrict__ cub_c, float *__restrict__ cub_d,
                           float *__restrict__ cub_q, float *__restrict__ cyl_c, float *__restrict__ cyl_r,
                           float *__restrict__ cyl_h, float *__restrict__ cyl_q, float *__restrict__ sup_box,
                           int32_t *__restrict__ sup_kind) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long b = (long long)blockIdx.x * SREF_WAVES + wave;
  if (b >= B) return;  // (wave-uniform; the kernel has no barrier)
  const int kind = __builtin_amdgcn_readfirstlane(scene_kind[b]);
  if (kind < SREF_TABLETOP || kind > SREF_MERGED) return;  // not this entry's row: left untouched
  const uint32_t id = scene_ids ? (uint32_t)scene_ids[b] : id0 + (uint32_t)b;

  // what this lane stores: a table or plate in row `lane` (has_cub), an object in row obj_row of the cuboids (otype 2) or
  // of the cylinders (otype 1), the support of row `lane`
  const SrefBox pad = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 1.0f, 0.0f};
  SrefBox cub = pad, sup = pad, obj = pad;
  bool has_cub = false;
  int otype = 0, obj_row = -1, skind = 0;
  float weight = 0.0f, orad = 0.0f;  // (orad: a cylinder object's radius)
  int n_cub = 0, n_cyl = 0;  // live rows (wave-uniform)

  const Philox a0 = philox4x32(0u, id, SREF_STREAM, 0u, seed_lo, seed_hi);
  const Philox a1 = philox4x32(0u, id, SREF_STREAM, 1u, seed_lo, seed_hi);
  const Philox a2 = philox4x32(0u, id, SREF_STREAM, 2u, seed_lo, seed_hi);
  const Philox a3 = philox4x32(0u, id, SREF_STREAM, 3u, seed_lo, seed_hi);
  if (kind == SREF_TABLETOP) {
    const float h = u01(a0.c[0]) < 0.35f ? 0.0f : u01(a0.c[1]) * 0.4f;
    const float tz = (h - 0.02f) * 0.5f, td = h + 0.02f;
    const float fx0 = mpx_fma(u01(a0.c[2]), 0.1f, 0.275f), fx1 = mpx_fma(u01(a0.c[3]), 0.1f, 1.275f);
    const float fy1 = mpx_fma(u01(a1.c[0]), SREF_SPAN_15, 1.5f);
    const bool side = u01(a1.c[1]) < 0.5f;
    const float fy0 = side ? mpx_fma(u01(a1.c[2]), 0.25f, -1.0f) : mpx_fma(u01(a1.c[2]), 0.2f, -0.75f);
    const float Dx = fx1 - fx0, Dy = fy1 - fy0;
    const float ty = mpx_fma(u01(a1.c[3]), 0.1f, 0.55f) * Dy;
    const float sy1 = mpx_fma(u01(a2.c[0]), 0.05f, -0.325f);
    const float L = u01(a2.c[1]) * 1.375f;
    const float sdx = L * mpx_fma(u01(a2.c[2]), 0.1f, 0.55f);
    const float SDy = sy1 - fy0;
    const float mcx = mpx_fma(u01(a2.c[3]), 0.04f, -0.02f), mcy = mpx_fma(u01(a3.c[0]), 0.04f, -0.02f);
    const float mdy = mpx_fma(u01(a3.c[1]), 0.04f, 0.9f);
    const int K = 3 + sref_draw_int(a3.c[3], 12u);
    const int T = side ? 5 : 3;
    const int role = side ? lane : lane == 0 ? 0 : lane == 1 ? 2 : 4;  // 0 front task, 1 side task, 2 front free, 3 side free, 4 mount
    if (lane < T) {
      has_cub = true;
      cub.c[2] = tz, cub.d[2] = td;
      if (role == 0) {
        cub.c[0] = (fx0 + fx1) * 0.5f, cub.c[1] = mpx_fma(ty, 0.5f, fy0);
        cub.d[0] = Dx, cub.d[1] = ty;
      } else if (role == 2) {
        cub.c[0] = (fx0 + fx1) * 0.5f, cub.c[1] = (fy1 + (fy0 + ty)) * 0.5f;
        cub.d[0] = Dx, cub.d[1] = Dy - ty;
      } else if (role == 1) {
        cub.c[0] = fx0 - sdx * 0.5f, cub.c[1] = (sy1 + fy0) * 0.5f;
        cub.d[0] = sdx, cub.d[1] = SDy;
      } else if (role == 3) {
        cub.c[0] = ((fx0 - L) + (fx0 - sdx)) * 0.5f, cub.c[1] = (sy1 + fy0) * 0.5f;
        cub.d[0] = L - sdx, cub.d[1] = SDy;
      } else {
        cub.c[0] = mcx, cub.c[1] = mcy, cub.c[2] = -0.01f;
        cub.d[0] = 2.0f * (fx0 - mcx), cub.d[1] = side ? 2.0f * (mcy - sy1) : mdy, cub.d[2] = 0.02f;
      }
      if (role < 2) {  // the task tables' tops; the free tables and the mount table are not supports
        sup = cub;
        skind = SREF_SURFACE;
        weight = cub.d[0] * cub.d[1];
      }
    }
    // the candidates, three per lane: position, the type uniform, the four shape uniforms
    const float A0 = Dx * ty, A1 = side ? sdx * SDy : 0.0f;
    float kx[SREF_ROUNDS], ky[SREF_ROUNDS], kt[SREF_ROUNDS], k4[SREF_ROUNDS], k5[SREF_ROUNDS], k6[SREF_ROUNDS], k7[SREF_ROUNDS];
#pragma unroll
    for (int r = 0; r < SREF_ROUNDS; ++r) {
      const uint32_t item = (uint32_t)(64 * r + lane + 1);
      const Philox o = philox4x32(item, id, SREF_STREAM, 0u, seed_lo, seed_hi);
      const Philox p = philox4x32(item, id, SREF_STREAM, 1u, seed_lo, seed_hi);
      const bool on_side = side && u01(o.c[0]) * (A0 + A1) >= A0;
      kx[r] = on_side ? mpx_fma(u01(o.c[1]), sdx, fx0 - sdx) : mpx_fma(u01(o.c[1]), Dx, fx0);
      ky[r] = on_side ? mpx_fma(u01(o.c[2]), SDy, fy0) : mpx_fma(u01(o.c[2]), ty, fy0);
      kt[r] = u01(o.c[3]);
      k4[r] = u01(p.c[0]), k5[r] = u01(p.c[1]), k6[r] = u01(p.c[2]), k7[r] = u01(p.c[3]);
    }
    // the accept walk: lane i < placed holds object i's footprint (ocs, osn: cosine and sine of a cuboid's yaw)
    float ocs = 1.0f, osn = 0.0f;
    int placed = 0, n_box = 0;  // (n_box: the objects among the cuboids)
    const int ncand = 10 * K;
#pragma unroll
    for (int r = 0; r < SREF_ROUNDS; ++r) {
      for (int j = 0; j < 64; ++j) {
        if (64 * r + j >= ncand || placed >= K) break;  // (wave-uniform)
        const float x = sref_lane(kx[r], j), y = sref_lane(ky[r], j);
        float d = 1000.0f;
        if (lane < placed) {
          const float dx = x - obj.c[0], dy = y - obj.c[1];
          if (otype == 1) {
            d = sqrtf(mpx_fma(dx, dx, dy * dy)) - orad;
          } else {
            const float lx = mpx_fma(ocs, dx, osn * dy), ly = mpx_fma(ocs, dy, -(osn * dx));
            const float qx = fabsf(lx) - 0.5f * obj.d[0], qy = fabsf(ly) - 0.5f * obj.d[1];
            const float ex = fmaxf(qx, 0.0f), ey = fmaxf(qy, 0.0f);
            d = sqrtf(mpx_fma(ex, ex, ey * ey)) + fminf(fmaxf(qx, qy), 0.0f);
          }
        }
        if (__builtin_amdgcn_ballot_w64(d <= 0.05f) != 0ull) continue;  // too close to a placed object
        float m = d;  // the least distance: the placed objects sit on lanes 0 .. 13, the other lanes hold 1000
        m = fminf(m, __shfl_xor(m, 8));
        m = fminf(m, __shfl_xor(m, 4));
        m = fminf(m, __shfl_xor(m, 2));
        m = fminf(m, __shfl_xor(m, 1));
        m = sref_lane(m, 0);
        const float span = fminf(m, SREF_SPAN_15) - 0.05f;
        const bool is_cyl = sref_lane(kt[r], j) < 0.3f;
        const float v4 = sref_lane(k4[r], j), v5 = sref_lane(k5[r], j);
        if (is_cyl) {
          if (n_cyl >= M2) continue;  // the overflow rule: no row, not counted, blocks nothing
          if (lane == placed) {
            otype = 1, obj_row = n_cyl;
            orad = mpx_fma(v4, span, 0.05f);
            obj.d[2] = mpx_fma(v5, 0.3f, 0.05f);
            obj.c[0] = x, obj.c[1] = y, obj.c[2] = mpx_fma(obj.d[2], 0.5f, h);
          }
          ++n_cyl;
        } else {
          if (T + n_box >= M1) continue;
          const float yaw = sref_lane(k7[r], j) * SREF_PIO2;
          const float dz = mpx_fma(sref_lane(k6[r], j), 0.3f, 0.05f);
          float sn, cs, qz, qw;
          mpx_sincos(yaw, sn, cs);
          mpx_sincos(0.5f * yaw, qz, qw);
          if (lane == placed) {
            otype = 2, obj_row = T + n_box;
            obj.d[0] = mpx_fma(v4, span, 0.05f), obj.d[1] = mpx_fma(v5, span, 0.05f), obj.d[2] = dz;
            obj.c[0] = x, obj.c[1] = y, obj.c[2] = mpx_fma(dz, 0.5f, h);
            obj.qw = qw, obj.qz = qz;
            ocs = cs, osn = sn;
          }
          ++n_box;
        }
        ++placed;
      }
    }
    n_cub = T + n_box;
  } else {  // the cubby (kind 4) and the merged cubby (kind 5): one set of parameters
    const float left = mpx_fma(u01(a0.c[0]), 0.2f, 0.6f), right = mpx_fma(u01(a0.c[1]), 0.2f, -0.8f);
    const float bottom = mpx_fma(u01(a0.c[2]), 0.2f, 0.1f), front = mpx_fma(u01(a0.c[3]), 0.2f, 0.45f);
    const float back = front + mpx_fma(u01(a1.c[0]), 0.4f, SREF_SPAN_15), top = mpx_fma(u01(a1.c[1]), 0.2f, 0.6f);
    const float mz = mpx_fma(u01(a1.c[2]), 0.2f, 0.35f), my = mpx_fma(u01(a1.c[3]), 0.2f, -0.1f);
    const float t = mpx_fma(u01(a2.c[0]), 0.02f, 0.01f);
    const float yaw = mpx_fma(u01(a2.c[1]), SREF_PI9, -SREF_PI18);
    int pa = -1, pb = -1;
    if (kind == SREF_MERGED) {
      if (merge_pockets) {
        pa = merge_pockets[2 * b], pb = merge_pockets[2 * b + 1];
      } else {  // the six unordered pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const int i = sref_draw_int(a3.c[0], 6u);
        pa = i < 3 ? 0 : i < 5 ? 1 : 2;
        pb = i < 3 ? i + 1 : i < 5 ? i - 1 : 3;
      }
    }
    pa = __builtin_amdgcn_readfirstlane(pa), pb = __builtin_amdgcn_readfirstlane(pb);
    const bool merged = pa >= 0 && pa <= 3 && pb >= 0 && pb <= 3 && pa != pb;  // anything else: unmerged
    const bool no_shelf = merged && (pa >> 1) != (pb >> 1), no_wall = merged && (pa & 1) != (pb & 1);
    float s, c, qz, qw;
    mpx_sincos(yaw, s, c);
    mpx_sincos(0.5f * yaw, qz, qw);
    const float px = (front + back) * 0.5f, py = (left + right) * 0.5f, pz = (top + bottom) * 0.5f;
    const float Dd = back - front, Wd = left - right, Hd = (top - bottom) + t;
    n_cub = 7 - (no_shelf ? 1 : 0) - (no_wall ? 1 : 0);
    float lx = px, ly = py, lz = pz;
    bool placed_box = false;
    if (lane < n_cub) {
      // plates 0 back, 1 bottom, 2 top, 3 right, 4 left, 5 centre wall, 6 middle shelf; a removed plate's successors move up
      const int pl = lane < 5 ? lane : lane == 5 ? (no_wall ? 6 : 5) : 6;
      has_cub = placed_box = true;
      lx = pl == 0 ? back : px;
      ly = pl == 3 ? right : pl == 4 ? left : pl == 5 ? my : py;
      lz = pl == 0 ? top * 0.5f : pl == 1 ? bottom : pl == 2 ? top : pl == 6 ? mz : pz;
      cub.d[0] = pl == 0 ? t : Dd;
      cub.d[1] = (pl >= 3 && pl <= 5) ? t : Wd;
      cub.d[2] = pl == 0 ? top : (pl >= 3 && pl <= 5) ? Hd : t;
    }
    if (placed_box) {
      const float ax = lx - px, ay = ly - py;
      cub.c[0] = (c * ax - s * ay) + px, cub.c[1] = (s * ax + c * ay) + py, cub.c[2] = lz;
      cub.qw = qw, cub.qz = qz;
    }
    const int ns = no_shelf && no_wall ? 1 : (no_shelf || no_wall) ? 2 : 4;
    if (lane < ns) {
      const int level = no_shelf ? -1 : no_wall ? lane : lane >> 1;  // -1: the whole extent
      const int sd = no_wall ? -1 : no_shelf ? lane : lane & 1;
      const float ya = sd == 0 ? my : right, yb = sd == 1 ? my : left;
      const float za = level == 0 ? mz : bottom, zb = level == 1 ? mz : top;
      const float ay = (ya + yb) * 0.5f - py;  // (the local x is the pivot's)
      sup.c[0] = -(s * ay) + px, sup.c[1] = c * ay + py, sup.c[2] = (za + zb) * 0.5f;
      sup.d[0] = Dd, sup.d[1] = yb - ya, sup.d[2] = zb - za;
      sup.qw = qw, sup.qz = qz;
      skind = SREF_VOLUME;
      weight = 1.0f;
    }
  }

  // ---- the stores: the lane's table or plate, its object, then the padding of the rows with its own index behind the live
  // prefix.  Live rows are 0 .. n-1 and padding rows n .. M-1, so every element of the scene's rows is written exactly once.
  if (has_cub) sref_store_cuboid(cub_c, cub_d, cub_q, (size_t)b * M1 + lane, cub);
  if (otype == 2) sref_store_cuboid(cub_c, cub_d, cub_q, (size_t)b * M1 + obj_row, obj);
  if (lane < M1 && lane >= n_cub) sref_store_cuboid(cub_c, cub_d, cub_q, (size_t)b * M1 + lane, pad);
  if (otype == 1) sref_store_cylinder(cyl_c, cyl_r, cyl_h, cyl_q, (size_t)b * M2 + obj_row, obj.c[0], obj.c[1], obj.c[2], orad, obj.d[2]);
  if (lane < M2 && lane >= n_cyl) sref_store_cylinder(cyl_c, cyl_r, cyl_h, cyl_q, (size_t)b * M2 + lane, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
  if (sup_box && lane < S) {  // (a live support of a row >= S is not kept: "the first S"; a lane without one holds the padding)
    const size_t r = (size_t)b * S + lane;
    float4 *row = reinterpret_cast<float4 *>(sup_box + 12 * r);
    row[0] = make_float4(sup.c[0], sup.c[1], sup.c[2], sup.d[0]);
    row[1] = make_float4(sup.d[1], sup.d[2], sup.qw, 0.0f);
    row[2] = make_float4(0.0f, sup.qz, 0.0f, weight);
    sup_kind[r] = skind;
  }
}

MPX_EXPORT int mpx_scene_generate_reference(const int32_t *scene_kind, const int64_t *scene_ids, const int32_t *merge_pockets, int B,
                                            int M1, int M2, int S, uint64_t seed, int64_t scene_offset, float *cuboid_centers,
                                            float *cuboid_dims, float *cuboid_quats, float *cylinder_centers, float *cylinder_radii,
                                            float *cylinder_heights, float *cylinder_quats, float *support_boxes,
                                            int32_t *support_kind, mpx_stream_t stream) {
  const char *who = "mpx_scene_generate_reference";
  MPX_REQUIRE(B >= 0, "%s: negative size", who);
  MPX_REQUIRE(M1 >= 7 && M1 <= 64, "%s: M1 = %d cuboid rows, need 7 .. 64 (the cubby's plates; a lane per row)", who, M1);
  MPX_REQUIRE(M2 >= 0 && M2 <= 64, "%s: M2 = %d cylinder rows, need 0 .. 64 (a lane per row)", who, M2);
  MPX_REQUIRE((support_boxes != nullptr) == (support_kind != nullptr),
              "%s: support_boxes and support_kind go together: one of them is NULL", who);
  if (support_boxes)
    MPX_REQUIRE(S >= 1 && S <= MPX_TASK_MAX_SUPPORTS, "%s: S = %d supports per scene, need 1 .. %d", who, S, MPX_TASK_MAX_SUPPORTS);
  else
    MPX_REQUIRE(S == 0, "%s: S = %d without support arrays, need 0", who, S);
  MPX_REQUIRE(scene_offset >= 0, "%s: scene_offset is negative", who);
  MPX_REQUIRE(scene_offset + (int64_t)B <= ((int64_t)1 << 32), "%s: scene_offset + B exceeds 2^32", who);
  if (B == 0) return 0;
  MPX_REQUIRE(scene_kind, "%s: NULL operand (scene_kind)", who);
  MPX_REQUIRE((((uintptr_t)cuboid_quats | (uintptr_t)cylinder_quats | (uintptr_t)support_boxes) & 15) == 0,
              "%s: cuboid_quats, cylinder_quats and support_boxes must be 16-byte aligned (rows are stored as float4)", who);
  MPX_REQUIRE(cuboid_centers && cuboid_dims && cuboid_quats, "%s: NULL output (cuboid_centers, cuboid_dims, cuboid_quats)", who);
  MPX_REQUIRE(M2 == 0 || (cylinder_centers && cylinder_radii && cylinder_heights && cylinder_quats),
              "%s: NULL output (cylinder_centers, cylinder_radii, cylinder_heights, cylinder_quats) with M2 = %d", who, M2);
  const unsigned grid = (unsigned)(((int64_t)B + SREF_WAVES - 1) / SREF_WAVES);
  hipLaunchKernelGGL(scene_reference_kernel, dim3(grid), dim3(SREF_THREADS), 0, mpx_s(stream), scene_kind, scene_ids, merge_pockets,
                     B, M1, M2, S, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)scene_offset, cuboid_centers, cuboid_dims,
                     cuboid_quats, cylinder_centers, cylinder_radii, cylinder_heights, cylinder_quats, support_boxes, support_kind);
  MPX_LAUNCH_CHECK(who);
}
