// scene_gen.hip -- scenes drawn on the device: the distributions of scenes.py's host generators (_tabletop, _cubby,
// _dresser) and the supports make_task_scenes reads off them, every scene a function of (seed, scene id, kind, M1, M2, S)
// alone.  The contract, draw by draw and operation by operation, is stated in include/mpinets_hip.h (mpx_scene_generate).
//
// One wave per scene, four scenes per workgroup of 256 threads; nothing is shared between the waves, so there is no barrier
// and no LDS.  A lane owns one row of every output array (M1, M2, S <= 64): it computes the primitive that lands in a row --
// the scene's parameters (item 0) are computed by every lane, they are wave-uniform -- and stores it, or stores the padding
// of the row with its own index behind the live prefix.  Only the tabletop moves a lane's object to a row that is not the
// lane's: the objects sit on lanes 3 .. 3 + K-1 behind the tables' lanes, and two ordered ballot compactions (the idiom of
// task_candidates.hip) give a cylinder its row among the cylinders and a cuboid candidate its row behind the tables.  Live
// rows and padding rows are disjoint by construction (live rows are 0 .. n-1, padding n .. M-1), so every element is
// written exactly once.
#include "common.h"
#include "philox.h"

enum { STREAM_SCENE_GEN = 19 };
enum { SCENE_WAVES = 4, SCENE_THREADS = 64 * SCENE_WAVES };
enum { SCENE_TABLETOP = 0, SCENE_CUBBY = 1, SCENE_DRESSER = 2 };
enum { SUPPORT_SURFACE = 1, SUPPORT_VOLUME = 2 };

#define SCENE_SPAN_15 1.5e-1f  // 0.15: the width of two uniform ranges (the decimal spelling is franka_device.h's body radius alone)
#define SCENE_PIO2 1.57079632679489661923f
#define SCENE_PI18 0.17453292519943295f
#define SCENE_PI9 0.3490658503988659f
#define SCENE_PI6 0.52359877559829887f
#define SCENE_2PI3 2.0943951023931953f

__device__ __forceinline__ int scene_draw_int(uint32_t word, uint32_t n) { return (int)(((word >> 8) * n) >> 24); }

struct SceneBox {  // a cuboid row or a support row: centre, dims, the quaternion (w, 0, 0, z)
  float c[3], d[3], qw, qz;
};
// W(l) of the contract: the local point under the yaw (c, s) at the origin (ox, oz)
__device__ __forceinline__ void scene_place(SceneBox &b, float c, float s, float lx, float ly, float lz, float ox, float oz) {
  b.c[0] = (c * lx - s * ly) + ox;
  b.c[1] = s * lx + c * ly;
  b.c[2] = lz + oz;
}

__device__ __forceinline__ void scene_store_cuboid(float *__restrict__ cc, float *__restrict__ cd, float *__restrict__ cq, size_t r,
                                                   const SceneBox &b) {
  cc[3 * r + 0] = b.c[0], cc[3 * r + 1] = b.c[1], cc[3 * r + 2] = b.c[2];
  cd[3 * r + 0] = b.d[0], cd[3 * r + 1] = b.d[1], cd[3 * r + 2] = b.d[2];
  *reinterpret_cast<float4 *>(cq + 4 * r) = make_float4(b.qw, 0.0f, 0.0f, b.qz);
}
__device__ __forceinline__ void scene_store_cylinder(float *__restrict__ yc, float *__restrict__ yr, float *__restrict__ yh,
                                                     float *__restrict__ yq, size_t r, float x, float y, float z, float radius,
                                                     float height) {
  yc[3 * r + 0] = x, yc[3 * r + 1] = y, yc[3 * r + 2] = z;
  yr[r] = radius, yh[r] = height;
  *reinterpret_cast<float4 *>(yq + 4 * r) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(SCENE_THREADS)
    scene_generate_kernel(const int32_t *__restrict__ scene_kind, const int64_t *__restrict__ scene_ids, int B, int M1, int M2,
                          int S, uint32_t seed_lo, uint32_t seed_hi, uint32_t id0, float *__restrict__ cub_c,
                          float *__restrict__ cub_d, float *__restrict__ cub_q, float *__restrict__ cyl_c,
                          float *__restrict__ cyl_r, float *__restrict__ cyl_h, float *__restrict__ cyl_q,
                          float *__restrict__ sup_box, int32_t *__restrict__ sup_kind) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long b = (long long)blockIdx.x * SCENE_WAVES + wave;
  if (b >= B) return;  // (wave-uniform; the kernel has no barrier)
  const uint32_t id = scene_ids ? (uint32_t)scene_ids[b] : id0 + (uint32_t)b;
  const int kind = __builtin_amdgcn_readfirstlane(scene_kind[b]);
  const unsigned long long below = (1ull << lane) - 1ull;

  // what this lane stores: a cuboid in row cub_row, a cylinder in row cyl_row (-1: none), the support of row `lane`
  SceneBox cub = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 1.0f, 0.0f}, sup = cub;
  float yc[3] = {0.0f, 0.0f, 0.0f}, yr = 0.0f, yh = 0.0f, approach = 0.0f, weight = 0.0f;
  int cub_row = -1, cyl_row = -1, skind = 0;
  int n_cub = 0, n_cyl = 0;  // live rows (wave-uniform)

  const Philox a = philox4x32(0u, id, STREAM_SCENE_GEN, 0u, seed_lo, seed_hi);
  const Philox e = philox4x32(0u, id, STREAM_SCENE_GEN, 1u, seed_lo, seed_hi);
  if (kind == SCENE_TABLETOP) {
    const float h = u01(a.c[0]) < 0.35f ? 0.0f : u01(a.c[1]) * 0.4f;
    const float x0 = mpx_fma(u01(a.c[2]), 0.1f, 0.275f), x1 = mpx_fma(u01(a.c[3]), 0.1f, 1.275f);
    const float w = mpx_fma(u01(e.c[0]), SCENE_SPAN_15, 1.5f);
    const bool has_side = u01(e.c[1]) < 0.5f;
    const float side = u01(e.c[2]) < 0.5f ? -1.0f : 1.0f;
    const int K = 3 + scene_draw_int(e.c[3], 12u);
    const int T = has_side ? 3 : 2;
    // the objects: lane 3 + k
    const int k = lane - 3;
    const bool is_obj = k >= 0 && k < K;
    const Philox o = philox4x32((uint32_t)(k + 1), id, STREAM_SCENE_GEN, 0u, seed_lo, seed_hi);
    const Philox p = philox4x32((uint32_t)(k + 1), id, STREAM_SCENE_GEN, 1u, seed_lo, seed_hi);
    const float lo = x0 + 0.1f;
    const float px = mpx_fma(u01(o.c[0]), (x1 - 0.1f) - lo, lo);
    const float hw = w * 0.5f - 0.1f;
    const float py = mpx_fma(u01(o.c[1]), hw + hw, -hw);
    const bool drew_cyl = is_obj && u01(o.c[2]) < 0.3f;
    const unsigned long long cyl_mask = __builtin_amdgcn_ballot_w64(drew_cyl);
    const int rank_c = __builtin_popcountll(cyl_mask & below);
    const bool is_cyl = drew_cyl && rank_c < M2;
    const bool cand = is_obj && !is_cyl;
    const unsigned long long cand_mask = __builtin_amdgcn_ballot_w64(cand);
    const int rank_b = __builtin_popcountll(cand_mask & below);
    const int drawn = __builtin_popcountll(cyl_mask), cands = __builtin_popcountll(cand_mask);
    n_cyl = drawn < M2 ? drawn : M2;
    n_cub = T + (cands < M1 - T ? cands : M1 - T);
    if (is_cyl) {
      cyl_row = rank_c;
      yr = mpx_fma(u01(p.c[0]), 0.1f, 0.05f);
      yh = mpx_fma(u01(p.c[1]), 0.3f, 0.05f);
      yc[0] = px, yc[1] = py, yc[2] = mpx_fma(yh, 0.5f, h);
    } else if (cand && T + rank_b < M1) {
      cub_row = T + rank_b;
      cub.d[0] = mpx_fma(u01(p.c[0]), 0.1f, 0.05f);
      cub.d[1] = mpx_fma(u01(p.c[1]), 0.1f, 0.05f);
      cub.d[2] = mpx_fma(u01(p.c[2]), 0.3f, 0.05f);
      cub.c[0] = px, cub.c[1] = py, cub.c[2] = mpx_fma(cub.d[2], 0.5f, h);
      mpx_sincos(0.5f * (u01(p.c[3]) * SCENE_PIO2), cub.qz, cub.qw);
    } else if (lane == 0) {  // the front table
      cub_row = 0;
      cub.c[0] = (x0 + x1) * 0.5f, cub.c[2] = h - 0.025f;
      cub.d[0] = x1 - x0, cub.d[1] = w, cub.d[2] = 0.05f;
    } else if (lane == 1 && has_side) {
      cub_row = 1;
      cub.c[1] = side * mpx_fma(w, 0.25f, 0.45f), cub.c[2] = h - 0.025f;
      cub.d[0] = 0.9f, cub.d[1] = w * 0.5f, cub.d[2] = 0.05f;
    } else if (lane == T - 1) {  // the mount table under the robot
      cub_row = T - 1;
      cub.c[0] = -0.35f, cub.c[2] = -0.025f;
      cub.d[0] = 0.6f, cub.d[1] = 0.6f, cub.d[2] = 0.05f;
    }
    if (lane < T - 1) {  // the table tops; the mount table is not a support
      sup = cub;
      skind = SUPPORT_SURFACE;
      weight = cub.d[0] * cub.d[1];
    }
  } else if (kind == SCENE_CUBBY) {
    const float t = mpx_fma(u01(a.c[0]), 0.02f, 0.01f), W = mpx_fma(u01(a.c[1]), 0.4f, 0.7f);
    const float H = mpx_fma(u01(a.c[2]), 0.4f, 0.5f), D = mpx_fma(u01(a.c[3]), SCENE_SPAN_15, 0.2f);
    const float ox = mpx_fma(u01(e.c[0]), 0.25f, 0.55f), oz = mpx_fma(u01(e.c[1]), 0.2f, 0.1f);
    const float yaw = mpx_fma(u01(e.c[2]), SCENE_PI9, -SCENE_PI18);
    float s, c, qz, qw;
    mpx_sincos(yaw, s, c);
    mpx_sincos(0.5f * yaw, qz, qw);
    const float hH = H * 0.5f, hW = W * 0.5f, ht = t * 0.5f;
    n_cub = M1 < 7 ? M1 : 7;
    if (lane < n_cub) {
      cub_row = lane;
      const float lx = lane == 6 ? D * 0.5f : 0.0f;
      const float ly = lane == 3 ? -hW : lane == 4 ? hW : 0.0f;
      const float lz = lane == 0 ? 0.0f : lane == 1 ? H : hH;
      scene_place(cub, c, s, lx, ly, lz, ox, oz);
      cub.d[0] = lane == 6 ? t : D;
      cub.d[1] = (lane < 3 || lane == 6) ? W : t;
      cub.d[2] = lane < 3 ? t : H;
      cub.qw = qw, cub.qz = qz;
    }
    if (lane < 4) {  // the pockets
      const bool up = (lane >> 1) != 0, right = (lane & 1) != 0;
      const float z0 = up ? hH + ht : ht, z1 = up ? H - ht : hH - ht;
      const float y0 = right ? ht : -hW + ht, y1 = right ? hW - ht : -ht;
      scene_place(sup, c, s, -(t * 0.25f), (y0 + y1) * 0.5f, (z0 + z1) * 0.5f, ox, oz);
      sup.d[0] = D - ht, sup.d[1] = y1 - y0, sup.d[2] = z1 - z0;
      sup.qw = qw, sup.qz = qz;
      skind = SUPPORT_VOLUME;
      weight = 1.0f;
    }
  } else if (kind == SCENE_DRESSER) {
    const float W = mpx_fma(u01(a.c[0]), 0.4f, 0.8f), D = mpx_fma(u01(a.c[1]), 0.2f, 0.2f);
    const float H = mpx_fma(u01(a.c[2]), 0.3f, 0.55f), ox = mpx_fma(u01(a.c[3]), 0.2f, 0.55f);
    const float yaw = mpx_fma(u01(e.c[0]), SCENE_2PI3, SCENE_PI6);
    const int drawn = 12 + scene_draw_int(e.c[1], 29u);
    const int n = drawn < M1 ? drawn : M1;
    int rows = 1;
    while (rows * rows < n) ++rows;
    float s, c, qz, qw;
    mpx_sincos(yaw, s, c);
    mpx_sincos(0.5f * yaw, qz, qw);
    const float wc = W / (float)rows, hc = H / (float)rows;
    n_cub = n;
    if (lane < n) {
      cub_row = lane;
      const Philox o = philox4x32((uint32_t)(lane + 1), id, STREAM_SCENE_GEN, 0u, seed_lo, seed_hi);
      const float jitter = mpx_fma(u01(o.c[0]), 0.04f, -0.02f);
      const int ri = lane / rows, ci = lane - ri * rows;
      const float lx = mpx_fma((float)ci + 0.5f, wc, -(W * 0.5f));
      scene_place(cub, c, s, lx, jitter, ((float)ri + 0.5f) * hc, ox, 0.0f);
      cub.d[0] = wc * 0.95f, cub.d[1] = D, cub.d[2] = hc * 0.2f;
      cub.qw = qw, cub.qz = qz;
      sup = cub;  // the free space above the plate inside its cell
      sup.c[2] = ((float)ri + 0.8f) * hc;
      sup.d[2] = hc * 0.4f;
      skind = SUPPORT_VOLUME;
      weight = 1.0f;
      approach = yaw - SCENE_PIO2;
    }
  }

  // ---- the stores: the lane's live rows, then the padding of the rows with its own index behind the live prefix (a tabletop
  // lane may hold both: its object went to a row in front of its own) -------------------------------------------------------
  if (cub_row >= 0) scene_store_cuboid(cub_c, cub_d, cub_q, (size_t)b * M1 + cub_row, cub);
  if (lane < M1 && lane >= n_cub) scene_store_cuboid(cub_c, cub_d, cub_q, (size_t)b * M1 + lane, SceneBox{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 1.0f, 0.0f});
  if (cyl_row >= 0) scene_store_cylinder(cyl_c, cyl_r, cyl_h, cyl_q, (size_t)b * M2 + cyl_row, yc[0], yc[1], yc[2], yr, yh);
  if (lane < M2 && lane >= n_cyl) scene_store_cylinder(cyl_c, cyl_r, cyl_h, cyl_q, (size_t)b * M2 + lane, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
  if (sup_box && lane < S) {  // (a live support of a row >= S is not kept: "the first S"; a lane without one holds the padding)
    const size_t r = (size_t)b * S + lane;
    float4 *row = reinterpret_cast<float4 *>(sup_box + 12 * r);
    row[0] = make_float4(sup.c[0], sup.c[1], sup.c[2], sup.d[0]);
    row[1] = make_float4(sup.d[1], sup.d[2], sup.qw, 0.0f);
    row[2] = make_float4(0.0f, sup.qz, approach, weight);
    sup_kind[r] = skind;
  }
}

MPX_EXPORT int mpx_scene_generate(const int32_t *scene_kind, const int64_t *scene_ids, int B, int M1, int M2, int S, uint64_t seed,
                                  int64_t scene_offset, float *cuboid_centers, float *cuboid_dims, float *cuboid_quats,
                                  float *cylinder_centers, float *cylinder_radii, float *cylinder_heights, float *cylinder_quats,
                                  float *support_boxes, int32_t *support_kind, mpx_stream_t stream) {
  const char *who = "mpx_scene_generate";
  MPX_REQUIRE(B >= 0, "%s: negative size", who);
  MPX_REQUIRE(M1 >= 3 && M1 <= 64, "%s: M1 = %d cuboid rows, need 3 .. 64 (the tables; a lane per row)", who, M1);
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
  const unsigned grid = (unsigned)(((int64_t)B + SCENE_WAVES - 1) / SCENE_WAVES);
  hipLaunchKernelGGL(scene_generate_kernel, dim3(grid), dim3(SCENE_THREADS), 0, mpx_s(stream), scene_kind, scene_ids, B, M1, M2,
                     S, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)scene_offset, cuboid_centers, cuboid_dims, cuboid_quats,
                     cylinder_centers, cylinder_radii, cylinder_heights, cylinder_quats, support_boxes, support_kind);
  MPX_LAUNCH_CHECK(who);
}
