// plan_prims_device.h -- the validity test of ONE configuration against a problem's live primitives (the LDS rows of
// franka_live_rows.inc) and the self model: the clause "a sphere with sdf <= r_s + clearance + check_margin" of
// mpx_franka_plan's contract (include/mpinets_hip.h).  Shared by plan.hip (the validity sweep, the endpoints) and
// roadmap.hip (nodes and the interior configurations of an edge): both judge a configuration by the same statements.
#pragma once
#include "plan_device.h"
#include "sdf_device.h"

// min over the live primitives (LDS rows [R | Rt (3 x 4 floats) | sizes]; cuboids from row 0, cylinders from row 64) and
// the row that attains it: the first minimum, cuboids before cylinders (-1: no live primitive)
__device__ __forceinline__ float plan_min_sdf(const float *prim_rows, int n_cub, int n_cyl, float x, float y, float z,
                                              int &arg) {
  float best = __builtin_inff();
  arg = -1;
  for (int m = 0; m < n_cub; ++m) {
    const float *row = prim_rows + 16 * m;
    const float v = cuboid_sdf_live(row, row[12], row[13], row[14], x, y, z);
    if (v < best) best = v, arg = m;
  }
  for (int m = 0; m < n_cyl; ++m) {
    const float *row = prim_rows + 16 * (64 + m);
    const float v = cylinder_sdf_live(row, row[12], row[13], x, y, z);
    if (v < best) best = v, arg = 64 + m;
  }
  return best;
}

// bits PLAN_BIT_ENV / PLAN_BIT_SELF of one configuration
__device__ __forceinline__ int plan_config_bits(const float *q, float finger, const float *__restrict__ sc,
                                                const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                                                const float *prim_rows, int n_cub, int n_cyl, float reach, bool test_self,
                                                float self_margin) {
  int bits = 0;
  const bool test_env = S > 0 && n_cub + n_cyl > 0;
  franka_fk_visit(q, finger, [&](auto ID, const Rigid &g) __attribute__((always_inline)) {
    constexpr int id = decltype(ID)::value;
    if (test_env) {
      for (int s = 0; s < S; ++s) {
        if (sl[s] != id) continue;  // (wave-uniform)
        float x, y, z;
        rigid_apply(g, sc[3 * s + 0], sc[3 * s + 1], sc[3 * s + 2], x, y, z);
        int arg;
        const float best = plan_min_sdf(prim_rows, n_cub, n_cyl, x, y, z, arg);
        if (best <= sr[s] + reach) bits |= PLAN_BIT_ENV;
      }
    }
    if constexpr (franka_self_sphere(id) >= 0) {
      if (test_self && franka_self_hit<id>(g, self_margin)) bits |= PLAN_BIT_SELF;
    }
  });
  return bits;
}
