// field_device.h -- the distance field as the kernels that read it take it: the grid (mpx_field_grid with inv_h formed once
// on the host), its host-side check, and the trilinear sampler of include/mpinets_hip.h.  cloud_field.hip (the build, the
// sample entry, the planner's cost) and roadmap_cloud.hip (the roadmap's validity test) use this one text.
#pragma once
#include "common.h"

struct FieldGrid {  // mpx_field_grid as the kernels take it (inv_h formed once on the host)
  float lox, loy, loz, h, inv_h, trunc;
  int nx, ny, nz;
};

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

static inline int field_grid_check(const char *who, const mpx_field_grid *grid, FieldGrid &G) {
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
