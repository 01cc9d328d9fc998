// common.h -- shared host/device helpers for libmpinets_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mpinets_hip.h"
#include "launch_routes.h"

#define MPX_EXPORT extern "C" __attribute__((visibility("default")))

// ---- error plumbing -------------------------------------------------------------------------
void mpx_set_error(const char *fmt, ...);

#define MPX_REQUIRE(cond, ...)        \
  do {                                \
    if (!(cond)) {                    \
      mpx_set_error(__VA_ARGS__);     \
      return 1;                       \
    }                                 \
  } while (0)

// Raises a kernel's dynamic-LDS limit to `bytes` (its largest supported launch) ONCE per (kernel, device): the first
// launch on a device pays the hipFuncSetAttribute, later calls only enqueue.  One static mask per expansion site, so
// use it once per kernel instantiation.
#define MPX_LDS_LIMIT_ONCE(kernel, bytes, what)                                                                \
  do {                                                                                                         \
    static std::atomic<unsigned long long> lds_done_{0};                                                       \
    int dev_ = 0;                                                                                              \
    (void)hipGetDevice(&dev_);                                                                                 \
    const unsigned long long bit_ = 1ull << (dev_ & 63);                                                       \
    if (!(lds_done_.load(std::memory_order_acquire) & bit_)) {                                                 \
      hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),                              \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes));           \
      MPX_REQUIRE(e_ == hipSuccess, "%s: cannot reserve %d B of LDS: %s", what, (int)(bytes), hipGetErrorString(e_)); \
      lds_done_.fetch_or(bit_, std::memory_order_release);                                                     \
    }                                                                                                          \
  } while (0)

#define MPX_LAUNCH_CHECK(name)                                              \
  do {                                                                      \
    hipError_t e_ = hipGetLastError();                                      \
    if (e_ != hipSuccess) {                                                 \
      mpx_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
      return 2;                                                             \
    }                                                                       \
    return 0;                                                               \
  } while (0)

static inline hipStream_t mpx_s(mpx_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
// The 8 unit-queue counters (one per XCD) of `stream` on the current device, zeroed on that stream in front of the launch
// that uses them (unit_queue.hip; nullptr on failure).  Persistent grouped-MLP kernels take their work units from it.
unsigned int *mpx_unit_queue_for(hipStream_t stream, int *exhausted);
int mpx_unit_queue_slots();
void mpx_unit_queue_set_slots(int n);
// CUs of the current device (asked once per device; 0 if the runtime cannot say)
inline int mpx_cu_count() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int n = cus[dev & 63].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
    cus[dev & 63].store(n, std::memory_order_relaxed);
  }
  return n;
}
// THE grouped-MLP modules the fused SA kernels are built for, (C, c1, c2, c3): every dispatch and size query expands this
#define MPX_SA_SHAPES(X) X(1, 64, 64, 64) X(64, 128, 128, 256)
#define MPX_SA_SHAPE_IS(a, b, c, d) (C == a && c1 == b && c2 == c && c3 == d)

// ---- host helpers shared across files ----------------------------------------------------------------------------------
// dense.hip: the segment max-pool's checks and key unpacking (mpx_linear_segmax, dense_bf16.hip's mpx_linear_segmax_bf16x3)
int mpx_segmax_check(const char *name, int M, const int32_t *seg, int64_t Q, int N, const void *keys, const float *pooled,
                     int ldp, const int64_t *arg);
int mpx_segmax_unpack_launch(const unsigned long long *keys, int64_t Q, int N, float *pooled, int ldp, int64_t *arg,
                             hipStream_t stream);
// dense_bf16.hip: the split-bf16 weight-gradient kernel (dense_grad.hip's mpx_linear_wgrad_bf16x3)
void mpx_wgrad_bf16x3_launch(const float *dy, int lddy, const float *x, int ldx, int M, int N, int K, int rows_per_split,
                             int S, float *partial, int with_bias, hipStream_t stream);
// dense_grad.hip: the in-order sum of split partials (train_ops.hip: the sparse pool backward)
void mpx_reduce_partials_launch(const float *partial, int S, int64_t stride, int64_t n, float *out, hipStream_t stream);

// ---- launch slabs ----------------------------------------------------------------------------------------------------
// gridDim.y is limited to 65535, and kernels that reach an operand through a 32-bit buffer offset need it under 4 GB.
// A batched entry point whose batch exceeds one launch walks it in slabs (same kernels, same per-row arithmetic: results
// do not depend on the slabbing) -- the whole of BASELINE configs[4] (65 536 environments) runs on one 288 GB GPU.
constexpr int MPX_GRID_Y = 65535;
// rows one launch of a row-blocked GEMM may cover: <= 65528 blocks of `bm` rows (a multiple of 8 blocks: the XCD-aware
// tile order keeps its shape) and rows * row_bytes < 4 GB when row_bytes > 0
static inline int64_t mpx_row_slab(int bm, int64_t row_bytes) {
  int64_t blocks = 65528;
  if (row_bytes > 0) {
    const int64_t fit = ((((int64_t)1 << 32) - 8192) / row_bytes / bm) & ~(int64_t)7;
    if (fit < blocks) blocks = fit;
  }
  if (blocks < 8) blocks = 8;
  return blocks * bm;
}

// ---- device math with a pinned evaluation order ----------------------------------------------
// Build uses -ffp-contract=off: fused multiply-adds exist only where __builtin_fmaf is written,
// so these helpers evaluate exactly like their restatement in oracle/mpn_oracle.c.

__device__ __forceinline__ float mpx_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// THE squared distance of the index path (FPS, ball query; restated as sqdist() in oracle/mpn_oracle.c -- one definition
// on each side).  pointnet2_ops writes `(x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)` (sampling_gpu.cu,
// ball_query_gpu.cu) and nvcc contracts it (-fmad=true).  LLVM's DAG combiner -- NVVM is built on it -- fuses the LEFT
// multiply of each add first: (a*a + b*b) -> fma(a,a, b*b), then (. + c*c) -> fma(c,c, .), i.e. the product that is
// rounded on its own is dy^2 (profiles/r03_contraction_evidence.md: the x86 and gfx950 disassembly of exactly that
// expression under -ffp-contract=fast).  -DMPX_SQDIST_XFIRST builds the order rounds 1-2 assumed (dx^2 rounded on
// its own) for A/B runs; the two orders pick a different FPS sequence on ~0.2 % of 6272-point clouds
// (tests/test_oracle_pointnet.py::test_contraction_order_ab).  Both forms are monotone in |dx|, |dy|, |dz| (the culled FPS
// kernel's box bound relies on that).
__device__ __forceinline__ float mpx_sqdist(float dx, float dy, float dz) {
#ifdef MPX_SQDIST_XFIRST
  return mpx_fma(dz, dz, mpx_fma(dy, dy, dx * dx));
#else
  return mpx_fma(dz, dz, mpx_fma(dx, dx, dy * dy));
#endif
}

// ---- segmented max-pool in a GEMM epilogue (training: the last layer of a grouped MLP + its max-pool, row N1) ----------
// Rows belong to segments (seg[row], non-decreasing); per (segment, column) the largest activated value and the FIRST row
// attaining it are kept as one 64-bit key {order-preserving bits of the value, ~row} by atomicMax -- the [rows, columns]
// matrix never reaches memory.  keys are zeroed by the launcher (0 is below every real key) and unpacked afterwards.
__device__ __forceinline__ unsigned mpx_ordered_bits(float v) {  // monotone map float -> unsigned
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float mpx_ordered_float(unsigned u) {
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
// the 128 x 128 tile kernels' accumulator layout: a lane holds column col_base + 32 j + l31 of rows
// row_base + 32 i + (r & 3) + 8 (r >> 2) + 4 half, ascending in (i, r).  val(i, j, r) = the activated value.
template <class F>
__device__ __forceinline__ void mpx_segpool_tile(F &&val, int row_base, int col_base, int M, int N, int half, int l31,
                                                 const int32_t *__restrict__ seg, int row0,
                                                 unsigned long long *__restrict__ keys, int ldk) {
  int sg[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row_base + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      sg[i][r] = row < M ? seg[row] : -1;
    }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = col_base + j * 32 + l31;
    if (col >= N) continue;
    int cs = -1;
    unsigned long long best = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int s = sg[i][r];
        if (s < 0) continue;
        const unsigned row = (unsigned)(row0 + row_base + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half);
        const unsigned long long key = ((unsigned long long)mpx_ordered_bits(val(i, j, r)) << 32) | (0xFFFFFFFFu - row);
        if (s != cs) {
          if (cs >= 0) atomicMax(keys + (size_t)cs * ldk + col, best);
          cs = s, best = key;
        } else {
          best = key > best ? key : best;
        }
      }
    if (cs >= 0) atomicMax(keys + (size_t)cs * ldk + col, best);
  }
}

// Cody-Waite by pi/2 + fixed polynomials; |x| up to ~1e3 rad is far more than joint angles need.
__device__ __forceinline__ void mpx_sincos(float x, float &s, float &c) {
  const float TWO_OVER_PI = 0.63661977236758134308f;
  const float PIO2_HI = 1.57079625129699707031f;
  const float PIO2_LO = 7.54978941586159635335e-08f;
  float kf = __builtin_rintf(x * TWO_OVER_PI);
  float r = mpx_fma(-kf, PIO2_HI, x);
  r = mpx_fma(-kf, PIO2_LO, r);
  float r2 = r * r;
  float ps = mpx_fma(r2, 2.7557314297e-06f, -1.9841270114e-04f);
  ps = mpx_fma(ps, r2, 8.3333337680e-03f);
  ps = mpx_fma(ps, r2, -1.6666667163e-01f);
  float sn = mpx_fma(r * r2, ps, r);
  float pc = mpx_fma(r2, -2.7557314297e-07f, 2.4801587642e-05f);
  pc = mpx_fma(pc, r2, -1.3888889225e-03f);
  pc = mpx_fma(pc, r2, 4.1666667908e-02f);
  pc = mpx_fma(pc, r2, -0.5f);
  float cs = mpx_fma(pc, r2, 1.0f);
  int k = ((int)kf) & 3;
  s = (k & 1) ? cs : sn;
  c = (k & 1) ? sn : cs;
  if (k == 1 || k == 2) c = -c;
  if (k >= 2) s = -s;
}

// max of a value with its partner lane 32 apart (lane i <-> i ^ 32), in every lane: one v_permlane32_swap (VALU)
// instead of a ds_bpermute round trip through the LDS crossbar
__device__ __forceinline__ float mpx_max_across_halves(float v) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);  // r[0] = {lo, lo}, r[1] = {hi, hi}
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// ---- the fused set-abstraction kernels' shared vocabulary (sa_mlp.hip: fp32, sa_mlp_bf16.hip: bf16x3) ----------------------
// The vector types, the weight packs' "no channel" marker and the operand-tile loads that both files use.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define PAD_CH (-1)  // "no input channel" in the weight packs' channel maps

// 16-byte buffer load: wave-uniform descriptor + scalar byte offset + per-lane byte offset.  All
// address arithmetic stays on the scalar unit (no 64-bit VGPR pointers to keep alive or spill).
__device__ __forceinline__ float4 bload16(__amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
  const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
  return make_float4(__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w));
}
// the bias of output tile `ot` as an accumulator tile: register r holds channel ot*32 + (r&3) + 8*(r>>2) + 4*half
// (bias_tile: from the weight pack in global memory; bias_tile_lds: from a copy in LDS)
__device__ __forceinline__ f32x16 bias_tile(__amdgpu_buffer_rsrc_t rsrc, int bias_off_bytes, int ot, int half) {
  f32x16 v;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 q = bload16(rsrc, half * 16, bias_off_bytes + (ot * 32 + 8 * g) * 4);
    v[4 * g + 0] = q.x;
    v[4 * g + 1] = q.y;
    v[4 * g + 2] = q.z;
    v[4 * g + 3] = q.w;
  }
  return v;
}
__device__ __forceinline__ f32x16 bias_tile_lds(const float *bias_lds, int ot, int half) {
  f32x16 v;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 q = *reinterpret_cast<const float4 *>(bias_lds + ot * 32 + 8 * g + 4 * half);
    v[4 * g + 0] = q.x;
    v[4 * g + 1] = q.y;
    v[4 * g + 2] = q.z;
    v[4 * g + 3] = q.w;
  }
  return v;
}
