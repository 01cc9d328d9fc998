// follow_device.h -- what franka_follow_kernel (follow.hip) and franka_follow_cloud_kernel (follow_cloud.hip) state once
// beside their statement blocks (follow_state.inc, follow_step_head.inc, follow_step_tail.inc, follow_retime.inc,
// follow_miss.inc): the length of the retiming search, the bits of bad input, a guide pose and the distance to it, and the
// write-out of the state.  Plain inline functions: both kernels keep their instruction streams with them
// (profiles/follow_shared_isa.md).
#pragma once
#include "franka_device.h"
#include "plan_device.h"

constexpr int FOLLOW_BISECT_ROUNDS = 13;  // 2^13 > MPX_FOLLOW_MAX_STEPS: the search interval is one index wide after them
static_assert((1 << FOLLOW_BISECT_ROUNDS) > MPX_FOLLOW_MAX_STEPS, "the retiming search");
static_assert(MPX_FOLLOW_MAX_POSES <= 64 && MPX_PLAN_MAX_T <= 64, "one lane per guide pose / per waypoint");
constexpr int FOLLOW_BAD_BITS = PLAN_BIT_ENV | PLAN_BIT_SELF | PLAN_BIT_JERK | MPX_FOLLOW_BIT_MISS;  // `bits` of status 2

__device__ __forceinline__ void follow_load_pose(const float *__restrict__ tg, float (&Rt)[9], float (&pt)[3]) {
  Rt[0] = tg[0], Rt[1] = tg[1], Rt[2] = tg[2], Rt[3] = tg[4], Rt[4] = tg[5], Rt[5] = tg[6], Rt[6] = tg[8], Rt[7] = tg[9],
  Rt[8] = tg[10];
  pt[0] = tg[3], pt[1] = tg[7], pt[2] = tg[11];
}
__device__ __forceinline__ float follow_distance(const float (&pt)[3], const Rigid &eff) {
  const float dx = pt[0] - eff.t[0], dy = pt[1] - eff.t[1], dz = pt[2] - eff.t[2];
  return sqrtf(mpx_fma(dz, dz, mpx_fma(dy, dy, dx * dx)));
}

// one lane's write-out of problem b's state into the optional q_end, v_end [B,7] and progress_end [B,3]
__device__ __forceinline__ void follow_store_state(int b, const float (&q)[7], const float (&v)[7], int w, int nw, int fin,
                                                   float *__restrict__ q_end, float *__restrict__ v_end,
                                                   int32_t *__restrict__ progress_end) {
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    if (q_end) q_end[(size_t)b * 7 + j] = q[j];
    if (v_end) v_end[(size_t)b * 7 + j] = v[j];
  }
  if (progress_end)
    progress_end[(size_t)b * 3 + 0] = w, progress_end[(size_t)b * 3 + 1] = nw, progress_end[(size_t)b * 3 + 2] = fin;
}
