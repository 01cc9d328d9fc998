// roadmap_device.h -- what the roadmap kernels share besides the search itself (roadmap_search.inc): the workgroup size, the
// edge states and their 2-bit store in LDS, the pieces of an edge, the joint-space edge length.  roadmap.hip and roadmap_cloud.hip (joint space), gripper_roadmap.hip (SE(3)).
#pragma once
#include "common.h"

enum { ROADMAP_THREADS = 256, ROADMAP_MAX_PIECES = 1 << 20 };
enum { ROADMAP_UNTESTED = 0, ROADMAP_FREE = 1, ROADMAP_BLOCKED = 2 };
enum { STREAM_ROADMAP = 16 };  // the Philox stream of the joint-space roadmaps' node draws (roadmap.hip, roadmap_cloud.hip)

// |q_b - q_a|: j ascending, the first square rounded on its own, the others fused.  (x - y)^2 is (y - x)^2 bit for bit, so
// the length of an edge does not depend on the order of its ends.
__device__ __forceinline__ float roadmap_length(const float *qa, const float *qb) {
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const float d = qb[j] - qa[j];
    acc = j == 0 ? d * d : mpx_fma(d, d, acc);
  }
  return sqrtf(acc);
}

__device__ __forceinline__ int roadmap_pieces(float w, float resolution) {
  const float n = ceilf(w / resolution);
  return n >= (float)ROADMAP_MAX_PIECES ? ROADMAP_MAX_PIECES : n >= 1.0f ? (int)n : 1;
}

// 2 bits per pair, at bit 2 (lo V + hi) for lo < hi
__device__ __forceinline__ int roadmap_edge_get(const unsigned *bits, int V, int a, int b) {
  const int idx = (a < b ? a : b) * V + (a < b ? b : a);
  return (int)((bits[idx >> 4] >> ((idx & 15) * 2)) & 3u);
}
// (from ROADMAP_UNTESTED only: an OR sets the state, whichever lanes share the word)
__device__ __forceinline__ void roadmap_edge_set(unsigned *bits, int V, int a, int b, int state) {
  const int idx = (a < b ? a : b) * V + (a < b ? b : a);
  atomicOr(&bits[idx >> 4], (unsigned)state << ((idx & 15) * 2));
}
