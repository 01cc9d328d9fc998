// roadmap_device.h -- what the roadmap kernels share besides the search itself (roadmap_search.inc): the workgroup size, the
// edge states and their 2-bit store in LDS, the pieces of an edge, the joint-space edge length.  roadmap.hip and roadmap_cloud.hip (joint space), gripper_roadmap.hip and gripper_shortcut.hip (SE(3)) and their cloud forms.
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

// LDS of a shortcut kernel behind its primitive rows, in 4-byte words (shortcut_kernel.inc): [two polylines P x 7 | dist 2 x P
// (edge lengths; later cumulative and edge lengths) | two trajectories 64 x 7 | path, sel, pidx, pieces, blocked: P ints each |
// off, first: P + 1 each | ctl 4].  The gripper's shortcut kernels (gripper_shortcut.hip, gripper_shortcut_cloud.hip) end with
// guide poses, not a trajectory: their tbuf has no words.
__host__ __device__ static inline size_t shortcut_lds_words(int P, int tbuf_words = 2 * 64 * 7) {
  return 2 * (size_t)P * 7 + 2 * (size_t)P + (size_t)tbuf_words + 5 * (size_t)P + 2 * ((size_t)P + 1) + 4;
}
// ... and its carving, from `base` on
#define SHORTCUT_LDS_CARVE_T(base, P, TW)                                                                               \
  float *poly = (base);                                                                                                 \
  float *dist = poly + 2 * (P) * 7;                                                                                     \
  float *tbuf = dist + 2 * (P);                                                                                         \
  int *path = reinterpret_cast<int *>(tbuf + (TW));                                                                     \
  int *sel = path + (P), *pidx = sel + (P), *pieces = pidx + (P), *blocked = pieces + (P);                              \
  int *off = blocked + (P), *first = off + (P) + 1, *ctl = first + (P) + 1;
#define SHORTCUT_LDS_CARVE(base, P) SHORTCUT_LDS_CARVE_T(base, P, 2 * 64 * 7)
