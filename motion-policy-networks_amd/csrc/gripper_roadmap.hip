// gripper_roadmap.hip -- a lazy probabilistic roadmap per problem for the FREE-FLYING GRIPPER in SE(3): where the reference's
// data generator plans the end effector through the scene with OMPL before it hands the pose path to the fabric
// (data_pipeline/gen_data.py:156-189, plan_end_effector).  A STAND-IN for that planner, NOT a port of it and without any claim
// of parity with AIT*; "valid" means free by this engine's sphere model (the hand and fingertip spheres of the table), not by
// PyBullet's meshes.  V poses (start, goal, V - 2 Philox draws: positions in the problem's box, orientations scattered
// about the start-goal arc) are judged by the planner's own clause (plan_min_sdf on the live rows, franka_self_hit); the
// search is mpx_franka_roadmap's, statement for statement, over the SE(3) metric below; the surviving polyline is resampled
// to W guide poses for mpx_franka_follow.  The contract is stated in include/mpinets_hip.h.
//
// One workgroup of 256 threads per problem, everything in LDS, no scratch memory and no global atomics.  The mappings are
// roadmap.hip's: thread = node (draw, validity, one Jacobi sweep: V <= 256), thread = interior pose across the concatenated
// untested edges of the round's path (passes of 256), thread = output pose (W <= 64).  Every branch around a barrier is
// workgroup-uniform: it reads a value from LDS behind a barrier, or a barrier's own reduction.  The search is the statement
// block both kernels include (roadmap_search.inc), with this file's metric, edge pose and validity.
#include "common.h"
#include "franka_host.h"
#include "plan_prims_device.h"
#include "roadmap_device.h"

enum { STREAM_GRIPPER_ROADMAP = 17 };
enum { GRM_MAX_SPHERES = 64 };

// LDS, in 4-byte words: [128 primitive rows x 16 | gripper spheres 64 x 4 (point in the right_gripper frame, radius) |
// nodes V x 7 | dist 2 x V (later: cumulative and edge lengths) | pred, path, rev, pieces, blocked, valid: V ints each |
// first V + 1 | hops | sphere count | edge bits]
__host__ __device__ static inline size_t gripper_roadmap_lds_words(int V) {
  return (size_t)128 * 16 + (size_t)GRM_MAX_SPHERES * 4 + (size_t)V * 7 + 2 * (size_t)V + 6 * (size_t)V + (size_t)V + 1 + 1 +
         1 + ((size_t)V * V + 15) / 16;
}

// rows 0..2 of a row-major 4x4 pose -> position, unit quaternion (x, y, z, w) by Shepperd's method: the branch is the
// largest of (trace, r00, r11, r22), the first of equal ones in that order; the result is divided by its norm
__device__ __forceinline__ void gripper_pose_node(const float *m, float *node) {
  const float r00 = m[0], r01 = m[1], r02 = m[2], r10 = m[4], r11 = m[5], r12 = m[6], r20 = m[8], r21 = m[9], r22 = m[10];
  const float tr = r00 + r11 + r22;
  float x, y, z, w;
  if (tr >= r00 && tr >= r11 && tr >= r22) {
    const float s = 2.0f * sqrtf(1.0f + tr);
    w = 0.25f * s, x = (r21 - r12) / s, y = (r02 - r20) / s, z = (r10 - r01) / s;
  } else if (r00 >= r11 && r00 >= r22) {
    const float s = 2.0f * sqrtf(1.0f + r00 - r11 - r22);
    x = 0.25f * s, w = (r21 - r12) / s, y = (r01 + r10) / s, z = (r02 + r20) / s;
  } else if (r11 >= r22) {
    const float s = 2.0f * sqrtf(1.0f + r11 - r00 - r22);
    y = 0.25f * s, w = (r02 - r20) / s, x = (r01 + r10) / s, z = (r12 + r21) / s;
  } else {
    const float s = 2.0f * sqrtf(1.0f + r22 - r00 - r11);
    z = 0.25f * s, w = (r10 - r01) / s, x = (r02 + r20) / s, y = (r12 + r21) / s;
  }
  const float n = sqrtf(mpx_fma(w, w, mpx_fma(z, z, mpx_fma(y, y, x * x))));
  node[0] = m[3], node[1] = m[7], node[2] = m[11];
  node[3] = x / n, node[4] = y / n, node[5] = z / n, node[6] = w / n;
}

// unit quaternion (x, y, z, w) and position -> the frame
__device__ __forceinline__ Rigid gripper_frame(const float *node) {
  const float x = node[3], y = node[4], z = node[5], w = node[6];
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  Rigid g;
  g.r[0] = 1.0f - 2.0f * (yy + zz), g.r[1] = 2.0f * (xy - wz), g.r[2] = 2.0f * (xz + wy);
  g.r[3] = 2.0f * (xy + wz), g.r[4] = 1.0f - 2.0f * (xx + zz), g.r[5] = 2.0f * (yz - wx);
  g.r[6] = 2.0f * (xz - wy), g.r[7] = 2.0f * (yz + wx), g.r[8] = 1.0f - 2.0f * (xx + yy);
  g.t[0] = node[0], g.t[1] = node[1], g.t[2] = node[2];
  return g;
}

__device__ __forceinline__ float gripper_dot4(const float *a, const float *b) {
  return mpx_fma(a[3], b[3], mpx_fma(a[2], b[2], mpx_fma(a[1], b[1], a[0] * b[0])));
}

// w_ab: k ascending, the first square rounded on its own, the others fused; positions first, then (2 rot_weight)^2 times
// the squared quaternion chord.  Every term is the same bits for (b,a): products commute, (x - y)^2 = (y - x)^2, and with
// sigma = -1 the chord is a sum.
__device__ __forceinline__ float gripper_length(const float *na, const float *nb, float rot_k) {
  float acc = 0.0f, rq = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = nb[k] - na[k];
    acc = k == 0 ? d * d : mpx_fma(d, d, acc);
  }
  const bool same = gripper_dot4(na + 3, nb + 3) >= 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float d = same ? nb[3 + k] - na[3 + k] : nb[3 + k] + na[3 + k];
    rq = k == 0 ? d * d : mpx_fma(d, d, rq);
  }
  return sqrtf(mpx_fma(rot_k, rq, acc));
}

// the pose at fraction f of the edge from na to nb: positions by fma, orientations by nlerp toward sigma q_b
__device__ __forceinline__ void gripper_edge_pose(const float *na, const float *nb, float f, float *out) {
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = mpx_fma(f, nb[k] - na[k], na[k]);
  const bool same = gripper_dot4(na + 3, nb + 3) >= 0.0f;
  float raw[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) raw[k] = mpx_fma(f, (same ? nb[3 + k] : -nb[3 + k]) - na[3 + k], na[3 + k]);
  const float n = sqrtf(mpx_fma(raw[3], raw[3], mpx_fma(raw[2], raw[2], mpx_fma(raw[1], raw[1], raw[0] * raw[0]))));
#pragma unroll
  for (int k = 0; k < 4; ++k) out[3 + k] = raw[k] / n;
}

// the planner's validity clause on the gripper alone: a sphere with sdf <= r_s + reach, or (test_self) the origin of the
// hand or a fingertip frame inside the body column
__device__ __forceinline__ bool gripper_pose_hit(const float *node, float finger, const float *gsph, int n_g,
                                                 const float *prim_rows, int n_cub, int n_cyl, float reach, bool test_self,
                                                 float self_margin) {
  const Rigid g = gripper_frame(node);
  bool hit = false;
  if (n_cub + n_cyl > 0) {
    for (int s = 0; s < n_g; ++s) {
      float x, y, z;
      rigid_apply(g, gsph[4 * s + 0], gsph[4 * s + 1], gsph[4 * s + 2], x, y, z);
      int arg;
      const float best = plan_min_sdf(prim_rows, n_cub, n_cyl, x, y, z, arg);
      hit |= best <= gsph[4 * s + 3] + reach;
    }
  }
  if (test_self) {  // (the origins of frames 9, 12, 13 in the right_gripper frame: the offsets of the sphere rows below)
    const float tip = (0.0584f + 0.045f) - 0.1f;
    Rigid o = g;
    rigid_apply(g, 0.0f, 0.0f, -0.1f, o.t[0], o.t[1], o.t[2]);
    hit |= franka_self_hit<9>(o, self_margin);
    rigid_apply(g, 0.0f, -finger, tip, o.t[0], o.t[1], o.t[2]);
    hit |= franka_self_hit<12>(o, self_margin);
    rigid_apply(g, 0.0f, finger, tip, o.t[0], o.t[1], o.t[2]);
    hit |= franka_self_hit<13>(o, self_margin);
  }
  return hit;
}

__global__ void __launch_bounds__(ROADMAP_THREADS)
    gripper_roadmap_kernel(const float *__restrict__ start_pose, const float *__restrict__ goal_pose, int W,
                           const float *__restrict__ bounds, float finger, const float *__restrict__ sc,
                           const float *__restrict__ sr, const int32_t *__restrict__ sl, int S,
                           const float *__restrict__ cub_f, const float *__restrict__ cub_d, int M1,
                           const float *__restrict__ cyl_f, const float *__restrict__ cyl_r,
                           const float *__restrict__ cyl_h, int M2, mpx_gripper_roadmap_options opt, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t env0, float *__restrict__ poses, int32_t *__restrict__ status,
                           int32_t *__restrict__ path_out, int32_t *__restrict__ hops_out, float *__restrict__ nodes_out,
                           uint8_t *__restrict__ edge_out, int32_t *__restrict__ rounds_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int V = opt.nodes;
  float *prim_rows = lds;
  float *gsph = prim_rows + 128 * 16;
  float *nodes = gsph + GRM_MAX_SPHERES * 4;
  float *dist = nodes + V * 7;
  int *pred = reinterpret_cast<int *>(dist + 2 * V);
  int *path = pred + V, *rev = path + V, *pieces = rev + V, *blocked = pieces + V, *valid = blocked + V;
  int *first = valid + V;  // first[i]: index of edge i's first interior pose among the round's tests
  int *hops_lds = first + V + 1;
  int *ng_lds = hops_lds + 1;
  unsigned *ebits = reinterpret_cast<unsigned *>(ng_lds + 1);
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int k = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float inf = __builtin_inff(), nan = __builtin_nanf("");
  const float *sp = start_pose + (size_t)b * 16, *gp = goal_pose + (size_t)b * 16;

#define FRANKA_LIVE_ROWS_STORE (k == 0)
#include "franka_live_rows.inc"
#undef FRANKA_LIVE_ROWS_STORE
  for (int i = tid; i < (V * V + 15) / 16; i += ROADMAP_THREADS) ebits[i] = 0u;

  // the gripper's rows of the sphere table (links 9, 12, 13), in table order, as points of the right_gripper frame:
  // a point h of the hand frame sits at (-h_x, -h_y, h_z - 0.1); a fingertip frame is the hand frame shifted by
  // (0, +-finger, 0.0584 + 0.045).  Wave 1 lane s takes row s (S <= 64).
  if (k == 1) {
    const int link = lane < S ? sl[lane] : -1;
    const bool mine_g = link == 9 || link == 12 || link == 13;
    const unsigned long long gmask = __builtin_amdgcn_ballot_w64(mine_g);
    if (mine_g) {
      float *dst = gsph + 4 * __builtin_popcountll(gmask & (((unsigned long long)1 << lane) - 1));
      const float hy = link == 12 ? sc[3 * lane + 1] + finger : link == 13 ? sc[3 * lane + 1] - finger : sc[3 * lane + 1];
      const float hz = link == 9 ? sc[3 * lane + 2] : sc[3 * lane + 2] + (0.0584f + 0.045f);
      dst[0] = -sc[3 * lane + 0], dst[1] = -hy, dst[2] = hz - 0.1f, dst[3] = sr[lane];
    }
    if (lane == 0) *ng_lds = __builtin_popcountll(gmask);
  }

  // ---- nodes: thread = node ------------------------------------------------------------------------------------------------------
  float ns[7], ng[7];  // (every thread: the draw mixes the two orientations)
  gripper_pose_node(sp, ns);
  gripper_pose_node(gp, ng);
  float mine[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  bool inside = true;
  if (tid < V) {
    if (tid < 2) {
      const float *m = tid == 0 ? sp : gp;
#pragma unroll
      for (int j = 0; j < 7; ++j) mine[j] = tid == 0 ? ns[j] : ng[j];
#pragma unroll
      for (int i = 0; i < 12; ++i) inside &= __builtin_fabsf(m[i]) < inf;  // (NaN fails)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        inside &= (mine[j] >= bounds[(size_t)b * 6 + j]) & (mine[j] <= bounds[(size_t)b * 6 + 3 + j]);
    } else {
      const Philox p0 = philox4x32(2u * (uint32_t)tid, env0 + (uint32_t)b, STREAM_GRIPPER_ROADMAP, 0u, seed_lo, seed_hi);
      const Philox p1 = philox4x32(2u * (uint32_t)tid + 1u, env0 + (uint32_t)b, STREAM_GRIPPER_ROADMAP, 0u, seed_lo, seed_hi);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float lo = bounds[(size_t)b * 6 + j], hi = bounds[(size_t)b * 6 + 3 + j];
        mine[j] = mpx_fma(u01(p0.c[j]), hi - lo, lo);
      }
      const float u = u01(p0.c[3]);
      const bool same = gripper_dot4(ns + 3, ng + 3) >= 0.0f;
      float raw[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float m = mpx_fma(u, (same ? ng[3 + j] : -ng[3 + j]) - ns[3 + j], ns[3 + j]);
        raw[j] = mpx_fma(opt.orient_spread, mpx_fma(2.0f, u01(p1.c[j]), -1.0f), m);
      }
      const float n2 = mpx_fma(raw[3], raw[3], mpx_fma(raw[2], raw[2], mpx_fma(raw[1], raw[1], raw[0] * raw[0])));
      inside = n2 >= 9.5367431640625e-07f;  // 2^-20 (NaN fails)
      const float n = sqrtf(n2);
#pragma unroll
      for (int j = 0; j < 4; ++j) mine[3 + j] = raw[j] / n;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      nodes[tid * 7 + j] = mine[j];
      if (nodes_out) nodes_out[((size_t)b * V + tid) * 7 + j] = mine[j];
    }
  }
  __syncthreads();  // (the primitive rows, the gripper spheres, the nodes, the cleared edge bits)

  const int n_g = *ng_lds;
  const bool test_self = opt.check_self != 0;
  const float reach = opt.clearance + opt.check_margin;
  const float two_rw = 2.0f * opt.rot_weight, rot_k = two_rw * two_rw;
  if (tid < V)
    valid[tid] = inside && !gripper_pose_hit(mine, finger, gsph, n_g, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin);
  __syncthreads();

  // ---- the lazy search: roadmap.hip's, over the SE(3) metric and the gripper's validity ----------------------------------------------
#define ROADMAP_SEARCH_LENGTH(a, b) gripper_length(a, b, rot_k)
#define ROADMAP_SEARCH_POINT(a, e, f, q) gripper_edge_pose(nodes + a * 7, nodes + e * 7, f, q);
#define ROADMAP_SEARCH_HIT(q) \
  gripper_pose_hit(q, finger, gsph, n_g, prim_rows, n_cub, n_cyl, reach, test_self, opt.check_margin)
#include "roadmap_search.inc"
#undef ROADMAP_SEARCH_LENGTH
#undef ROADMAP_SEARCH_POINT
#undef ROADMAP_SEARCH_HIT

  // ---- what the search found -----------------------------------------------------------------------------------------------------
  if (tid == 0) {
    status[b] = st, hops_out[b] = hops;
    if (rounds_out) rounds_out[b] = rounds;
  }
  if (tid < V) path_out[(size_t)b * V + tid] = (st == 0 && tid <= hops) ? path[tid] : -1;
  if (edge_out)
    for (int i = tid; i < V * V; i += ROADMAP_THREADS) {
      const int a = i / V, c = i - a * V;
      edge_out[(size_t)b * V * V + i] =
          (uint8_t)(a == c ? (valid[a] ? ROADMAP_FREE : ROADMAP_BLOCKED) : roadmap_edge_get(ebits, V, a, c));
    }

  // ---- the guide poses: thread = pose --------------------------------------------------------------------------------------------
  float *out = poses + (size_t)b * W * 16;
  if (st != 0) {
    for (int i = tid; i < W * 16; i += ROADMAP_THREADS) out[i] = nan;
    return;
  }
  float *cum = dist, *len = dist + V;  // (the search is over: cum[i] = metric length at path node i, len[i] = w of edge i)
  __syncthreads();
  if (tid == 0) {
    cum[0] = 0.0f;
    for (int i = 0; i < hops; ++i) {
      len[i] = gripper_length(nodes + path[i] * 7, nodes + path[i + 1] * 7, rot_k);
      cum[i + 1] = cum[i] + len[i];
    }
  }
  __syncthreads();
  if (tid < W) {
    float *o = out + tid * 16;
    if (tid == W - 1) {  // the goal as given
#pragma unroll
      for (int i = 0; i < 12; ++i) o[i] = gp[i];
    } else {
      const float s = ((float)(tid + 1) / (float)W) * cum[hops];
      int i = 0;
      for (int e = 1; e < hops; ++e)
        if (cum[e] <= s) i = e;
      const float f = len[i] > 0.0f ? fminf((s - cum[i]) / len[i], 1.0f) : 0.0f;
      float q[7];
      gripper_edge_pose(nodes + path[i] * 7, nodes + path[i + 1] * 7, f, q);
      const Rigid g = gripper_frame(q);
#pragma unroll
      for (int r = 0; r < 3; ++r) o[4 * r + 0] = g.r[3 * r + 0], o[4 * r + 1] = g.r[3 * r + 1], o[4 * r + 2] = g.r[3 * r + 2], o[4 * r + 3] = g.t[r];
    }
    o[12] = 0.0f, o[13] = 0.0f, o[14] = 0.0f, o[15] = 1.0f;
  }
}

MPX_EXPORT int mpx_gripper_roadmap(const float *start_pose, const float *goal_pose, int B, int W, const float *bounds,
                                   float finger, const float *sph_centers, const float *sph_radii, const int32_t *sph_link,
                                   int S, const float *cub_inv_frames, const float *cub_dims, int M1,
                                   const float *cyl_inv_frames, const float *cyl_radii, const float *cyl_heights, int M2,
                                   const mpx_gripper_roadmap_options *options, uint64_t seed, int64_t env_offset, float *poses,
                                   int32_t *status, int32_t *path, int32_t *hops, float *nodes, uint8_t *edge_state,
                                   int32_t *rounds, mpx_stream_t stream) {
  const char *who = "mpx_gripper_roadmap";
  const mpx_gripper_roadmap_options opt = options ? *options : gripper_roadmap_defaults();
  MPX_REQUIRE(B >= 0 && S >= 0 && M1 >= 0 && M2 >= 0, "%s: negative size", who);
  if (gripper_roadmap_options_check(who, W, opt) || franka_counts_check(who, S, M1, M2) ||
      franka_env_offset_check(who, env_offset, B) || franka_rows_check(who, B, W * 16, "B x W x 16 pose entries"))
    return 1;
  if (B == 0) return 0;
  MPX_REQUIRE(poses && status && path && hops, "%s: NULL output (poses, status, path, hops)", who);
  MPX_REQUIRE(start_pose && goal_pose && bounds, "%s: NULL operand (start_pose, goal_pose, bounds)", who);
  if (franka_sphere_table_check(who, S, sph_centers, sph_radii, sph_link) ||
      franka_primitive_arrays_check(who, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames, cyl_radii, cyl_heights, M2))
    return 1;
  const size_t lds = 4 * gripper_roadmap_lds_words(opt.nodes);  // 41 996 B at 256 nodes
  hipLaunchKernelGGL(gripper_roadmap_kernel, dim3((unsigned)B), dim3(ROADMAP_THREADS), lds, mpx_s(stream), start_pose, goal_pose,
                     W, bounds, finger, sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames,
                     cyl_radii, cyl_heights, M2, opt, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env_offset, poses,
                     status, path, hops, nodes, edge_state, rounds);
  MPX_LAUNCH_CHECK(who);
}
