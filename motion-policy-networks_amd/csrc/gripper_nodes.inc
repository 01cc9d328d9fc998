// gripper_nodes.inc -- the nodes of a gripper roadmap, thread = node: node 0 the start pose, node 1 the goal pose, node
// v >= 2 a Philox draw (stream 17, keyed by seed / GLOBAL problem id / node): the position in the problem's box, the
// orientation scattered about the start-goal arc.  The clause "Nodes" of mpx_gripper_roadmap's contract
// (include/mpinets_hip.h).  Included as a statement block by gripper_roadmap.hip and gripper_roadmap_cloud.hip: the same
// seed gives the same nodes in both.
//   in scope: tid, b, V, inf, sp, gp (the two poses of problem b), bounds, opt (.orient_spread), seed_lo, seed_hi, env0,
//             float *nodes (V x 7, LDS), float *nodes_out (optional)
//   defines:  ns, ng (the two endpoint nodes, every thread), mine[7] (this thread's node), inside (false: the node is
//             invalid whatever the scene).  The caller's barrier publishes the nodes.
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
