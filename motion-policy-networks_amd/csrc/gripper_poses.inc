// gripper_poses.inc -- the guide poses of a polyline in SE(3): the polyline resampled to W poses at equal steps of its
// metric length (thread = pose), the start not among them, the last one the caller's goal, NaN rows where st != 0.  The clause
// "poses" of mpx_gripper_roadmap's contract (include/mpinets_hip.h).  Included as a statement block, last in the kernel, by
// gripper_tail.inc (the roadmap kernels: the polyline is the path found) and by gripper_shortcut.hip and
// gripper_shortcut_cloud.hip (the polyline returned, path[i] = i); the compiler sees the lines it saw when gripper_tail.inc
// wrote them out (profiles/gripper_shortcut_timing.md has the instruction-stream comparison).
//   in scope: b, tid, W, nan, rot_k, st (0: there is a polyline), hops (its edges), V, float *nodes and int *path (vertex i is
//             nodes[path[i]]), float *dist (2 V, free to overwrite), and the kernel's output poses
//   GRIPPER_POSES_GOAL(o): writes rows 0-2 (12 floats) of the last pose at float *o
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
    GRIPPER_POSES_GOAL(o)
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
