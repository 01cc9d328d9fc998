// gripper_tail.inc -- the end of a gripper roadmap kernel, from what the search found to the guide poses: status, hops,
// rounds, path and edge_state as mpx_franka_roadmap writes them, then the surviving polyline resampled to W guide poses at
// equal steps of its metric length (thread = pose), the goal copied bit for bit, NaN rows where status != 0.  The clauses
// "Search" (outputs) and "poses" of mpx_gripper_roadmap's contract (include/mpinets_hip.h).  Included as a statement block,
// the last of the kernel's body, by gripper_roadmap.hip and gripper_roadmap_cloud.hip.
//   in scope: what roadmap_search.inc leaves (st, hops, rounds, path, valid, ebits, dist, nodes), tid, b, V, W, nan, rot_k,
//             gp (the goal pose of problem b), poses, status, path_out, hops_out, edge_out, rounds_out
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
