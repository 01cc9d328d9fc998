// gripper_tail.inc -- the end of a gripper roadmap kernel, from what the search found to the guide poses: status, hops,
// rounds, path and edge_state as mpx_franka_roadmap writes them, then the guide poses over the surviving polyline
// (gripper_poses.inc, which the gripper's shortcut kernels end with too), the goal copied bit for bit.  The clauses "Search"
// (outputs) and "poses" of mpx_gripper_roadmap's contract (include/mpinets_hip.h).  Included as a statement block, the last
// of the kernel's body, by gripper_roadmap.hip and gripper_roadmap_cloud.hip.
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


#define GRIPPER_POSES_GOAL(o) _Pragma("unroll") for (int i = 0; i < 12; ++i) o[i] = gp[i];
#include "gripper_poses.inc"
#undef GRIPPER_POSES_GOAL
