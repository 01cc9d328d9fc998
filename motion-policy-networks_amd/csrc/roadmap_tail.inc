// roadmap_tail.inc -- what a joint-space roadmap kernel does once the search is over: status, hops, rounds, path and edge_state
// go out, then the seed trajectory (roadmap_traj.inc, which the shortcut kernels end with too: the planner's line for a
// one-edge path; else the path resampled by arc length to T waypoints and rounded).  The clauses "path", "edge_state" and "traj" of
// mpx_franka_roadmap's contract (include/mpinets_hip.h).  Included as a statement block, last in the kernel, by roadmap.hip and
// roadmap_cloud.hip; the compiler sees the lines it saw when roadmap.hip wrote them out (profiles/roadmap_cloud_timing.md
// has the instruction-stream comparison).
//   in scope: what roadmap_search.inc takes and defines (V, tid, opt, nodes, dist, path, valid, ebits; st, rounds, hops), b, T,
//             nan, qs[7], qg[7], float *tbuf (2 x 64 x 7), and the kernel's outputs traj, status, path_out, hops_out,
//             edge_out, rounds_out
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

#include "roadmap_traj.inc"
