// roadmap_search.inc -- the lazy search of a roadmap kernel, from "both endpoints are valid" to the status: Jacobi sweeps to a
// fixed point over the edges not known to be blocked, the path walk, the test of the path's untested edges at their interior
// points (thread = interior point, in passes of the workgroup), the verdicts, at most opt.max_rounds rounds.  The clauses
// "Search" of mpx_franka_roadmap's contract (include/mpinets_hip.h).  Included as a statement block by roadmap.hip (nodes are
// joint configurations) and gripper_roadmap.hip (nodes are poses); the compiler sees the lines it saw when roadmap.hip wrote
// them out (profiles/gripper_roadmap_timing.md has the instruction-stream comparison).
//   in scope: V, tid, inf, opt (.connect_radius, .resolution, .max_rounds), float *nodes (V x 7), float mine[7] (this
//             thread's node), float *dist (2 V), int *pred, *path, *rev, *pieces, *blocked, *valid (V each), *first (V + 1),
//             *hops_lds, unsigned *ebits; the helpers of roadmap_device.h
//   ROADMAP_SEARCH_LENGTH(a, b):        the metric between two nodes (const float *), the same bits for (b, a)
//   ROADMAP_SEARCH_POINT(a, e, f, q):   statements that fill float q[7] with the point at fraction f of edge a < e
//   ROADMAP_SEARCH_HIT(q):              that point is invalid
//   defines:  st (0 found, 1 none, 2 an endpoint is invalid), rounds, hops (0 unless st == 0).
// Every branch around a barrier is workgroup-uniform: it reads a value from LDS behind a barrier, or a barrier's own reduction.
int st = (valid[0] && valid[1]) ? 1 : 2, rounds = 0, hops = 0;
for (int round = 0; st == 1 && round < opt.max_rounds; ++round) {
  rounds = round + 1;
  if (tid < V) dist[tid] = tid == 0 ? 0.0f : inf, pred[tid] = -1;
  __syncthreads();
  int cur = 0;
  for (int sweep = 0; sweep < V; ++sweep) {  // (Jacobi: a sweep reads dist[cur], writes the other half; V - 1 suffice)
    const float *dp = dist + cur * V;
    int changed = 0;
    if (tid < V) {
      float best = dp[tid];
      int bp = pred[tid];
      if (tid != 0 && valid[tid]) {
        for (int u = 0; u < V; ++u) {
          const float du = dp[u];
          if (u == tid || !(du < inf) || roadmap_edge_get(ebits, V, u, tid) == ROADMAP_BLOCKED) continue;
          const float w = ROADMAP_SEARCH_LENGTH(nodes + u * 7, mine);
          if (w > opt.connect_radius) continue;
          const float cand = du + w;
          if (cand < best) best = cand, bp = u;
        }
      }
      changed = best < dp[tid];
      dist[(cur ^ 1) * V + tid] = best, pred[tid] = bp;
    }
    cur ^= 1;
    if (!__syncthreads_or(changed)) break;
  }
  if (!(dist[cur * V + 1] < inf)) break;  // the goal cannot be reached over what is not blocked

  // the path, and where each of its untested edges starts among this round's tests
  if (tid == 0) {
    int n = 0, v = 1;
    for (; v > 0 && n < V; v = pred[v]) rev[n++] = v;
    if (v != 0) n = 0;  // (a finite distance has a chain of predecessors down to node 0: never taken)
    path[0] = 0;
    first[0] = 0;
    for (int i = 0; i < n; ++i) {
      path[i + 1] = rev[n - 1 - i];
      const int a = path[i] < path[i + 1] ? path[i] : path[i + 1], c = path[i] < path[i + 1] ? path[i + 1] : path[i];
      pieces[i] = roadmap_pieces(ROADMAP_SEARCH_LENGTH(nodes + a * 7, nodes + c * 7), opt.resolution);
      first[i + 1] = first[i] + (roadmap_edge_get(ebits, V, a, c) == ROADMAP_UNTESTED ? pieces[i] - 1 : 0);
      blocked[i] = 0;
    }
    *hops_lds = n;
  }
  __syncthreads();
  hops = *hops_lds;
  if (hops == 0) break;
  const int total = first[hops];
  for (int c = tid; c < total; c += ROADMAP_THREADS) {  // thread = interior point
    int i = 0, top = hops;                              // the last edge with first[i] <= c
    while (top - i > 1) {
      const int mid = (i + top) >> 1;
      if (first[mid] <= c) i = mid; else top = mid;
    }
    const int a = path[i] < path[i + 1] ? path[i] : path[i + 1], e = path[i] < path[i + 1] ? path[i + 1] : path[i];
    const float f = (float)(c - first[i] + 1) / (float)pieces[i];
    float q[7];
    ROADMAP_SEARCH_POINT(a, e, f, q)
    if (ROADMAP_SEARCH_HIT(q))
      blocked[i] = 1;  // (every lane that stores, stores 1)
  }
  __syncthreads();
  int hit = 0;
  if (tid < hops && roadmap_edge_get(ebits, V, path[tid], path[tid + 1]) == ROADMAP_UNTESTED) {
    hit = blocked[tid];
    roadmap_edge_set(ebits, V, path[tid], path[tid + 1], hit ? ROADMAP_BLOCKED : ROADMAP_FREE);
  }
  if (!__syncthreads_or(hit)) st = 0;
}
if (st != 0) hops = 0;
