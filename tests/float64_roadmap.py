"""Restatement of ``mpx_franka_roadmap`` and of ``mpx_franka_plan_seeded`` on the CPU, in float64 by default, written from
the contract in include/mpinets_hip.h (not from csrc/roadmap.hip): the node draws (Philox4x32-10 keyed by (seed, global
problem id, node), stream 16), edges cut into pieces of at most ``resolution``, the lazy search by Jacobi sweeps, the
resampled and corner-filtered seed trajectory, and the seeded optimiser as ``float64_plan.solve`` with one more candidate.

Built on tests/float64_plan.py: ``config_bits`` judges a configuration (the planner's validity test), ``line`` is the
one-edge trajectory, ``refine`` / ``validity`` / ``solve`` judge and optimise a seed.  ``search`` takes the validity test
as a callable, so a planar toy can stand in for the robot.  ``dtype=np.float32`` runs the same statements in float32: the
reference-against-reference measurement that sets the bar of the GPU seed-trajectory test.
"""
import heapq

import numpy as np
import torch

import float64_plan as fp
from float64_ik import limits32, philox4x32_np
from mpinets_amd import franka_tables as ft

STREAM_ROADMAP = 16
MAX_NODES = 256
MAX_PIECES = 1 << 20
# MPX_ROADMAP_DEFAULT_* of include/mpinets_hip.h
DEFAULTS = dict(nodes=64, resolution=0.05, connect_radius=float("inf"), max_rounds=64, smooth_passes=8, check_margin=1e-4,
                clearance=0.0, check_self=True)
UNTESTED, FREE, BLOCKED = 0, 1, 2


def fma32(a, b, c):
    """float32 fma(a, b, c) through float64: the product of two float32 is exact there; the sum is rounded once to float64
    and once to float32 (a double rounding can differ from the fused result only on an exact float32 tie of the float64 sum)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def draw_nodes(q_start, q_goal, limits=ft.JOINT_LIMITS_REAL, V=64, seed=0, env_offset=0):
    """-> float32 [B,V,7]: node 0 = q_start, node 1 = q_goal, node v >= 2 = fma(u, hi - lo, lo), the device's bits."""
    qs, qg = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    B = qs.shape[0]
    lim = limits32(limits)
    lo, hi = lim[:, 0], lim[:, 1]
    v = np.arange(V, dtype=np.uint64)[None, :]
    gid = ((env_offset + np.arange(B, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))[:, None]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r0 = philox4x32_np(2 * v, gid, STREAM_ROADMAP, 0, k0, k1)
    r1 = philox4x32_np(2 * v + 1, gid, STREAM_ROADMAP, 0, k0, k1)
    bits = np.stack(list(r0) + list(r1[:3]), axis=-1)  # [B,V,7]
    u = (bits >> np.uint32(8)).astype(np.float32) * np.float32(5.9604644775390625e-08)
    nodes = fma32(u, hi - lo, lo)
    nodes[:, 0] = qs
    if V > 1:
        nodes[:, 1] = qg
    return nodes


def lengths(nodes, dtype=np.float64):
    """[V,7] -> W [V,V] in ``dtype``: the 2-norm of the joint difference, j ascending."""
    q = np.asarray(nodes).astype(dtype)
    d = q[None, :, :] - q[:, None, :]
    acc = np.zeros(d.shape[:2], dtype)
    for j in range(7):
        acc = acc + d[..., j] * d[..., j]
    return np.sqrt(acc)


def pieces(w, resolution, dtype=np.float64):
    n = np.ceil(dtype(w) / dtype(resolution))
    return int(min(MAX_PIECES, max(1.0, n)))


def edge_configs(qa, qb, n, dtype=np.float64):
    """The interior configurations i = 1 .. n-1 of the edge from ``qa`` to ``qb`` (a < b): [n-1,7].  float32: the device's
    fma((float)i / (float)n, d, q_a)."""
    if dtype == np.float32:
        f = (np.arange(1, n, dtype=np.float32) / np.float32(n))[:, None]
        return fma32(f, (qb.astype(np.float32) - qa.astype(np.float32))[None], qa.astype(np.float32)[None])
    f = (np.arange(1, n, dtype=dtype) / dtype(n))[:, None]
    return qa.astype(dtype)[None] + f * (qb.astype(dtype) - qa.astype(dtype))[None]


def sweeps(W, usable, valid):
    """Jacobi sweeps to a fixed point as the header states them -> dist [V], pred [V] (-1: none).  ``usable`` [V,V] bool:
    the edge exists and is not blocked."""
    V = W.shape[0]
    dist = np.full(V, np.inf, W.dtype)
    dist[0] = 0
    pred = np.full(V, -1, np.int64)
    for _ in range(V):
        cand = np.where(usable & valid[:, None] & valid[None, :], dist[:, None] + W, np.inf)  # [u,v]
        np.fill_diagonal(cand, np.inf)
        cand[:, 0] = np.inf
        best = cand.min(axis=0)
        arg = cand.argmin(axis=0)  # (the first of equal values: the lowest u)
        lower = best < dist
        if not lower.any():
            break
        pred = np.where(lower, arg, pred)
        dist = np.where(lower, best, dist)
    return dist, pred


def search(nodes, is_valid, resolution=0.05, connect_radius=float("inf"), max_rounds=64, dtype=np.float64):
    """The lazy search on one problem.  ``nodes`` [V,7] float32; ``is_valid(q [N,7] in dtype) -> bool [N]``.
    -> status (0 / 1 / 2), path (list of node indices, empty unless status 0), edge_state uint8 [V,V], rounds."""
    nodes = np.asarray(nodes, np.float32)
    V = nodes.shape[0]
    valid = np.asarray(is_valid(nodes.astype(dtype)), bool)
    state = np.zeros((V, V), np.uint8)
    state[np.arange(V), np.arange(V)] = np.where(valid, FREE, BLOCKED)
    if not (valid[0] and valid[1]):
        return 2, [], state, 0
    W = lengths(nodes, dtype)
    exists = W <= connect_radius
    for rnd in range(1, max_rounds + 1):
        dist, pred = sweeps(W, exists & (state != BLOCKED), valid)
        if not np.isfinite(dist[1]):
            return 1, [], state, rnd
        path = [1]
        while path[-1] != 0:
            path.append(int(pred[path[-1]]))
        path.reverse()
        todo, configs = [], []
        for u, v in zip(path[:-1], path[1:]):
            a, b = min(u, v), max(u, v)
            if state[a, b] == UNTESTED:
                c = edge_configs(nodes[a], nodes[b], pieces(W[a, b], resolution, dtype), dtype)
                todo.append((a, b, len(c)))
                configs.append(c)
        any_blocked = False
        if todo:
            flat = np.concatenate(configs, 0)
            ok = np.asarray(is_valid(flat), bool) if len(flat) else np.zeros(0, bool)
            at = 0
            for a, b, n in todo:
                free = bool(ok[at:at + n].all())
                at += n
                state[a, b] = state[b, a] = FREE if free else BLOCKED
                any_blocked |= not free
        if not any_blocked:
            return 0, path, state, rnd
    return 1, [], state, max_rounds


def resample(points, T, dtype=np.float64):
    """The polyline through ``points`` [H+1,7] at arc lengths t / (T-1) x total, cumulative lengths summed in path order ->
    [T,7] in ``dtype`` (waypoints 0 and T-1 are the end points themselves)."""
    p = np.asarray(points).astype(dtype)
    d = p[1:] - p[:-1]
    acc = np.zeros(len(d), dtype)
    for j in range(7):
        acc = acc + d[:, j] * d[:, j]
    w = np.sqrt(acc)
    c = np.zeros(len(p), dtype)
    for i in range(len(w)):
        c[i + 1] = c[i] + w[i]
    s = (np.arange(T, dtype=dtype) / dtype(T - 1)) * c[-1]
    seg = np.clip(np.searchsorted(c[:-1], s, side="right") - 1, 0, len(w) - 1)  # the last edge with c_i <= s
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(w[seg] > 0, np.minimum((s - c[seg]) / w[seg], dtype(1)), dtype(0)).astype(dtype)
    out = p[seg] + f[:, None] * d[seg]
    out[0], out[-1] = p[0], p[-1]
    return out


def smooth(traj, passes, dtype=np.float64):
    q = np.asarray(traj).astype(dtype)
    for _ in range(passes):
        new = q.copy()
        new[1:-1] = dtype(0.25) * (q[:-2] + q[2:]) + dtype(0.5) * q[1:-1]
        q = new
    return q


def seed_trajectory(nodes, path, T, smooth_passes, dtype=np.float64):
    """-> [T,7]: ``float64_plan.line`` (float32 bits, cast) for a one-edge path, else the resampled, filtered polyline."""
    nodes = np.asarray(nodes, np.float32)
    if len(path) == 2:
        return fp.line(nodes[path[0]][None], nodes[path[1]][None], T)[0].astype(dtype)
    return smooth(resample(nodes[np.asarray(path)], T, dtype), smooth_passes, dtype)


def franka_validity(scene_b, reach, check_self, self_margin, with_base_link=False):
    """-> ``is_valid`` of one problem (scene arrays with a leading batch axis of 1, or None)."""
    def is_valid(q):
        q = torch.from_numpy(np.ascontiguousarray(q))
        if q.shape[0] == 0:
            return np.zeros(0, bool)
        return (fp.config_bits(q, scene_b, q.shape[0], reach, check_self, self_margin, with_base_link) == 0).numpy()
    return is_valid


def solve(q_start, q_goal, scene=None, limits=ft.JOINT_LIMITS_REAL, T=50, seed=0, env_offset=0, dtype=np.float64,
          with_base_link=False, **options):
    """-> traj [B,T,7] (NaN rows where status != 0), status [B], path [B,V] (-1 padded), hops [B], nodes float32 [B,V,7],
    edge_state uint8 [B,V,V], rounds [B]: like ``robot.franka_roadmap`` with ``return_graph``."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    V = opt["nodes"]
    qs, qg = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    B = qs.shape[0]
    lim = limits32(limits)
    nodes = draw_nodes(qs, qg, limits, V, seed, env_offset)
    traj = np.full((B, T, 7), np.nan, dtype)
    status, hops, rounds = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    path = np.full((B, V), -1, np.int32)
    edge_state = np.zeros((B, V, V), np.uint8)
    for b in range(B):
        sc = None if scene is None else {k: v[b:b + 1] for k, v in scene.items()}
        base = franka_validity(sc, opt["clearance"] + opt["check_margin"], opt["check_self"], opt["check_margin"], with_base_link)
        ends = nodes[b, :2]
        inside = bool(((ends >= lim[:, 0]) & (ends <= lim[:, 1])).all())  # (NaN fails)

        def is_valid(q, base=base):
            return base(np.nan_to_num(q))

        if not inside:
            status[b] = 2
            v = is_valid(nodes[b].astype(dtype))
            v[:2] &= ((ends >= lim[:, 0]) & (ends <= lim[:, 1])).all(-1)
            edge_state[b][np.arange(V), np.arange(V)] = np.where(v, FREE, BLOCKED)
            continue
        st, p, es, r = search(nodes[b], is_valid, opt["resolution"], opt["connect_radius"], opt["max_rounds"], dtype)
        status[b], edge_state[b], rounds[b] = st, es, r
        if st == 0:
            hops[b] = len(p) - 1
            path[b, :len(p)] = p
            traj[b] = seed_trajectory(nodes[b], p, T, opt["smooth_passes"], dtype)
    return traj, status, path, hops, nodes, edge_state, rounds


def dijkstra_cost(nodes, edge_state, connect_radius=float("inf")):
    """The float64 cost of the shortest path from node 0 to node 1 over "valid nodes, edges not in state 2" of the given
    ``edge_state`` [V,V] (+inf: unreachable).  A heap, not the sweeps: an independent route to the same number."""
    V = len(nodes)
    W = lengths(nodes, np.float64)
    valid = edge_state[np.arange(V), np.arange(V)] == FREE
    if not (valid[0] and valid[1]):
        return float("inf")
    dist = np.full(V, np.inf)
    dist[0] = 0.0
    heap, done = [(0.0, 0)], np.zeros(V, bool)
    while heap:
        d, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        if u == 1:
            return d
        ok = valid & ~done & (edge_state[u] != BLOCKED) & (W[u] <= connect_radius)
        for v in np.flatnonzero(ok):
            nd = d + W[u, v]
            if nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, int(v)))
    return float("inf")


def path_cost(nodes, path):
    p = np.asarray(nodes, np.float64)[np.asarray(path)]
    return float(np.sqrt(((p[1:] - p[:-1]) ** 2).sum(-1)).sum())


def solve_seeded(q_start, q_goal, seeds, scene=None, limits=ft.JOINT_LIMITS_REAL, T=50, seed=0, env_offset=0,
                 dtype=torch.float64, with_base_link=False, chunk=64, **options):
    """``mpx_franka_plan_seeded``: ``float64_plan.solve`` from the drawn candidates followed by ``seeds`` [B,Ks,T,7] (interior
    clamped into the limits, endpoints replaced); a seed with a non-finite entry ends with NaN rows and bits 7 and cannot
    win.  -> what ``float64_plan.solve`` returns, over K + Ks candidates."""
    opt = dict(fp.DEFAULTS, **options)
    K = opt["candidates"]
    qs, qg = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    seeds = np.asarray(seeds, np.float32)
    B, Ks = seeds.shape[:2]
    lim = limits32(limits)
    drawn = fp.candidates(qs, qg, limits, T, K, opt["spread"], seed, env_offset)
    L = fp.line(qs, qg, T)
    dead = ~np.isfinite(seeds).all(axis=(2, 3))  # [B,Ks]
    sd = np.where(dead[:, :, None, None], L[:, None], np.minimum(np.maximum(seeds, lim[:, 0]), lim[:, 1])).astype(np.float32)
    sd[:, :, 0], sd[:, :, -1] = L[:, None, 0], L[:, None, -1]
    start = np.concatenate([drawn, sd], 1)
    _, status, _, all_traj, all_bits = fp.solve(qs, qg, scene, limits, T, seed, env_offset, dtype, with_base_link, chunk,
                                                start=start, **dict(options, candidates=K + Ks))
    planned = status != 2
    kill = np.zeros((B, K + Ks), bool)
    kill[:, K:] = dead
    kill &= planned[:, None]
    all_bits[kill] = fp.BIT_ENV | fp.BIT_SELF | fp.BIT_JERK
    all_traj[kill] = np.nan
    traj, st, choice = fp.pick(all_traj, all_bits)
    traj[~planned], st[~planned], choice[~planned] = np.nan, 2, -1
    return traj, st, choice, all_traj, all_bits
