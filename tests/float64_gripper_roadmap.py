"""Restatement of ``mpx_gripper_roadmap`` on the CPU, in float64 by default, written from the contract in
include/mpinets_hip.h (not from csrc/gripper_roadmap.hip): the node draws (Philox4x32-10 keyed by (seed, global problem id,
node), stream 17, on a float32 path of their own as ``float64_roadmap.draw_nodes`` has), the placement of the gripper's spheres
from a pose, the validity clause, the SE(3) metric, pieces and nlerp of an edge, the lazy search (``float64_roadmap.sweeps``,
which only sees a weight matrix), the resampling to guide poses, and a Dijkstra cost over a given ``edge_state``.

A stand-in's restatement: like the kernel it claims nothing about the reference's OMPL planner.  ``dtype=np.float32`` runs the
placement and the edge poses as the device rounds them: the reference-against-reference measurement behind ``GRIPPER_BAND``
(tests/test_gripper_roadmap_host.py).  The three scenarios of the GPU tests (wall, cylinder, free space) are built here so
that the CPU test that chooses their seed and the GPU tests use the same problems.
"""
import heapq

import numpy as np
import torch

import float64_plan as fp
import float64_roadmap as fr
from float64_ik import philox4x32_np
from float64_roadmap import BLOCKED, FREE, UNTESTED, fma32
from mpinets_amd import franka_tables as ft

STREAM_GRIPPER_ROADMAP = 17
MAX_PIECES = 1 << 20
# MPX_GRIPPER_ROADMAP_DEFAULT_* of include/mpinets_hip.h
DEFAULTS = dict(nodes=64, resolution=0.01, rot_weight=0.12, orient_spread=0.5, connect_radius=float("inf"), max_rounds=256,
                check_margin=1e-4, clearance=0.0, check_self=True)
BOUNDS_PAD = 0.3
GRIPPER_LINKS = (9, 12, 13)
F32 = np.float32


# ---- quaternions (x, y, z, w) --------------------------------------------------------------------------------------------------
def dot4(a, b, dtype=np.float64):
    """fma(a_3, b_3, fma(a_2, b_2, fma(a_1, b_1, a_0 b_0))) over the last axis."""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    if dtype == np.float32:
        acc = a[..., 0] * b[..., 0]
        for k in (1, 2, 3):
            acc = fma32(a[..., k], b[..., k], acc)
        return acc
    return (a * b).sum(-1)


def pose_nodes(M, dtype=np.float64):
    """[N,4,4] poses -> [N,7] (p, q): Shepperd's method with the header's branch rule (the first of trace, R00, R11, R22 that
    is >= the other three), then divided by the norm.  ``dtype`` is the arithmetic; float32 is the device's (which reads
    float32 matrices: cast them before the call where that is meant)."""
    M = np.asarray(M).astype(dtype)
    R = M[:, :3, :3]
    r00, r11, r22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = r00 + r11 + r22
    one, two, quarter = dtype(1), dtype(2), dtype(0.25)
    with np.errstate(invalid="ignore", divide="ignore"):
        s0 = two * np.sqrt(one + tr)
        b0 = np.stack([(R[:, 2, 1] - R[:, 1, 2]) / s0, (R[:, 0, 2] - R[:, 2, 0]) / s0, (R[:, 1, 0] - R[:, 0, 1]) / s0, quarter * s0], -1)
        s1 = two * np.sqrt(one + r00 - r11 - r22)
        b1 = np.stack([quarter * s1, (R[:, 0, 1] + R[:, 1, 0]) / s1, (R[:, 0, 2] + R[:, 2, 0]) / s1, (R[:, 2, 1] - R[:, 1, 2]) / s1], -1)
        s2 = two * np.sqrt(one + r11 - r00 - r22)
        b2 = np.stack([(R[:, 0, 1] + R[:, 1, 0]) / s2, quarter * s2, (R[:, 1, 2] + R[:, 2, 1]) / s2, (R[:, 0, 2] - R[:, 2, 0]) / s2], -1)
        s3 = two * np.sqrt(one + r22 - r00 - r11)
        b3 = np.stack([(R[:, 0, 2] + R[:, 2, 0]) / s3, (R[:, 1, 2] + R[:, 2, 1]) / s3, quarter * s3, (R[:, 1, 0] - R[:, 0, 1]) / s3], -1)
        c0 = (tr >= r00) & (tr >= r11) & (tr >= r22)
        c1 = ~c0 & (r00 >= r11) & (r00 >= r22)
        c2 = ~c0 & ~c1 & (r11 >= r22)
        q = np.where(c0[:, None], b0, np.where(c1[:, None], b1, np.where(c2[:, None], b2, b3))).astype(dtype)
        q = q / np.sqrt(dot4(q, q, dtype))[:, None]
    return np.concatenate([M[:, :3, 3], q], -1).astype(dtype)


def rotation(q):
    """Unit quaternions [...,4] -> R [...,3,3], the header's formula, in the dtype of q."""
    x, y, z, w = (q[..., i] for i in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def pose_matrix(node):
    """(p, q) [...,7] -> [...,4,4] in the dtype of ``node``."""
    M = np.zeros(node.shape[:-1] + (4, 4), node.dtype)
    M[..., :3, :3] = rotation(node[..., 3:])
    M[..., :3, 3] = node[..., :3]
    M[..., 3, 3] = 1
    return M


# ---- the gripper's spheres -----------------------------------------------------------------------------------------------------
def gripper_points(finger=ft.FINGER_OPENING, dtype=np.float64, with_base_link=False):
    """-> (points [G,3] in the right_gripper frame, radii [G], rows of the sphere table [G], frame origins [3,3] of links
    9 / 12 / 13 in the right_gripper frame).  float64: the decimal constants of the URDF; float32: the device's."""
    c, r, l, _ = ft.collision_sphere_table(with_base_link)
    rows = np.flatnonzero(np.isin(l, GRIPPER_LINKS))
    tip_z = dtype(0.0584) + dtype(0.045)
    off = {9: np.zeros(3, dtype), 12: np.array([0, dtype(finger), tip_z], dtype), 13: np.array([0, -dtype(finger), tip_z], dtype)}

    def to_gripper(h):
        return np.stack([-h[..., 0], -h[..., 1], h[..., 2] - dtype(0.1)], -1).astype(dtype)

    h = c[rows].astype(dtype) + np.stack([off[int(k)] for k in l[rows]])
    origins = to_gripper(np.stack([off[k] for k in GRIPPER_LINKS]))
    return to_gripper(h), r[rows].astype(dtype), rows, origins


def place(nodes, points, dtype=np.float64):
    """(p, q) [N,7], points [G,3] of the right_gripper frame -> world [N,G,3]: R g + p (float32: the device's fma chain)."""
    nodes = np.asarray(nodes).astype(dtype)
    R, p = rotation(nodes[:, 3:]), nodes[:, :3]
    g = np.asarray(points).astype(dtype)
    if dtype == np.float32:
        acc = R[:, None, :, 0] * g[None, :, None, 0]
        acc = fma32(R[:, None, :, 1], g[None, :, None, 1], acc)
        acc = fma32(R[:, None, :, 2], g[None, :, None, 2], acc)
        return acc + p[:, None]
    return np.einsum("nij,gj->ngi", R, g) + p[:, None]


def margins(nodes, scene_b, reach=1e-4, check_self=True, self_margin=1e-4, finger=ft.FINGER_OPENING, dtype=np.float64):
    """Poses (p, q) [N,7] against one problem (scene arrays with a leading axis of 1, or None) -> the smallest signed
    distance to a verdict's threshold per pose: min over the gripper's spheres of ``sdf - r_s - reach`` and, with
    ``check_self``, over the origins of frames 9 / 12 / 13 of ``distance to the base segment - (0.15 + 0.01 + margin)``.
    Positive: valid."""
    pts, radii, _, origins = gripper_points(finger, dtype)
    N = len(nodes)
    m = np.full(N, np.inf)
    if N == 0:
        return m
    if scene_b is not None and scene_b["cub_dims"].shape[1] + scene_b["cyl_radii"].shape[1] > 0:
        x = torch.from_numpy(np.ascontiguousarray(place(nodes, pts, dtype))).reshape(1, -1, 3)
        best = fp.sdf_min_grad(x, scene_b)[0].reshape(N, len(radii)).numpy().astype(np.float64)
        m = np.minimum(m, (best - radii.astype(np.float64) - reach).min(-1))
    if check_self:
        c = place(nodes, origins, dtype).astype(np.float64)
        dz = c[..., 2] - np.clip(c[..., 2], -0.3, 0.333)
        d = np.sqrt(c[..., 0] ** 2 + c[..., 1] ** 2 + dz ** 2)
        m = np.minimum(m, (d - (0.15 + 0.01 + self_margin)).min(-1))
    return m


# ---- nodes ---------------------------------------------------------------------------------------------------------------------
def default_bounds(start_pose, goal_pose):
    """float32 [B,2,3]: the box hull of the two positions grown by BOUNDS_PAD per side, as ``solvers.gripper_roadmap`` makes it."""
    ends = np.stack([np.asarray(start_pose, F32)[:, :3, 3], np.asarray(goal_pose, F32)[:, :3, 3]], 1)
    return np.stack([ends.min(1) - F32(BOUNDS_PAD), ends.max(1) + F32(BOUNDS_PAD)], 1).astype(F32)


def draw_nodes(start_pose, goal_pose, bounds, V=64, seed=0, env_offset=0, orient_spread=0.5):
    """-> nodes float32 [B,V,7] as the device rounds them (positions bit for bit; quaternions to the rounding of its division
    and square root) and ``drawn_ok`` bool [B,V] (|raw|^2 >= 2^-20; True for nodes 0 and 1)."""
    ns, ng = pose_nodes(start_pose, F32), pose_nodes(goal_pose, F32)
    B = ns.shape[0]
    bounds = np.broadcast_to(np.asarray(bounds, F32), (B, 2, 3))
    lo, hi = bounds[:, None, 0], bounds[:, None, 1]
    v = np.arange(V, dtype=np.uint64)[None, :]
    gid = ((env_offset + np.arange(B, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))[:, None]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r0 = philox4x32_np(2 * v, gid, STREAM_GRIPPER_ROADMAP, 0, k0, k1)
    r1 = philox4x32_np(2 * v + 1, gid, STREAM_GRIPPER_ROADMAP, 0, k0, k1)
    bits = np.stack(list(r0) + list(r1), axis=-1)  # [B,V,8]
    u = (bits >> np.uint32(8)).astype(F32) * F32(5.9604644775390625e-08)
    nodes = np.zeros((B, V, 7), F32)
    nodes[..., :3] = fma32(u[..., :3], hi - lo, lo)
    same = dot4(ns[:, 3:], ng[:, 3:], F32) >= 0
    toward = (np.where(same[:, None], ng[:, 3:], -ng[:, 3:]) - ns[:, 3:]).astype(F32)  # [B,4]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = fma32(u[..., 3:4], toward[:, None], ns[:, None, 3:])
        raw = fma32(F32(orient_spread), fma32(F32(2), u[..., 4:], F32(-1)), m)
        n2 = dot4(raw, raw, F32)
        nodes[..., 3:] = raw / np.sqrt(n2)[..., None]
        ok = n2 >= F32(2.0 ** -20)
    nodes[:, 0], ok[:, 0] = ns, True
    if V > 1:
        nodes[:, 1], ok[:, 1] = ng, True
    return nodes, ok


def endpoints_ok(start_pose, goal_pose, bounds):
    """bool [B]: rows 0-2 of both poses finite and both positions inside ``bounds`` (NaN fails)."""
    sp, gp = np.asarray(start_pose, F32), np.asarray(goal_pose, F32)
    bounds = np.broadcast_to(np.asarray(bounds, F32), (len(sp), 2, 3))
    ok = np.isfinite(sp[:, :3]).all((1, 2)) & np.isfinite(gp[:, :3]).all((1, 2))
    with np.errstate(invalid="ignore"):
        for M in (sp, gp):
            ok &= ((M[:, :3, 3] >= bounds[:, 0]) & (M[:, :3, 3] <= bounds[:, 1])).all(-1)
    return ok


# ---- metric, pieces, edge poses ------------------------------------------------------------------------------------------------
def _sq_chain(d, dtype):
    """Sum of squares over the last axis, k ascending: the first square rounded on its own, the others fused."""
    if dtype == np.float32:
        acc = d[..., 0] * d[..., 0]
        for k in range(1, d.shape[-1]):
            acc = fma32(d[..., k], d[..., k], acc)
        return acc
    return (d * d).sum(-1)


def lengths(nodes, rot_weight=DEFAULTS["rot_weight"], dtype=np.float64):
    """[V,7] -> w [V,V] in ``dtype``: sqrt(|p_b - p_a|^2 + (2 rot_weight)^2 |q_b - sigma q_a|^2); float32: the device's chain."""
    n = np.asarray(nodes).astype(dtype)
    dp = n[None, :, :3] - n[:, None, :3]
    same = dot4(n[:, None, 3:], n[None, :, 3:], dtype) >= 0
    dq = np.where(same[..., None], n[None, :, 3:] - n[:, None, 3:], n[None, :, 3:] + n[:, None, 3:]).astype(dtype)
    two_rw = dtype(2) * dtype(F32(rot_weight))
    rot_k = dtype(two_rw * two_rw)
    acc, rq = _sq_chain(dp, dtype), _sq_chain(dq, dtype)
    return np.sqrt(fma32(rot_k, rq, acc) if dtype == np.float32 else rot_k * rq + acc).astype(dtype)


def pieces(w, resolution, dtype=np.float64):
    n = np.ceil(dtype(w) / dtype(resolution))
    return int(min(MAX_PIECES, max(1.0, n)))


def edge_pose(na, nb, f, dtype=np.float64):
    """The poses at fractions ``f`` [n] of the edge from node ``na`` toward ``nb``: [n,7] (positions by fma, nlerp)."""
    a, b = np.asarray(na).astype(dtype), np.asarray(nb).astype(dtype)
    f = np.asarray(f).astype(dtype)[:, None]
    sb = b[3:] if dot4(a[3:], b[3:], dtype) >= 0 else -b[3:]
    if dtype == np.float32:
        p, raw = fma32(f, (b[:3] - a[:3])[None], a[None, :3]), fma32(f, (sb - a[3:])[None], a[None, 3:])
    else:
        p, raw = a[None, :3] + f * (b[:3] - a[:3])[None], a[None, 3:] + f * (sb - a[3:])[None]
    return np.concatenate([p, raw / np.sqrt(dot4(raw, raw, dtype))[:, None]], -1).astype(dtype)


def edge_poses(na, nb, n, dtype=np.float64):
    """The interior poses i = 1 .. n-1 of edge (a, b), a < b: [n-1,7]; float32: f = (float)i / (float)n as the device has it."""
    return edge_pose(na, nb, np.arange(1, n, dtype=dtype) / dtype(n), dtype)


# ---- search --------------------------------------------------------------------------------------------------------------------
def search(nodes, node_ok, is_valid, resolution=0.01, rot_weight=0.12, connect_radius=float("inf"), max_rounds=256,
           dtype=np.float64):
    """The lazy search on one problem.  ``nodes`` [V,7] float32; ``node_ok`` bool [V] (endpoint rules / the draw's norm);
    ``is_valid(poses [N,7] in dtype) -> bool [N]``.  -> status, path, edge_state uint8 [V,V], rounds."""
    nodes = np.asarray(nodes, F32)
    V = nodes.shape[0]
    valid = np.asarray(node_ok, bool) & np.asarray(is_valid(np.nan_to_num(nodes).astype(dtype)), bool)
    state = np.zeros((V, V), np.uint8)
    state[np.arange(V), np.arange(V)] = np.where(valid, FREE, BLOCKED)
    if not (valid[0] and valid[1]):
        return 2, [], state, 0
    Wm = lengths(np.nan_to_num(nodes), rot_weight, dtype)
    exists = Wm <= connect_radius
    for rnd in range(1, max_rounds + 1):
        dist, pred = fr.sweeps(Wm, exists & (state != BLOCKED), valid)
        if not np.isfinite(dist[1]):
            return 1, [], state, rnd
        path = [1]
        while path[-1] != 0:
            path.append(int(pred[path[-1]]))
        path.reverse()
        todo, poses = [], []
        for u, v in zip(path[:-1], path[1:]):
            a, b = min(u, v), max(u, v)
            if state[a, b] == UNTESTED:
                c = edge_poses(nodes[a], nodes[b], pieces(Wm[a, b], resolution, dtype), dtype)
                todo.append((a, b, len(c)))
                poses.append(c)
        any_blocked = False
        if todo:
            flat = np.concatenate(poses, 0)
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


def resample(nodes, path, W, rot_weight=DEFAULTS["rot_weight"], dtype=np.float64):
    """-> guide poses [W,4,4] in ``dtype``: pose t at s_t = (t+1)/W of the path's cumulative metric, on the last edge i with
    c_i <= s_t, by that edge's nlerp in path order.  (Pose W-1 is the last node's own pose here; the device copies the
    goal's matrix.)"""
    p = np.asarray(nodes, F32)[np.asarray(path)]
    Wm = lengths(p, rot_weight, dtype)
    w = np.array([Wm[i, i + 1] for i in range(len(p) - 1)], dtype)
    c = np.zeros(len(p), dtype)
    for i in range(len(w)):
        c[i + 1] = c[i] + w[i]
    s = (np.arange(1, W + 1, dtype=dtype) / dtype(W)) * c[-1]
    seg = np.clip(np.searchsorted(c[:-1], s, side="right") - 1, 0, len(w) - 1)
    out = np.zeros((W, 7), dtype)
    for t in range(W):
        i = seg[t]
        f = min((s[t] - c[i]) / w[i], dtype(1)) if w[i] > 0 else dtype(0)
        out[t] = edge_pose(p[i], p[i + 1], [f], dtype)[0]
    return pose_matrix(out)


def dijkstra_cost(nodes, edge_state, rot_weight=DEFAULTS["rot_weight"], connect_radius=float("inf")):
    """The float64 cost of the shortest path from node 0 to node 1 over "valid nodes, edges not in state 2" of the given
    ``edge_state`` [V,V] (+inf: unreachable).  A heap, not the sweeps: an independent route to the same number."""
    V = len(nodes)
    Wm = lengths(np.nan_to_num(np.asarray(nodes, F32)), rot_weight, np.float64)
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
        ok = valid & ~done & (edge_state[u] != BLOCKED) & (Wm[u] <= connect_radius)
        for v in np.flatnonzero(ok):
            nd = d + Wm[u, v]
            if nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, int(v)))
    return float("inf")


def path_cost(nodes, path, rot_weight=DEFAULTS["rot_weight"]):
    Wm = lengths(np.asarray(nodes, F32)[np.asarray(path)], rot_weight, np.float64)
    return float(sum(Wm[i, i + 1] for i in range(len(path) - 1)))


def validity(scene_b, reach, check_self, self_margin, finger=ft.FINGER_OPENING, dtype=np.float64):
    """-> ``is_valid`` of one problem for ``search``."""
    def is_valid(poses):
        return margins(poses, scene_b, reach, check_self, self_margin, finger, dtype) > 0
    return is_valid


def solve(start_pose, goal_pose, scene=None, W=8, bounds=None, seed=0, env_offset=0, dtype=np.float64, **options):
    """-> poses [B,W,4,4] (NaN rows where status != 0), status, path [B,V] (-1 padded), hops, nodes float32 [B,V,7],
    edge_state uint8 [B,V,V], rounds: like ``solvers.gripper_roadmap`` with ``return_graph``."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    V = opt["nodes"]
    sp, gp = np.asarray(start_pose, F32), np.asarray(goal_pose, F32)
    B = sp.shape[0]
    bounds = default_bounds(sp, gp) if bounds is None else np.broadcast_to(np.asarray(bounds, F32), (B, 2, 3))
    nodes, ok = draw_nodes(sp, gp, bounds, V, seed, env_offset, opt["orient_spread"])
    ok[:, :2] &= endpoints_ok(sp, gp, bounds)[:, None]
    poses = np.full((B, W, 4, 4), np.nan, dtype)
    status, hops, rounds = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    path = np.full((B, V), -1, np.int32)
    edge_state = np.zeros((B, V, V), np.uint8)
    for b in range(B):
        sc = None if scene is None else {k: v[b:b + 1] for k, v in scene.items()}
        is_valid = validity(sc, opt["clearance"] + opt["check_margin"], opt["check_self"], opt["check_margin"], dtype=dtype)
        st, p, es, r = search(nodes[b], ok[b], is_valid, opt["resolution"], opt["rot_weight"], opt["connect_radius"],
                              opt["max_rounds"], dtype)
        status[b], edge_state[b], rounds[b] = st, es, r
        if st == 0:
            hops[b] = len(p) - 1
            path[b, :len(p)] = p
            poses[b] = resample(nodes[b], p, W, opt["rot_weight"], dtype)
            poses[b, -1, :3] = gp[b, :3]
    return poses, status, path, hops, nodes, edge_state, rounds


# ---- the scenarios of the GPU tests --------------------------------------------------------------------------------------------
PROBLEM_SEED = 0   # numpy's default_rng for the start / goal draws
ROADMAP_SEED = 5   # the Philox seed the GPU tests plan with: chosen on the CPU (tests/test_gripper_roadmap_host.py)
WALL_CENTRE, WALL_DIMS = (0.45, 0.0, 0.45), (0.4, 0.02, 0.5)  # half-extents (0.2, 0.01, 0.25)
CYLINDER_RADIUS, CYLINDER_HEIGHT = 0.1, 0.5


def _rodrigues(rv):
    th = np.linalg.norm(rv, axis=-1)[:, None, None]
    k = rv / np.maximum(th[:, 0], 1e-30)
    K = np.zeros((len(rv), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3)[None] + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def problems(B=64, seed=PROBLEM_SEED, tilt=0.3):
    """-> start_pose, goal_pose float32 [B,4,4]: starts x in [0.35, 0.55], y in [-0.35, -0.25], z in [0.3, 0.6], goals
    drawn likewise and mirrored in y; the gripper points down (a half turn about x), perturbed by a rotation vector uniform in
    [-tilt, tilt]^3."""
    rng = np.random.default_rng(seed)
    down = np.diag([1.0, -1.0, -1.0])
    out = []
    for sign in (1.0, -1.0):
        M = np.tile(np.eye(4), (B, 1, 1))
        M[:, 0, 3], M[:, 1, 3], M[:, 2, 3] = rng.uniform(0.35, 0.55, B), sign * rng.uniform(-0.35, -0.25, B), rng.uniform(0.3, 0.6, B)
        M[:, :3, :3] = _rodrigues(rng.uniform(-tilt, tilt, (B, 3))) @ down
        out.append(M.astype(F32))
    return out[0], out[1]


def scene_arrays(B, kind):
    """``kind`` "wall" | "cylinder" | "free" -> the ``scenes.make_scenes``-layout arrays (identity quaternions, w first) that
    ``geometry.TorchCuboids`` / ``TorchCylinders`` take, M1 = 1 / M2 = 0 for the wall and M1 = 0 / M2 = 1 for the cylinder; None
    for free space."""
    if kind == "free":
        return None
    one = np.tile(F32([1, 0, 0, 0]), (B, 1, 1))
    centre = np.tile(F32(WALL_CENTRE), (B, 1, 1))
    if kind == "wall":
        return {"cuboid_centers": centre, "cuboid_dims": np.tile(F32(WALL_DIMS), (B, 1, 1)), "cuboid_quats": one}
    assert kind == "cylinder"
    return {"cylinder_centers": centre, "cylinder_radii": np.full((B, 1, 1), CYLINDER_RADIUS, F32),
            "cylinder_heights": np.full((B, 1, 1), CYLINDER_HEIGHT, F32), "cylinder_quats": one}


def scene_of(arrays, B):
    """``scene_arrays`` -> the float32 inverse frames and sizes ``float64_plan.sdf_min_grad`` reads (None for free space)."""
    from oracle import oracle as orc

    if arrays is None:
        return None
    s = {"cub_frames": np.zeros((B, 0, 4, 4), F32), "cub_dims": np.zeros((B, 0, 3), F32),
         "cyl_frames": np.zeros((B, 0, 4, 4), F32), "cyl_radii": np.zeros((B, 0), F32), "cyl_heights": np.zeros((B, 0), F32)}
    if "cuboid_dims" in arrays:
        s["cub_frames"] = orc.inv_frames_4x4(arrays["cuboid_centers"], orc.repair_quaternions(arrays["cuboid_quats"]))
        s["cub_dims"] = arrays["cuboid_dims"]
    if "cylinder_radii" in arrays:
        s["cyl_frames"] = orc.inv_frames_4x4(arrays["cylinder_centers"], orc.repair_quaternions(arrays["cylinder_quats"]))
        s["cyl_radii"], s["cyl_heights"] = arrays["cylinder_radii"][..., 0], arrays["cylinder_heights"][..., 0]
    return s


def graph_verdicts(nodes, node_ok, edge_state, scene_b, band, resolution=DEFAULTS["resolution"], rot_weight=DEFAULTS["rot_weight"],
                   reach=1e-4, check_self=True, self_margin=1e-4):
    """The float64 verdict on the diagonal and on every TESTED edge of a given ``edge_state`` [V,V] over float32 ``nodes``
    (a device's, or the restatement's own), the edge poses as float32 states them -> (expected uint8 [V,V] on those entries, 0
    elsewhere; in_band: a pose that decides one of them lies within ``band`` of its threshold; the tested poses [N,7] float32)."""
    nodes = np.nan_to_num(np.asarray(nodes, F32))
    V = nodes.shape[0]
    W32 = lengths(nodes, rot_weight, F32)
    want = np.zeros((V, V), np.uint8)
    edges = list(zip(*np.nonzero(np.triu(edge_state != UNTESTED, 1))))
    poses = [edge_poses(nodes[a], nodes[b], pieces(W32[a, b], F32(resolution), F32), F32) for a, b in edges]
    tested = np.concatenate([nodes] + poses, 0)
    m = margins(tested.astype(np.float64), scene_b, reach, check_self, self_margin)
    mv, at = m[:V], V
    ok = np.asarray(node_ok, bool)
    want[np.arange(V), np.arange(V)] = np.where(ok & (mv > 0), FREE, BLOCKED)
    in_band = bool((np.abs(mv[ok]) <= band).any())
    for (a, b), q in zip(edges, poses):
        me, at = m[at:at + len(q)], at + len(q)
        want[a, b] = want[b, a] = FREE if (me > 0).all() else BLOCKED
        if not (me < -band).any() and (np.abs(me) <= band).any():  # (a definite hit decides the edge whatever else is close)
            in_band = True
    return want, in_band, tested
