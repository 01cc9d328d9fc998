"""Restatement of ``mpx_gripper_shortcut`` / ``mpx_gripper_shortcut_cloud`` on the CPU, written from the contract in
include/mpinets_hip.h (not from csrc/shortcut_kernel.inc or csrc/gripper_shortcut.hip): the row rule, alternating passes, each
densifying the SE(3) polyline to at most P points and walking it greedily from the anchor to the furthest point whose chord is
free, found by a K-ary search, then the guide poses over the returned polyline.

Built on tests/float64_gripper_roadmap.py (``lengths``, ``pieces``, ``edge_pose``, ``edge_poses``, ``margins``, ``resample``,
``pose_matrix``), tests/float64_gripper_roadmap_cloud.py (``margins`` of the field) and tests/float64_shortcut.py
(``probes``).  The validity test is a callable, ``is_valid(poses [N,7] float64) -> bool [N]``, always asked in float64.
``dtype`` is the precision of the GEOMETRY (lengths, pieces, the densification, the chords' interior poses, the resampling):
float64 by default; ``np.float32`` states the device's own float32 operations (``fma32`` where the contract says fma), so that
run takes the device's decisions wherever a verdict is not within rounding of its threshold.

``in_band`` is reported when a pose that decides a chord has ``margins(pose)`` within ``band`` of zero, and also when a
chord's w / resolution lies within 2^-20 (relative) of an integer: one ulp of a device square root could then change the
piece count, and with it every interior pose of the chord.
"""
import numpy as np

import float64_gripper_roadmap as fg
import float64_gripper_roadmap_cloud as fgc
from float64_shortcut import probes

MAX_POINTS = 256   # MPX_ROADMAP_MAX_NODES
MAX_FANOUT = 256   # MPX_SHORTCUT_MAX_FANOUT
MAX_POSES = 64     # MPX_FOLLOW_MAX_POSES
# MPX_SHORTCUT_DEFAULT_* of include/mpinets_hip.h and the gripper roadmap's values
DEFAULTS = dict(points=64, passes=2, fanout=4, resolution=0.01, rot_weight=0.12, check_margin=1e-4, clearance=0.0,
                check_self=True)
UNIT_TOL = 2.0 ** -10      # a vertex quaternion's |q|^2 must be within this of 1
PIECES_BAND = 2.0 ** -20   # relative distance of w / resolution to an integer below which the piece count is fragile
F32 = np.float32


def bad_row(polyline, count):
    """The status-2 rule on one row: ``polyline`` float32 [Pin,7], ``count`` its vertices."""
    p = np.asarray(polyline, F32)
    if count < 2 or count > len(p):
        return True
    v = p[:count]
    if not np.isfinite(v).all():
        return True
    n2 = fg.dot4(v[:, 3:], v[:, 3:], F32)
    return bool((~(np.abs(n2 - F32(1)) <= F32(UNIT_TOL))).any())


def length(na, nb, rot_weight=DEFAULTS["rot_weight"], dtype=np.float64):
    """w of the segment (a, b): ``float64_gripper_roadmap.lengths`` on the pair."""
    return dtype(fg.lengths(np.stack([np.asarray(na).astype(dtype), np.asarray(nb).astype(dtype)]), rot_weight, dtype)[0, 1])


def polyline_length(p, rot_weight=DEFAULTS["rot_weight"], dtype=np.float64):
    total = dtype(0)
    for i in range(len(p) - 1):
        total = dtype(total + length(p[i], p[i + 1], rot_weight, dtype))
    return total


def densify(p, P, rot_weight=DEFAULTS["rot_weight"], dtype=np.float64):
    """[n,7] -> the dense polyline [N,7] in ``dtype``, N <= P, and the index of every vertex in it.  An interior point is the
    edge pose of (v_i, v_{i+1}) at (float)k / (float)(m+1); the vertices are copied."""
    p = np.asarray(p).astype(dtype)
    n = len(p)
    w = [length(p[i], p[i + 1], rot_weight, dtype) for i in range(n - 1)]
    L = dtype(0)
    for x in w:
        L = dtype(L + x)
    extra = P - n
    left = extra if (L > 0 and np.isfinite(L) and extra > 0) else 0
    out, at = [], []
    for i in range(n - 1):
        m = 0
        if left > 0:
            x = np.floor(dtype(dtype(w[i] * dtype(extra)) / L))
            m = left if x >= left else int(x) if x >= 1 else 0
        left -= m
        at.append(len(out))
        out.append(p[i])
        if m:
            f = (np.arange(1, m + 1).astype(dtype) / dtype(m + 1)).astype(dtype)
            out.extend(fg.edge_pose(p[i], p[i + 1], f, dtype))
    at.append(len(out))
    out.append(p[-1])
    return np.stack(out).astype(dtype), at


def chord_pieces(w, resolution, dtype=np.float64):
    """-> (n, fragile): the pieces of a chord of length ``w`` and whether w / resolution is within PIECES_BAND of an integer."""
    x = float(w) / float(F32(resolution))
    fragile = x > 0 and abs(x - round(x)) <= PIECES_BAND * x
    return fg.pieces(w, dtype(F32(resolution)), dtype), bool(fragile)


def greedy(D, is_valid, K, resolution, rot_weight, dtype=np.float64, trace=None, margins=None, band=0.0):
    """One greedy walk over the dense polyline ``D`` -> the indices kept (``float64_shortcut.greedy``'s walk with the gripper's
    length, pieces and edge poses)."""
    N = len(D)
    kept, a = [0], 0
    while a != N - 1:
        lo, hi = a + 1, N - 1
        while hi > lo:
            pr = probes(lo, hi, K)
            blocked = []
            for e in pr:
                n, fragile = chord_pieces(length(D[a], D[e], rot_weight, dtype), resolution, dtype)
                q = fg.edge_poses(D[a], D[e], n, dtype).astype(np.float64)
                ok = np.asarray(is_valid(q), bool) if len(q) else np.zeros(0, bool)
                blocked.append(not ok.all())
                if trace is not None:
                    trace["chords"] += 1
                    trace["configs"] += len(q)
                    trace["in_band"] |= fragile
                    if margins is not None and len(q):
                        m = margins(q)
                        if not (m < -band).any() and (np.abs(m) <= band).any():
                            trace["in_band"] = True
                    if ok.all():
                        trace["free"].append((D[a].copy(), D[e].copy()))
            if not blocked[-1]:
                lo = hi
                break
            free = [i for i in range(len(pr) - 1) if not blocked[i]]
            best = free[-1] if free else -1
            if best >= 0:
                lo = pr[best]
            hi = pr[best + 1] - 1
        kept.append(lo)
        a = lo
    return kept


def guide_poses(polyline, W, goal_pose=None, rot_weight=DEFAULTS["rot_weight"], dtype=np.float64):
    """The clause "poses" over a polyline [n,7]: ``float64_gripper_roadmap.resample`` with path[i] = i; pose W-1 is
    ``goal_pose`` (rows 0-2 of a [4,4]) or, without one, the last vertex's own frame."""
    p = np.asarray(polyline)
    out = fg.resample(p, np.arange(len(p)), W, rot_weight, dtype)
    out[-1] = fg.pose_matrix(p[-1:].astype(dtype))[0]
    if goal_pose is not None:
        out[-1, :3] = np.asarray(goal_pose, F32)[:3]
    return out


def shortcut(polyline, is_valid, W=8, goal_pose=None, dtype=np.float64, margins=None, band=0.0, **options):
    """One problem.  ``polyline`` [n,7] float32, a good row.  -> dict of ``points_out`` [n',7] in ``dtype``, ``poses`` [W,4,4]
    in ``dtype``, ``length`` (before, after) in ``dtype``, ``chords``, ``configs``, ``in_band``, ``free`` (the chords found
    free, as pairs of end points in the order tested, in the pass's order) and ``dense`` (the dense polyline of every pass, in
    the pass's order)."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    P, K, rw = opt["points"], opt["fanout"], opt["rot_weight"]
    cur = np.asarray(polyline, F32).astype(dtype)
    assert 2 <= len(cur) <= P <= MAX_POINTS and 1 <= K <= MAX_FANOUT and 1 <= W <= MAX_POSES
    assert not bad_row(polyline, len(cur))
    trace = dict(chords=0, configs=0, in_band=False, free=[], dense=[])
    before = polyline_length(cur, rw, dtype)
    for p in range(opt["passes"]):
        if len(cur) <= 2:
            break
        if p & 1:
            cur = cur[::-1]
        D, _ = densify(cur, P, rw, dtype)
        trace["dense"].append(D)
        cur = D[greedy(D, is_valid, K, opt["resolution"], rw, dtype, trace, margins, band)]
        if p & 1:
            cur = cur[::-1]
    cur = np.ascontiguousarray(cur)
    poses = guide_poses(cur, W, goal_pose, rw, dtype)
    return dict(points_out=cur, poses=poses, length=(before, polyline_length(cur, rw, dtype)), **trace)


# ---- the two validity rules, each as (is_valid, margins) of one problem ----------------------------------------------------------
def prim_rule(scene_b, clearance=0.0, check_margin=1e-4, check_self=True):
    """``mpx_gripper_roadmap``'s clause against one problem's primitives (``float64_gripper_roadmap.scene_of`` arrays with a
    leading axis of 1, or None)."""
    def m(q):
        return fg.margins(np.asarray(q, np.float64), scene_b, clearance + check_margin, check_self, check_margin)
    return (lambda q: m(q) > 0), m


def field_rule(field_b, grid, point_radius=0.0, field_slack=0.0, clearance=0.0, check_margin=1e-4, check_self=True):
    """``mpx_gripper_roadmap_cloud``'s clause against one environment's field (None: no environment)."""
    def m(q):
        env, own = fgc.margins(np.asarray(q, np.float64), field_b, grid, point_radius, clearance, check_margin, field_slack,
                               check_self)
        return np.minimum(env, own)
    return (lambda q: m(q) > 0), m


def path_polylines(nodes, path, hops):
    """A gripper roadmap's graph -> what ``gripper_plan`` hands the shortcut: ``nodes[path]`` [B,V,7] float32 (rows behind a
    path: node 0) and the vertex counts (0 where there is no path: a bad row)."""
    nodes, path, hops = np.asarray(nodes, F32), np.asarray(path), np.asarray(hops)
    pts = np.take_along_axis(nodes, np.maximum(path, 0)[:, :, None].astype(np.int64), 1)
    return pts, np.where(hops > 0, hops + 1, 0).astype(np.int32)


def same_rotation(qa, qb):
    """|q_a - sigma q_b| per row, sigma the sign that makes it smaller: the difference of two quaternions up to sign."""
    qa, qb = np.asarray(qa, np.float64), np.asarray(qb, np.float64)
    return np.minimum(np.abs(qa - qb).max(-1), np.abs(qa + qb).max(-1))
