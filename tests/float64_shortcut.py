"""Restatement of ``mpx_franka_shortcut`` / ``mpx_franka_shortcut_cloud`` on the CPU, written from the contract in
include/mpinets_hip.h (not from csrc/shortcut_kernel.inc): alternating passes, each densifying the polyline to at most P
points and walking it greedily from the anchor to the furthest point whose chord is free, found by a K-ary search.

Built on tests/float64_roadmap.py (``pieces``, ``edge_configs``, ``resample``, ``smooth``, ``franka_validity``, ``fma32``)
and tests/float64_roadmap_cloud.py (``field_validity``): the validity test is a callable, ``is_valid(q [N,7] float64) ->
bool [N]``, always asked in float64.  ``dtype`` is the precision of the GEOMETRY (lengths, the densification, the chords'
interior configurations, resampling and the corner filter): float64 by default; ``np.float32`` states the device's own
float32 operations (``fma32`` where the contract says fma), so that run takes the device's decisions wherever the validity
test is not within rounding of its threshold -- ``edge_configs``'s float32 mode, for the whole algorithm.  The segment length
here is the contract's (the first square rounded on its own, the others fused), not ``float64_roadmap.lengths``' plain sum.
"""
import numpy as np

import float64_plan as fp
import float64_roadmap as fr

MAX_POINTS = 256   # MPX_ROADMAP_MAX_NODES
MAX_FANOUT = 256   # MPX_SHORTCUT_MAX_FANOUT
# MPX_SHORTCUT_DEFAULT_* of include/mpinets_hip.h and the roadmap's values
DEFAULTS = dict(points=64, passes=2, fanout=4, resolution=0.05, smooth_passes=8, check_margin=1e-4, clearance=0.0,
                check_self=True)


def length(qa, qb, dtype=np.float64):
    """|q_b - q_a|, j ascending; float32: d_0 d_0 rounded, then fma(d_j, d_j, acc)."""
    d = np.asarray(qb).astype(dtype) - np.asarray(qa).astype(dtype)
    acc = d[0] * d[0]
    for j in range(1, 7):
        acc = fr.fma32(d[j], d[j], acc) if dtype == np.float32 else acc + d[j] * d[j]
    return dtype(np.sqrt(dtype(acc)))


def polyline_length(p, dtype=np.float64):
    total = dtype(0)
    for i in range(len(p) - 1):
        total = dtype(total + length(p[i], p[i + 1], dtype))
    return total


def densify(p, P, dtype=np.float64):
    """[n,7] -> the dense polyline [N,7] in ``dtype``, N <= P, and the index of every vertex in it."""
    p = np.asarray(p).astype(dtype)
    n = len(p)
    w = [length(p[i], p[i + 1], dtype) for i in range(n - 1)]
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
        for k in range(1, m + 1):
            f = dtype(dtype(k) / dtype(m + 1))
            out.append(fr.fma32(f, p[i + 1] - p[i], p[i]) if dtype == np.float32 else p[i] + f * (p[i + 1] - p[i]))
    at.append(len(out))
    out.append(p[-1])
    return np.stack(out).astype(dtype), at


def probes(lo, hi, K):
    span = hi - lo
    out = []
    for k in range(1, K + 1):
        pr = lo + (span * k + K - 1) // K
        if not out or out[-1] != pr:
            out.append(pr)
    return out


def greedy(D, is_valid, K, resolution, dtype=np.float64, trace=None, margins=None, band=0.0):
    """One greedy walk over the dense polyline ``D`` -> the indices kept.  ``trace``: a dict whose ``chords`` / ``configs``
    are counted up, whose ``free`` gets (a, e) of every chord found free and whose ``in_band`` is set when a configuration
    that decides a chord has ``margins(q)`` within ``band`` of zero."""
    N = len(D)
    kept, a = [0], 0
    while a != N - 1:
        lo, hi = a + 1, N - 1
        while hi > lo:
            pr = probes(lo, hi, K)
            blocked = []
            for e in pr:
                n = fr.pieces(length(D[a], D[e], dtype), dtype(resolution), dtype)
                q = fr.edge_configs(D[a], D[e], n, dtype).astype(np.float64)
                ok = np.asarray(is_valid(q), bool) if len(q) else np.zeros(0, bool)
                blocked.append(not ok.all())
                if trace is not None:
                    trace["chords"] += 1
                    trace["configs"] += len(q)
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


def shortcut(polyline, is_valid, T=50, dtype=np.float64, margins=None, band=0.0, **options):
    """One problem.  ``polyline`` [n,7] float32, n >= 2 and finite.  -> dict of ``points_out`` [n',7] in ``dtype``, ``traj``
    [T,7] in ``dtype``, ``length`` (before, after) in ``dtype``, ``chords``, ``configs``, ``in_band``, ``free`` (the
    chords found free, as pairs of end points in the order tested)."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    P, K = opt["points"], opt["fanout"]
    cur = np.asarray(polyline, np.float32).astype(dtype)
    assert 2 <= len(cur) <= P <= MAX_POINTS and 1 <= K <= MAX_FANOUT and np.isfinite(cur).all()
    trace = dict(chords=0, configs=0, in_band=False, free=[])
    before = polyline_length(cur, dtype)
    for p in range(opt["passes"]):
        if len(cur) <= 2:
            break
        if p & 1:
            cur = cur[::-1]
        D, _ = densify(cur, P, dtype)
        cur = D[greedy(D, is_valid, K, opt["resolution"], dtype, trace, margins, band)]
        if p & 1:
            cur = cur[::-1]
    cur = np.ascontiguousarray(cur)
    if len(cur) == 2:
        traj = fp.line(cur[:1].astype(np.float32), cur[1:].astype(np.float32), T)[0].astype(dtype)
    else:
        traj = fr.smooth(fr.resample(cur, T, dtype), opt["smooth_passes"], dtype)
    return dict(points_out=cur, traj=traj, length=(before, polyline_length(cur, dtype)), **trace)


def path_polylines(nodes, path, hops):
    """A roadmap's graph -> what the global planners hand the shortcut: ``nodes[path]`` [B,V,7] float32 (rows behind a
    path: node 0) and the vertex counts (0 where there is no path: a bad row)."""
    nodes, path, hops = np.asarray(nodes, np.float32), np.asarray(path), np.asarray(hops)
    pts = np.take_along_axis(nodes, np.maximum(path, 0)[:, :, None].astype(np.int64), 1)
    return pts, np.where(hops > 0, hops + 1, 0).astype(np.int32)
