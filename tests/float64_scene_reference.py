"""Restatement of ``mpx_scene_generate_reference`` on the CPU in float64 NumPy, vectorised over the scenes and written from
the contract in include/mpinets_hip.h (not from csrc/scene_gen_reference.hip): the four Philox blocks of item 0 (the scene's
parameters), the tabletop's candidates (item c + 1, two blocks) and its greedy accept walk, the cubby's seven plates about
the cabinet's centre, its four pockets, and the merged cubby's dropped plates and merged supports.

Every DISCRETE decision that reads a uniform alone is the device's, exactly: a threshold compares the 24-bit uniform with
the float32 constant, an integer draw is integer arithmetic.  Two decisions of the tabletop read computed floats -- the
table a candidate lies on (``u (A0 + A1) >= A0``) and the accept test (``d > 0.05``); ``generate`` returns how close each
scene came to either (``margin``), and a comparison against the device leaves out the scenes that came closer than a stated
margin (tests/test_scene_reference_host.py derives it).  Every other quantity is computed in float64 from the float32
constants the contract names.
"""
import numpy as np

from float64_ik import philox4x32_np
from float64_scene_gen import PRIMITIVE_KEYS, SURFACE, VOLUME, _empty, draw_int, f, fma, live_rows, yaw_quat  # noqa: F401

STREAM_SCENE_GEN = 19
TABLETOP_REFERENCE, CUBBY_REFERENCE, MERGED_CUBBY = 3, 4, 5
MAX_OBJECTS, MAX_CANDIDATES = 14, 140
PIO2, PI18, PI9 = f(np.pi / 2), f(np.pi / 18), f(np.pi / 9)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))  # the six unordered pocket pairs, in the order of the integer draw


def blocks(item, ids, seed, nblocks):
    """-> (words uint64 [...,4 nblocks], u float64 [...,4 nblocks]) of ``item`` (broadcast against ``ids``)."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    item, ids = np.broadcast_arrays(np.asarray(item, np.uint64), np.asarray(ids, np.uint64) & np.uint64(0xFFFFFFFF))
    w = ()
    for blk in range(nblocks):
        w = w + tuple(philox4x32_np(item, ids, STREAM_SCENE_GEN, blk, k0, k1))
    w = np.stack(w, -1).astype(np.uint64)
    return w, (w >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


def footprint_distance(x, y, obj):
    """The contract's 2-D distance of the points (x, y) [n] to the footprints ``obj`` [n,14] -> [n,14] (1000 where empty)."""
    dx, dy = x[:, None] - obj["x"], y[:, None] - obj["y"]
    cyl = np.sqrt(dx * dx + dy * dy) - obj["r"]
    lx, ly = obj["c"] * dx + obj["s"] * dy, obj["c"] * dy - obj["s"] * dx
    qx, qy = np.abs(lx) - 0.5 * obj["dx"], np.abs(ly) - 0.5 * obj["dy"]
    box = np.sqrt(np.maximum(qx, 0) ** 2 + np.maximum(qy, 0) ** 2) + np.minimum(np.maximum(qx, qy), 0)
    return np.where(obj["type"] == 1, cyl, np.where(obj["type"] == 2, box, 1000.0))


def tabletop(ids, M1, M2, S, seed):
    n = len(ids)
    out = _empty(n, M1, M2, S)
    w0, u = blocks(0, ids, seed, 4)
    h = np.where(u[:, 0] < f(0.35), 0.0, u[:, 1] * f(0.4))
    tz, td = (h - f(0.02)) * 0.5, h + f(0.02)
    fx0, fx1 = fma(u[:, 2], f(0.1), f(0.275)), fma(u[:, 3], f(0.1), f(1.275))
    fy1 = fma(u[:, 4], f(0.15), 1.5)
    side = u[:, 5] < 0.5
    fy0 = np.where(side, fma(u[:, 6], 0.25, -1.0), fma(u[:, 6], f(0.2), -0.75))
    Dx, Dy = fx1 - fx0, fy1 - fy0
    scalar = fma(u[:, 7], f(0.1), f(0.55))
    ty = scalar * Dy
    sy1 = fma(u[:, 8], f(0.05), f(-0.325))
    L = u[:, 9] * 1.375
    scalar_side = fma(u[:, 10], f(0.1), f(0.55))
    sdx = L * scalar_side
    SDy = sy1 - fy0
    mcx, mcy = fma(u[:, 11], f(0.04), f(-0.02)), fma(u[:, 12], f(0.04), f(-0.02))
    mdy = fma(u[:, 13], f(0.04), f(0.9))
    K = 3 + draw_int(w0[:, 15], 12)
    T = np.where(side, 5, 3)
    zero = np.zeros(n)
    tables = {  # role -> centre, dims
        0: ((fx0 + fx1) * 0.5, fma(ty, 0.5, fy0), tz, Dx, ty, td),
        1: (fx0 - sdx * 0.5, (sy1 + fy0) * 0.5, tz, sdx, SDy, td),
        2: ((fx0 + fx1) * 0.5, (fy1 + (fy0 + ty)) * 0.5, tz, Dx, Dy - ty, td),
        3: (((fx0 - L) + (fx0 - sdx)) * 0.5, (sy1 + fy0) * 0.5, tz, L - sdx, SDy, td),
        4: (mcx, mcy, zero + f(-0.01), 2.0 * (fx0 - mcx), np.where(side, 2.0 * (mcy - sy1), mdy), zero + f(0.02)),
    }
    ident = np.tile([1.0, 0, 0, 0], (n, 1))
    for role, vals in tables.items():
        box = np.stack(vals, -1)
        rows = np.flatnonzero(side) if role in (1, 3) else np.arange(n)
        at = np.where(side, role, {0: 0, 2: 1, 4: 2}.get(role, 0))[rows]
        out["cuboid_centers"][rows, at], out["cuboid_dims"][rows, at] = box[rows, :3], box[rows, 3:]
        if role < 2 and role < S:
            out["support_boxes"][rows, role] = np.concatenate([box[rows], ident[rows], zero[rows, None],
                                                               (box[rows, 3] * box[rows, 4])[:, None]], -1)
            out["support_kind"][rows, role] = SURFACE
    # the candidates
    c = np.arange(MAX_CANDIDATES)
    _, v = blocks(c[None] + 1, np.asarray(ids)[:, None], seed, 2)  # [n,140,8]
    A0, A1 = Dx * ty, np.where(side, sdx * SDy, 0.0)
    pick = v[..., 0] * (A0 + A1)[:, None] - A0[:, None]
    on_side = side[:, None] & (pick >= 0)
    x = np.where(on_side, fma(v[..., 1], sdx[:, None], (fx0 - sdx)[:, None]), fma(v[..., 1], Dx[:, None], fx0[:, None]))
    y = np.where(on_side, fma(v[..., 2], SDy[:, None], fy0[:, None]), fma(v[..., 2], ty[:, None], fy0[:, None]))
    margin = np.full(n, np.inf)  # how close the scene's float decisions came to their thresholds
    obj = {k: np.zeros((n, MAX_OBJECTS)) for k in ("x", "y", "r", "dx", "dy", "c", "s")}
    obj["type"] = np.zeros((n, MAX_OBJECTS), np.int64)
    clearance = np.full((n, MAX_OBJECTS), np.nan)
    accepted = np.full((n, MAX_OBJECTS), -1)
    placed, n_cyl, n_box = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    every = np.arange(n)
    for ci in range(MAX_CANDIDATES):
        walking = (ci < 10 * K) & (placed < K)
        if not walking.any():
            break
        d = footprint_distance(x[:, ci], y[:, ci], obj)
        m = d.min(1)
        seen = walking & side
        margin[seen] = np.minimum(margin[seen], np.abs(pick[seen, ci]) / (A0 + A1)[seen])
        margin[walking] = np.minimum(margin[walking], np.abs(d[walking] - f(0.05)).min(1))
        ok = walking & (m > f(0.05))
        is_cyl = v[:, ci, 3] < f(0.3)
        ok &= np.where(is_cyl, n_cyl < M2, T + n_box < M1)  # the overflow rule
        span = np.minimum(m, f(0.15)) - f(0.05)
        r = np.flatnonzero(ok & is_cyl)
        hh = fma(v[r, ci, 5], f(0.3), f(0.05))
        rad = fma(v[r, ci, 4], span[r], f(0.05))
        out["cylinder_centers"][r, n_cyl[r]] = np.stack([x[r, ci], y[r, ci], fma(hh, 0.5, h[r])], -1)
        out["cylinder_radii"][r, n_cyl[r], 0], out["cylinder_heights"][r, n_cyl[r], 0] = rad, hh
        obj["type"][r, placed[r]], obj["r"][r, placed[r]] = 1, rad
        n_cyl[r] += 1
        r = np.flatnonzero(ok & ~is_cyl)
        dz = fma(v[r, ci, 6], f(0.3), f(0.05))
        dims = np.stack([fma(v[r, ci, 4], span[r], f(0.05)), fma(v[r, ci, 5], span[r], f(0.05)), dz], -1)
        yaw = v[r, ci, 7] * PIO2
        row = T[r] + n_box[r]
        out["cuboid_centers"][r, row] = np.stack([x[r, ci], y[r, ci], fma(dz, 0.5, h[r])], -1)
        out["cuboid_dims"][r, row], out["cuboid_quats"][r, row] = dims, yaw_quat(yaw)
        obj["type"][r, placed[r]], obj["dx"][r, placed[r]], obj["dy"][r, placed[r]] = 2, dims[:, 0], dims[:, 1]
        obj["c"][r, placed[r]], obj["s"][r, placed[r]] = np.cos(yaw), np.sin(yaw)
        n_box[r] += 1
        r = np.flatnonzero(ok)
        obj["x"][r, placed[r]], obj["y"][r, placed[r]] = x[r, ci], y[r, ci]
        clearance[r, placed[r]], accepted[r, placed[r]] = np.minimum(m[r], f(0.15)), ci
        placed[r] += 1
    aux = dict(margin=margin, clearance=clearance, accepted=accepted, K=K, side=side, objects=obj, placed=placed,
               params=dict(h=h, fx0=fx0, fx1=fx1, fy0=fy0, fy1=fy1, scalar=scalar, sy1=sy1, L=L, scalar_side=scalar_side, mcx=mcx,
                           mcy=mcy, mdy=mdy))
    return out, aux


def cubby_parameters(ids, seed):
    w0, u = blocks(0, ids, seed, 4)
    front = fma(u[:, 3], f(0.2), f(0.45))
    return dict(left=fma(u[:, 0], f(0.2), f(0.6)), right=fma(u[:, 1], f(0.2), f(-0.8)), bottom=fma(u[:, 2], f(0.2), f(0.1)),
                front=front, back=front + fma(u[:, 4], f(0.4), f(0.15)), top=fma(u[:, 5], f(0.2), f(0.6)),
                mz=fma(u[:, 6], f(0.2), f(0.35)), my=fma(u[:, 7], f(0.2), f(-0.1)), t=fma(u[:, 8], f(0.02), f(0.01)),
                yaw=fma(u[:, 9], PI9, -PI18)), draw_int(w0[:, 12], 6)


def cubby(ids, M1, M2, S, seed, pairs):
    """``pairs`` int [n,2]: the merge of every scene ((-1, -1) and anything that is no pair of distinct pockets: unmerged);
    None: the drawn pair (the merged cubby without operand)."""
    n = len(ids)
    out = _empty(n, M1, M2, S)
    p, drawn = cubby_parameters(ids, seed)
    if pairs is None:
        pairs = np.asarray(PAIRS)[drawn]
    pa, pb = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
    merged = (pa >= 0) & (pa <= 3) & (pb >= 0) & (pb <= 3) & (pa != pb)
    no_shelf, no_wall = merged & ((pa >> 1) != (pb >> 1)), merged & ((pa & 1) != (pb & 1))
    c, s = np.cos(p["yaw"]), np.sin(p["yaw"])
    px, py, pz = (p["front"] + p["back"]) * 0.5, (p["left"] + p["right"]) * 0.5, (p["top"] + p["bottom"]) * 0.5
    Dd, Wd, Hd, t = p["back"] - p["front"], p["left"] - p["right"], (p["top"] - p["bottom"]) + p["t"], p["t"]

    def world(lx, ly, lz):
        ax, ay = lx - px, ly - py
        return np.stack([(c * ax - s * ay) + px, (s * ax + c * ay) + py, lz + 0 * px], -1)

    plates = [((p["back"], py, p["top"] * 0.5), (t, Wd, p["top"])), ((px, py, p["bottom"]), (Dd, Wd, t)),
              ((px, py, p["top"]), (Dd, Wd, t)), ((px, p["right"], pz), (Dd, t, Hd)), ((px, p["left"], pz), (Dd, t, Hd)),
              ((px, p["my"], pz), (Dd, t, Hd)), ((px, py, p["mz"]), (Dd, Wd, t))]
    quat = yaw_quat(p["yaw"])
    for i, (lc, dims) in enumerate(plates):
        keep = ~no_wall if i == 5 else ~no_shelf if i == 6 else np.ones(n, bool)
        row = np.full(n, i) - (no_wall & (i > 5))
        r = np.flatnonzero(keep)
        out["cuboid_centers"][r, row[r]], out["cuboid_dims"][r, row[r]] = world(*lc)[r], np.stack(dims, -1)[r]
        out["cuboid_quats"][r, row[r]] = quat[r]
    ns = np.where(no_shelf & no_wall, 1, np.where(no_shelf | no_wall, 2, 4))
    for slot in range(min(4, S)):
        level = np.where(no_shelf, -1, np.where(no_wall, slot, slot >> 1))
        sd = np.where(no_wall, -1, np.where(no_shelf, slot, slot & 1))
        ya, yb = np.where(sd == 0, p["my"], p["right"]), np.where(sd == 1, p["my"], p["left"])
        za, zb = np.where(level == 0, p["mz"], p["bottom"]), np.where(level == 1, p["mz"], p["top"])
        r = np.flatnonzero(slot < ns)
        box = np.concatenate([world(px, (ya + yb) * 0.5, (za + zb) * 0.5), np.stack([Dd, yb - ya, zb - za], -1), quat,
                              np.zeros((n, 1)), np.ones((n, 1))], -1)
        out["support_boxes"][r, slot], out["support_kind"][r, slot] = box[r], VOLUME
    return out, dict(no_shelf=no_shelf, no_wall=no_wall, params=p)


def merged_support(pocket, a, b):
    """The contract's pocket -> support map under the merge (a, b) (arrays broadcast; unmerged: the pocket itself)."""
    pocket, a, b = np.broadcast_arrays(np.asarray(pocket), np.asarray(a), np.asarray(b))
    merged = (a >= 0) & (a <= 3) & (b >= 0) & (b <= 3) & (a != b)
    no_shelf, no_wall = merged & ((a >> 1) != (b >> 1)), merged & ((a & 1) != (b & 1))
    return np.where(no_shelf & no_wall, 0, np.where(no_wall, pocket >> 1, np.where(no_shelf, pocket & 1, pocket)))


def generate(kind, ids, M1, M2, S, seed=0, merge_pockets=None, aux=False):
    """``mpx_scene_generate_reference`` on rows of ``kind`` 3, 4, 5 (every other row comes back as NaN / -1: UNTOUCHED) ->
    make_task_scenes' arrays in float64; ``S`` = 0: no support keys.  ``aux``: also {kind code: the generator's side data}."""
    kind, ids = np.asarray(kind), np.asarray(ids, np.int64)
    assert 7 <= M1 <= 64 and 0 <= M2 <= 64 and 0 <= S <= 64
    out = {k: np.full_like(v, -1 if v.dtype == np.int32 else np.nan) for k, v in _empty(len(kind), M1, M2, S).items()}
    side = {}
    for code in (TABLETOP_REFERENCE, CUBBY_REFERENCE, MERGED_CUBBY):
        sel = np.flatnonzero(kind == code)
        if not len(sel):
            continue
        if code == TABLETOP_REFERENCE:
            part, side[code] = tabletop(ids[sel], M1, M2, S, int(seed))
            side[code]["rows"] = sel
        else:
            pairs = np.full((len(sel), 2), -1) if code == CUBBY_REFERENCE else \
                None if merge_pockets is None else np.asarray(merge_pockets)[sel]
            part, side[code] = cubby(ids[sel], M1, M2, S, int(seed), pairs)
            side[code]["rows"] = sel
        for key in out:
            out[key][sel] = part[key]
    if S == 0:
        del out["support_boxes"], out["support_kind"]
    return (out, side) if aux else out
