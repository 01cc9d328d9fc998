"""Restatement of ``mpx_scene_generate`` on the CPU in float64 NumPy, vectorised over the scenes and written from the
contract in include/mpinets_hip.h (not from csrc/scene_gen.hip): the Philox blocks of a scene (stream 19, counter
``{item, scene id, 19, block}``; item 0 the scene's parameters, item k + 1 object or plate k), the tabletop with its slot rule
stated as two ordered ranks, the cubby's seven plates and four pockets, the dresser's grid of plates with one volume each.

Every DISCRETE decision is the device's, exactly: a threshold compares the 24-bit uniform (exact in both precisions) with
the float32 constant, an integer draw is integer arithmetic, ``rows`` is the smallest integer whose square reaches ``n``.
Every other quantity is computed in float64 from the float32 constants the contract names, so it differs from the device's
by the device's rounding alone.
"""
import numpy as np

from float64_ik import philox4x32_np

STREAM_SCENE_GEN = 19
TABLETOP, CUBBY, DRESSER = 0, 1, 2
SURFACE, VOLUME = 1, 2
PRIMITIVE_KEYS = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights",
                  "cylinder_quats")
MAX_OBJECTS = 14  # the tabletop's K is 3 .. 14


def f(x):
    """The float32 constant nearest to ``x``, as a float64."""
    return float(np.float32(x))


PIO2, PI18, PI9, PI6, TWO_PI3 = (f(np.pi / 2), f(np.pi / 18), f(np.pi / 9), f(np.pi / 6), f(2 * np.pi / 3))


def blocks(item, ids, seed):
    """-> (words uint64 [...,8], u float64 [...,8]) of ``item`` (broadcast against ``ids``): block 0 then block 1."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    item, ids = np.broadcast_arrays(np.asarray(item, np.uint64), np.asarray(ids, np.uint64) & np.uint64(0xFFFFFFFF))
    w = np.stack(philox4x32_np(item, ids, STREAM_SCENE_GEN, 0, k0, k1) + philox4x32_np(item, ids, STREAM_SCENE_GEN, 1, k0, k1), -1)
    w = w.astype(np.uint64)
    return w, (w >> np.uint64(8)).astype(np.float64) / 2.0 ** 24


def draw_int(word, n):
    return (((word >> np.uint64(8)) * np.uint64(n)) >> np.uint64(24)).astype(np.int64)


def fma(a, b, c):
    return a * b + c


def yaw_quat(yaw):
    q = np.zeros(np.shape(yaw) + (4,))
    q[..., 0], q[..., 3] = np.cos(0.5 * yaw), np.sin(0.5 * yaw)
    return q


def place(yaw, lx, ly, lz, ox, oz):
    """W(l) of the contract -> [...,3]."""
    c, s = np.cos(yaw), np.sin(yaw)
    lx, ly, lz = np.broadcast_arrays(lx, ly, lz)
    return np.stack([(c * lx - s * ly) + ox, s * lx + c * ly, lz + oz], -1)


def _empty(n, M1, M2, S):
    out = dict(cuboid_centers=np.zeros((n, M1, 3)), cuboid_dims=np.zeros((n, M1, 3)), cuboid_quats=np.zeros((n, M1, 4)),
               cylinder_centers=np.zeros((n, M2, 3)), cylinder_radii=np.zeros((n, M2, 1)), cylinder_heights=np.zeros((n, M2, 1)),
               cylinder_quats=np.zeros((n, M2, 4)), support_boxes=np.zeros((n, S, 12)), support_kind=np.zeros((n, S), np.int32))
    out["cuboid_quats"][..., 0] = out["cylinder_quats"][..., 0] = out["support_boxes"][..., 6] = 1.0
    return out


def _support_rows(out, rows, slot, kind, centre, dims, quat, approach, weight):
    """Support ``slot`` of the scenes ``rows`` (kept when it fits into S)."""
    if slot < out["support_kind"].shape[1]:
        box = np.concatenate([centre, dims, quat, np.broadcast_to(approach, centre.shape[:1])[:, None],
                              np.broadcast_to(weight, centre.shape[:1])[:, None]], -1)
        out["support_boxes"][rows, slot], out["support_kind"][rows, slot] = box, kind


def tabletop(ids, M1, M2, S, seed):
    n = len(ids)
    out = _empty(n, M1, M2, S)
    w0, u = blocks(0, ids, seed)
    h = np.where(u[:, 0] < f(0.35), 0.0, u[:, 1] * f(0.4))
    x0, x1 = fma(u[:, 2], f(0.1), f(0.275)), fma(u[:, 3], f(0.1), f(1.275))
    w = fma(u[:, 4], f(0.15), 1.5)
    has_side = u[:, 5] < 0.5
    side = np.where(u[:, 6] < 0.5, -1.0, 1.0)
    K = 3 + draw_int(w0[:, 7], 12)
    T = np.where(has_side, 3, 2)
    every, zero, ident = np.arange(n), np.zeros(n), np.tile([1.0, 0, 0, 0], (n, 1))
    front_c, front_d = np.stack([(x0 + x1) * 0.5, zero, h - f(0.025)], -1), np.stack([x1 - x0, w, zero + f(0.05)], -1)
    out["cuboid_centers"][:, 0], out["cuboid_dims"][:, 0] = front_c, front_d
    _support_rows(out, every, 0, SURFACE, front_c, front_d, ident, 0.0, front_d[:, 0] * front_d[:, 1])
    sd = np.flatnonzero(has_side)
    side_c = np.stack([zero, side * fma(w, 0.25, f(0.45)), h - f(0.025)], -1)[sd]
    side_d = np.stack([zero + f(0.9), w * 0.5, zero + f(0.05)], -1)[sd]
    out["cuboid_centers"][sd, 1], out["cuboid_dims"][sd, 1] = side_c, side_d
    _support_rows(out, sd, 1, SURFACE, side_c, side_d, ident[sd], 0.0, side_d[:, 0] * side_d[:, 1])
    out["cuboid_centers"][every, T - 1], out["cuboid_dims"][every, T - 1] = [f(-0.35), 0.0, f(-0.025)], [f(0.6), f(0.6), f(0.05)]
    # the objects
    k = np.arange(MAX_OBJECTS)
    _, v = blocks(k[None] + 1, np.asarray(ids)[:, None], seed)  # [n,14,8]
    is_obj = k[None] < K[:, None]
    lo = (x0 + f(0.1))[:, None]
    px = fma(v[..., 0], (x1[:, None] - f(0.1)) - lo, lo)
    hw = (w * 0.5 - f(0.1))[:, None]
    py = fma(v[..., 1], hw + hw, -hw)
    drew = is_obj & (v[..., 2] < f(0.3))
    rank_c = np.cumsum(drew, 1) - drew
    is_cyl = drew & (rank_c < M2)
    cand = is_obj & ~is_cyl
    row_b = T[:, None] + np.cumsum(cand, 1) - cand
    kept = cand & (row_b < M1)
    hh = fma(v[..., 5], f(0.3), f(0.05))
    b, j = np.nonzero(is_cyl)
    out["cylinder_centers"][b, rank_c[b, j]] = np.stack([px[b, j], py[b, j], fma(hh[b, j], 0.5, h[b])], -1)
    out["cylinder_radii"][b, rank_c[b, j], 0] = fma(v[b, j, 4], f(0.1), f(0.05))
    out["cylinder_heights"][b, rank_c[b, j], 0] = hh[b, j]
    dz = fma(v[..., 6], f(0.3), f(0.05))
    b, j = np.nonzero(kept)
    out["cuboid_centers"][b, row_b[b, j]] = np.stack([px[b, j], py[b, j], fma(dz[b, j], 0.5, h[b])], -1)
    out["cuboid_dims"][b, row_b[b, j]] = np.stack([fma(v[b, j, 4], f(0.1), f(0.05)), fma(v[b, j, 5], f(0.1), f(0.05)), dz[b, j]], -1)
    out["cuboid_quats"][b, row_b[b, j]] = yaw_quat(v[b, j, 7] * PIO2)
    return out


def cubby(ids, M1, M2, S, seed):
    n = len(ids)
    out = _empty(n, M1, M2, S)
    _, u = blocks(0, ids, seed)
    t, W, H, D = fma(u[:, 0], f(0.02), f(0.01)), fma(u[:, 1], f(0.4), f(0.7)), fma(u[:, 2], f(0.4), 0.5), fma(u[:, 3], f(0.15), f(0.2))
    ox, oz = fma(u[:, 4], 0.25, f(0.55)), fma(u[:, 5], f(0.2), f(0.1))
    yaw = fma(u[:, 6], PI9, -PI18)
    hH, hW, ht, zero = H * 0.5, W * 0.5, t * 0.5, np.zeros(n)
    plates = [((zero, zero, zero), (D, W, t)), ((zero, zero, H), (D, W, t)), ((zero, zero, hH), (D, W, t)),
              ((zero, -hW, hH), (D, t, H)), ((zero, hW, hH), (D, t, H)), ((zero, zero, hH), (D, t, H)),
              ((D * 0.5, zero, hH), (t, W, H))]
    for i, (lc, dims) in enumerate(plates[:M1]):
        out["cuboid_centers"][:, i], out["cuboid_dims"][:, i] = place(yaw, *lc, ox, oz), np.stack(dims, -1)
        out["cuboid_quats"][:, i] = yaw_quat(yaw)
    for p in range(4):
        zi, yi = p >> 1, p & 1
        z0, z1 = (hH + ht, H - ht) if zi else (ht, hH - ht)
        y0, y1 = (ht, hW - ht) if yi else (-hW + ht, -ht)
        _support_rows(out, np.arange(n), p, VOLUME, place(yaw, -(t * 0.25), (y0 + y1) * 0.5, (z0 + z1) * 0.5, ox, oz),
                      np.stack([D - ht, y1 - y0, z1 - z0], -1), yaw_quat(yaw), 0.0, 1.0)
    return out


def dresser(ids, M1, M2, S, seed):
    n_scenes = len(ids)
    out = _empty(n_scenes, M1, M2, S)
    w0, u = blocks(0, ids, seed)
    W, D, H = fma(u[:, 0], f(0.4), f(0.8)), fma(u[:, 1], f(0.2), f(0.2)), fma(u[:, 2], f(0.3), f(0.55))
    ox = fma(u[:, 3], f(0.2), f(0.55))
    yaw = fma(u[:, 4], TWO_PI3, PI6)
    n = np.minimum(M1, 12 + draw_int(w0[:, 5], 29))
    rows = np.ones(n_scenes, np.int64)
    while (rows * rows < n).any():
        rows += rows * rows < n
    wc, hc = (W / rows)[:, None], (H / rows)[:, None]
    i = np.arange(M1)
    live = i[None] < n[:, None]
    _, v = blocks(i[None] + 1, np.asarray(ids)[:, None], seed)
    jitter = fma(v[..., 0], f(0.04), f(-0.02))
    ri, ci = i[None] // rows[:, None], i[None] % rows[:, None]
    lx = fma(ci + 0.5, wc, -(W * 0.5)[:, None])
    centre = place(yaw[:, None], lx, jitter, (ri + 0.5) * hc, ox[:, None], 0.0)
    dims = np.stack(np.broadcast_arrays(wc * f(0.95), D[:, None], hc * f(0.2)), -1) + 0 * centre
    quat = yaw_quat(np.broadcast_to(yaw[:, None], live.shape))
    out["cuboid_centers"][live], out["cuboid_dims"][live], out["cuboid_quats"][live] = centre[live], dims[live], quat[live]
    sup_c = place(yaw[:, None], lx, jitter, (ri + f(0.8)) * hc, ox[:, None], 0.0)
    sup_d = np.stack(np.broadcast_arrays(wc * f(0.95), D[:, None], hc * f(0.4)), -1) + 0 * centre
    for s in range(min(S, M1)):
        r = np.flatnonzero(live[:, s])
        _support_rows(out, r, s, VOLUME, sup_c[r, s], sup_d[r, s], quat[r, s], yaw[r] - PIO2, 1.0)
    return out


_KINDS = {TABLETOP: tabletop, CUBBY: cubby, DRESSER: dresser}


def generate(kind, ids, M1, M2, S, seed=0):
    """``mpx_scene_generate``: ``kind`` int [B] (a code outside 0..2: an empty scene), ``ids`` int [B] -> make_task_scenes'
    arrays in float64 (``support_kind`` int32); ``S`` = 0: no support keys (make_scenes' form)."""
    kind, ids = np.asarray(kind), np.asarray(ids, np.int64)
    assert 3 <= M1 <= 64 and 0 <= M2 <= 64 and 0 <= S <= 64
    out = _empty(len(kind), M1, M2, S)
    for code, gen in _KINDS.items():
        sel = np.flatnonzero(kind == code)
        if len(sel):
            part = gen(ids[sel], M1, M2, S, int(seed))
            for key in out:
                out[key][sel] = part[key]
    if S == 0:
        del out["support_boxes"], out["support_kind"]
    return out


def live_rows(scn):
    """-> bool masks (cuboids [B,M1], cylinders [B,M2], supports [B,S] or None): a row is live when it is not padding."""
    cub = (scn["cuboid_dims"] != 0).any(-1)
    cyl = (scn["cylinder_radii"][..., 0] != 0) | (scn["cylinder_heights"][..., 0] != 0)
    return cub, cyl, (scn["support_kind"] != 0 if "support_kind" in scn else None)
