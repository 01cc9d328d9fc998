"""Restatement of the three training-loss entries of csrc/loss.hip on the CPU, in float64 by default, written from the
contract in include/mpinets_hip.h: ``mpx_collision_hinge`` per point, ``mpx_point_match`` per element and
``mpx_franka_cloud_grad`` per joint.

Every function takes the float32 arrays the device reads (stored inverse frames, sizes, points, q, the point table) and
evaluates in ``dtype``; ``torch.float32`` runs the same statements in float32: the reference-against-reference
measurement the tolerances of tests/test_gpu_loss_float64.py are computed from.  The hinge stands on
``float64_plan.sdf_min_grad`` (first minimum, cuboids before cylinders), so what pins the loss also pins the obstacle
gradient both planners descend on.

The seeded builders at the end make the inputs of the GPU tests; tests/test_loss_host.py checks the restatement and the
leave-out caps on the same arrays without a GPU.
"""
import collections
import functools
import math

import numpy as np
import torch

import float64_plan as fp
from mpinets_amd import franka_tables as ft
from mpinets_amd import scenes
from oracle import oracle as orc

FRAGILE = fp.FRAGILE
EPS32 = 2.0 ** -24
MIXED = ("tabletop", "cubby", "dresser")
NAMES = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights",
         "cylinder_quats")
LINKS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 13)  # the links that own rows of link_point_table (0 only with the base link)
FAR_POINT = (5.0, 5.0, 5.0)  # padding rows of the region cases: outside every margin, zero hinge


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---------------------------------------------------------------- collision hinge
def hinge(points, scene, margin=0.03, dtype=torch.float64):
    """points float32 [B,N,3], scene: the dict of ``float64_plan.scene_from_arrays`` (float32 inverse frames and sizes)
    -> dict of torch tensors in ``dtype``: ``sdf`` [B,N] (+inf without a live primitive), ``h`` = max(0, margin - sdf)
    [B,N], ``loss_sum`` [B], ``grad`` [B,N,3] = -(world gradient of the arg-min primitive) where h > 0 and +0 elsewhere,
    and bool ``leave_out`` [B,N]: ``sdf_min_grad``'s fragile points and the hinge's own kink |margin - sdf| < FRAGILE.
    ``margin`` enters as the float32 the entry receives."""
    x = _t(np.asarray(points, np.float32), dtype)
    B, N = x.shape[:2]
    m = float(np.float32(margin))
    if N == 0:
        z = torch.zeros(B, 0, dtype=dtype)
        return {"sdf": z, "h": z, "loss_sum": torch.zeros(B, dtype=dtype), "grad": torch.zeros(B, 0, 3, dtype=dtype),
                "leave_out": torch.zeros(B, 0, dtype=torch.bool)}
    sdf, g, fragile = fp.sdf_min_grad(x, scene, want_fragile=True)
    h = torch.clamp(m - sdf, min=0)
    grad = torch.where((h > 0)[..., None], -g, torch.zeros_like(g))
    return {"sdf": sdf, "h": h, "loss_sum": h.sum(1), "grad": grad, "leave_out": fragile | ((m - sdf).abs() < FRAGILE)}


def hinge_pair(points, scene, margin=0.03):
    """The float64 and the float32 evaluation of one case, and the figures the tolerances are made of: ``e32`` (largest
    float32-versus-float64 deviation of the gradient over the kept points), ``h32`` (the same of h over all points),
    ``active`` [B] (points with h > 0) and ``left_out`` (share of the points)."""
    r64, r32 = hinge(points, scene, margin), hinge(points, scene, margin, torch.float32)
    keep = ~r64["leave_out"]
    dg = (r32["grad"].double() - r64["grad"]).abs().amax(-1)
    r64["keep"] = keep
    r64["e32"] = float(dg[keep].max()) if bool(keep.any()) else 0.0
    r64["h32"] = float((r32["h"].double() - r64["h"]).abs().max()) if keep.numel() else 0.0
    r64["active"] = (r64["h"] > 0).sum(1)
    r64["left_out"] = float((~keep).double().mean()) if keep.numel() else 0.0
    return r64


def loss_sum_bound(r, N):
    """[B]: N_active * 4 * max|h32 - h64| (the per-term rounding, measured on the restatement) + (ceil(N / 256) + 16) *
    2^-24 * want (the kernel's fixed-order sum: ceil(N / 256) terms per thread, 6 shuffle adds, up to 4 adds)."""
    return r["active"].double() * 4 * r["h32"] + (math.ceil(N / 256) + 16) * EPS32 * r["loss_sum"]


# ---------------------------------------------------------------- point match
def point_match(a, t, w_sq, w_abs, dtype=torch.float64):
    """a, t float32 [B,n] -> sums [B,2] = (sum d^2, sum |d|) and grad [B,n] = 2 w_sq d + w_abs sign(d), sign(0) = 0; the
    weights enter as the float32 values the entry receives."""
    d = _t(np.asarray(a, np.float32), dtype) - _t(np.asarray(t, np.float32), dtype)
    ws, wa = float(np.float32(w_sq)), float(np.float32(w_abs))
    return torch.stack([(d * d).sum(1), d.abs().sum(1)], 1), 2 * ws * d + wa * torch.sign(d)


# ---------------------------------------------------------------- robot-cloud backward
def cloud_grad(q, finger, table_pts, table_link, subset, g, dtype=torch.float64):
    """q float32 [B,7], g float32 [B,n,3] -> gq [B,7] by autograd of ``oracle.robot_cloud_torch``, and A [B,7] =
    sum_j |p_j - o_k| |g_j| over the rows j that joint k moves (k < min(link_j, 7); o_k the origin of frame k + 1): the
    size of the terms the sum is made of, the scale the tolerance is stated in."""
    qq = _t(np.asarray(q, np.float32), dtype).requires_grad_(True)
    gg = _t(np.asarray(g, np.float32), dtype)
    f = float(np.float32(finger))
    cloud = orc.robot_cloud_torch(qq, table_pts, table_link, subset, f)
    (cloud * gg).sum().backward()
    gq = torch.zeros_like(qq) if qq.grad is None else qq.grad.detach()
    with torch.no_grad():
        _, t = orc.fk_frames_torch(qq.detach(), f)
        link = torch.from_numpy(np.asarray(table_link)).long()
        if subset is not None:
            link = link[torch.from_numpy(np.asarray(subset)).long()]
        arm = (cloud.detach()[:, :, None] - t[:, None, 1:8]).norm(dim=-1)  # [B,n,7]
        up = (torch.arange(7)[None, :] < link.clamp(max=7)[:, None]).to(dtype)  # [n,7]
        A = (arm * up * gg.norm(dim=-1)[:, :, None]).sum(1)
    return gq, A


def cloud_grad_pair(q, finger, table_pts, table_link, subset, g):
    """-> gq64, A64, c32 = the largest |gq32 - gq64| / (2^-24 A) over the entries with A > 0."""
    gq, A = cloud_grad(q, finger, table_pts, table_link, subset, g)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (the order of torch's float32 sums over 1024 rows, and with it this figure, follows the
    try:                      # thread count: 0.18 .. 0.28 on one input; one thread gives the same figure everywhere)
        g32, _ = cloud_grad(q, finger, table_pts, table_link, subset, g, torch.float32)
    finally:
        torch.set_num_threads(threads)
    on = A > 0
    c32 = float(((g32.double() - gq).abs()[on] / (EPS32 * A[on])).max()) if bool(on.any()) else 0.0
    return gq, A, c32


# ---------------------------------------------------------------- H2: regions by construction
def _axis_names(state):
    return "".join("-0+"[s + 1] for s in state)


def cuboid_labels(p, dims):
    """Local points p [P,3] (float64), full sizes -> one label per point: ``corner+-+`` / ``edge+0-`` / ``face0+0`` (the
    sign of each outside axis, 0 for an axis between its faces) or ``inside`` + the nearest axis and the point's sign on
    it (``inside1-``)."""
    d = np.abs(p) - np.asarray(dims, np.float64) / 2
    out = []
    for pi, di in zip(p, d):
        outside = di > 0
        if outside.any():
            kind = {3: "corner", 2: "edge", 1: "face"}[int(outside.sum())]
            out.append(kind + _axis_names(np.where(outside, np.sign(pi), 0).astype(int)))
        else:
            a = int(np.argmax(di))
            out.append(f"inside{a}{'+' if pi[a] > 0 else '-'}")
    return out


def cylinder_labels(p, radius, height):
    """``side``, ``cap+-``, ``rim+-``, ``inside_radial``, ``inside_axial+-``; ``axis_`` in front when rho is exactly 0."""
    rho = np.hypot(p[:, 0], p[:, 1])
    d0, d1 = rho - radius, np.abs(p[:, 2]) - height / 2
    out = []
    for r, a, b, z in zip(rho, d0, d1, p[:, 2]):
        s = "+" if z > 0 else "-"
        if a > 0 and b > 0:
            lab = "rim" + s
        elif a > 0:
            lab = "side"
        elif b > 0:
            lab = "cap" + s
        else:
            lab = "inside_radial" if a > b else "inside_axial" + s
        out.append(("axis_" if r == 0.0 else "") + lab)
    return out


CUBOID_LABELS = tuple(sorted(
    [k + _axis_names(s) for s in np.ndindex(3, 3, 3) for s in [tuple(v - 1 for v in s)]
     for k in [{3: "corner", 2: "edge", 1: "face"}.get(sum(v != 0 for v in s))] if k]
    + [f"inside{a}{s}" for a in range(3) for s in "+-"]))  # 8 + 12 + 6 + 6
CYLINDER_LABELS = ("side", "cap+", "cap-", "rim+", "rim-", "inside_radial", "inside_axial+", "inside_axial-")
AXIS_LABELS = ("axis_cap+", "axis_cap-", "axis_inside_radial", "axis_inside_axial+", "axis_inside_axial-")
GAP = 2e-3  # the generator's distance from every switch, in local coordinates [m] (the issue's floor is 1e-3)


def regions(kind, frame, size, seed, per_label=16):
    """One live primitive -> world points float32 [P,3] in every region of its gradient, ``per_label`` per label, and the
    label of each.  Points are made in LOCAL coordinates at least GAP from every switch (a face plane, a sign change, the
    tie of the largest d, the axis), mapped to the world in float64 through the inverse of the STORED 3x3 block (which
    need not be a rotation), rounded to float32 and labelled again in float64 from what the stored frame makes of the
    rounded point.  kind: "cuboid" (size = dims [3]), "cylinder" (size = (radius, height)) or "axis" (a cylinder, points
    exactly on its axis: the frame must be axis aligned, so that a float32 world point projects back to rho == 0)."""
    rng = np.random.default_rng(seed)
    F = np.asarray(frame, np.float64)
    M, t = F[:3, :3], F[:3, 3]
    local = []
    if kind == "cuboid":
        half = np.asarray(size, np.float64) / 2
        assert half.min() >= 0.04
        for state in np.ndindex(3, 3, 3):
            state = np.asarray(state) - 1
            if not state.any():
                continue
            p = np.empty((per_label, 3))
            for i in range(3):
                if state[i]:
                    p[:, i] = state[i] * (half[i] + rng.uniform(GAP, 0.06, per_label))
                else:
                    p[:, i] = rng.choice([-1.0, 1.0], per_label) * rng.uniform(GAP, half[i] - GAP, per_label)
            local.append(p)
        for a in range(3):
            for s in (1.0, -1.0):
                da = -rng.uniform(GAP, 0.015, per_label)  # the largest d
                p = np.empty((per_label, 3))
                for i in range(3):
                    if i == a:
                        p[:, i] = s * (half[i] + da)
                    else:
                        di = rng.uniform(-half[i] + GAP, da - GAP)
                        p[:, i] = rng.choice([-1.0, 1.0], per_label) * (half[i] + di)
                local.append(p)
    elif kind == "cylinder":
        r, hh = float(size[0]), float(size[1]) / 2
        assert min(r, hh) >= 0.04

        def polar(rho, z):
            th = rng.uniform(0, 2 * np.pi, per_label)
            return np.stack([rho * np.cos(th), rho * np.sin(th), z], -1)

        u = lambda lo, hi: rng.uniform(lo, hi, per_label)
        local.append(polar(r + u(GAP, 0.06), rng.choice([-1.0, 1.0], per_label) * u(GAP, hh - GAP)))  # side
        for s in (1.0, -1.0):
            local.append(polar(u(GAP, r - GAP), s * (hh + u(GAP, 0.06))))  # cap
            local.append(polar(r + u(GAP, 0.06), s * (hh + u(GAP, 0.06))))  # rim
        d0 = -u(GAP, 0.015)
        local.append(polar(r + d0, rng.choice([-1.0, 1.0], per_label) * (hh + rng.uniform(-hh + GAP, d0 - GAP))))
        for s in (1.0, -1.0):
            d1 = -u(GAP, 0.015)
            local.append(polar(r + rng.uniform(-r + GAP, d1 - GAP), s * (hh + d1)))
    else:
        r, hh = float(size[0]), float(size[1]) / 2
        assert abs(r - hh) > 0.02 and np.array_equal(M, np.eye(3)), "the axis case needs an axis-aligned frame"
        z = lambda lo, hi: np.stack([np.zeros(per_label), np.zeros(per_label), rng.uniform(lo, hi, per_label)], -1)
        for s in (1.0, -1.0):
            local.append(s * z(hh + GAP, hh + 0.06))  # above / below a cap
            if r < hh:  # -r > d1 possible: radially nearest for |z| < hh - r, axially nearest above
                local.append(s * z(GAP, hh - r - GAP))
                local.append(s * z(hh - r + GAP, hh - GAP))
            else:  # d1 = |z| - hh > -r always: axially nearest
                local.append(s * z(GAP, hh - GAP))
    p = np.concatenate(local)
    x = np.linalg.solve(M, (p - t).T).T.astype(np.float32)
    if kind == "axis":
        x[:, :2] = (-t[:2]).astype(np.float32)  # the centre's own floats: x + t == 0 exactly
    back = x.astype(np.float64) @ M.T + t
    labels = cuboid_labels(back, size) if kind == "cuboid" else cylinder_labels(back, float(size[0]), float(size[1]))
    return x, labels


# ---------------------------------------------------------------- seeded builders (shared by the host and GPU tests)
def band_points(scn, N, seed, near=1300):
    """N points per environment: ``near`` of them (scaled down with N) inside the band -0.05 < sdf < 0.03 around the
    obstacles' surfaces, the rest far (sdf > 0.1), shuffled.  -> float32 [B,N,3]."""
    scene = fp.scene_from_arrays(scn)
    B = scn["cuboid_dims"].shape[0]
    rng = np.random.default_rng(seed + 1)
    n_near = (near * N) // 1500
    pts = np.empty((B, N, 3), np.float32)
    surf = scenes.sample_scene_clouds_host(scn, 8 * max(N, 1), seed).astype(np.float64)
    cand = (surf + rng.normal(scale=0.03, size=surf.shape)).astype(np.float32)
    far = rng.uniform([-0.8, -1.2, -0.3], [1.6, 1.2, 1.3], size=(B, 8 * max(N, 1), 3)).astype(np.float32)
    sdf_c, _, _ = fp.sdf_min_grad(torch.from_numpy(cand).double(), scene)
    sdf_f, _, _ = fp.sdf_min_grad(torch.from_numpy(far).double(), scene)
    for b in range(B):
        a = cand[b][((sdf_c[b] > -0.05) & (sdf_c[b] < 0.03)).numpy()][:n_near]
        f = far[b][(sdf_f[b] > 0.1).numpy()][:N - n_near]
        assert len(a) == n_near and len(f) == N - n_near, (b, len(a), len(f))
        pts[b] = np.concatenate([a, f])[rng.permutation(N)]
    return pts


@functools.lru_cache(maxsize=None)
def h1_case(B=6, N=1500, M1=40, M2=16, seed=11):
    """Mixed tabletop / cubby / dresser scenes and N points each (``band_points``).  -> scn arrays, points [B,N,3]."""
    scn = scenes.make_scenes(B, seed, MIXED, M1, M2)
    return scn, band_points(scn, N, seed)


@functools.lru_cache(maxsize=None)
def cylinders_case(B=2, N=257, seed=13):
    """Tabletop scenes without their cuboids (M1 = 0), the points around the cylinders."""
    scn = scenes.make_scenes(B, seed, ("tabletop",), 8, 16)
    scn["cuboid_dims"] = np.zeros_like(scn["cuboid_dims"])
    assert (scn["cylinder_radii"][:, 0, 0] > 0).all()
    return only_cylinders(scn), band_points(scn, N, seed)


def slice_case(scn, pts, envs, N):
    """The environments ``envs`` and the first N points of a case."""
    envs = list(envs)
    return {k: np.ascontiguousarray(v[envs]) for k, v in scn.items()}, np.ascontiguousarray(pts[envs, :N])


def only_cuboids(scn):
    out = dict(scn)
    for k in ("cylinder_centers", "cylinder_radii", "cylinder_heights", "cylinder_quats"):
        out[k] = scn[k][:, :0]
    return out


def only_cylinders(scn):
    out = dict(scn)
    for k in ("cuboid_centers", "cuboid_dims", "cuboid_quats"):
        out[k] = scn[k][:, :0]
    return out


def with_masked_rows(scn):
    """Zero-volume primitives at index 0 and between the live ones, each a copy of a live neighbour grown threefold with
    one size at (or within 1e-8 of) zero: read as live, it would be the nearest primitive of many points.  The live rows
    move to other indices, so the arg-min index of the unfiltered arrays is what picks the frame."""
    out = {k: v.copy() for k, v in scn.items()}
    B = scn["cuboid_dims"].shape[0]

    def insert(keys, size_keys, at, src, kill):
        for k in keys:
            row = scn[k][:, src:src + 1].copy()
            if k in size_keys:
                row = row * 3
                kill(k, row)
            out[k] = np.concatenate([out[k][:, :at], row, out[k][:, at:]], 1)

    cub, cyl = NAMES[:3], NAMES[3:]

    def kill_cub(axis, value):
        def f(k, row):
            row[:, :, axis] = value
        return f

    def kill_cyl(which, value):
        def f(k, row):
            if k == which:
                row[...] = value
        return f

    insert(cub, ("cuboid_dims",), 2, 1, kill_cub(2, 5e-9))  # between live 1 and live 2 (placed first: indices of `out`)
    insert(cub, ("cuboid_dims",), 0, 0, kill_cub(0, 0.0))
    if scn["cylinder_radii"].shape[1]:
        insert(cyl, ("cylinder_radii", "cylinder_heights"), 1, 0, kill_cyl("cylinder_heights", 0.0))
        insert(cyl, ("cylinder_radii", "cylinder_heights"), 0, 0, kill_cyl("cylinder_radii", -5e-9))
    assert out["cuboid_dims"].shape[0] == B
    return out


def with_repeated_cuboid(scn, which=1):
    """Cuboid ``which`` listed a second time, at the end."""
    out = dict(scn)
    for k in NAMES[:3]:
        out[k] = np.concatenate([scn[k], scn[k][:, which:which + 1]], 1)
    return out


# quaternions (w, x, y, z) with roll and pitch; the second and fourth are not unit length
H2_QUATS = ((0.9, 0.3, 0.2, 0.1), (1.7, -0.8, 1.1, 0.6), (0.8, 0.5, -0.2, 0.1), (-1.2, 0.9, 0.7, -1.5))
H2_KINDS = ("cuboid", "cuboid", "cylinder", "cylinder", "axis")


def h2_scene():
    """Five environments with one live primitive each (M1 = M2 = 1, the other row zero-volume): two cuboids and two
    cylinders in frames of quaternions with roll, the last a cylinder in an axis-aligned frame for the on-axis labels."""
    z3, q0 = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]
    scn = {"cuboid_centers": [[[0.4, 0.1, 0.3]], [[0.1, -0.4, 0.5]], [z3], [z3], [z3]],
           "cuboid_dims": [[[0.3, 0.2, 0.25]], [[0.2, 0.4, 0.1]], [z3], [z3], [z3]],
           "cuboid_quats": [[list(H2_QUATS[0])], [list(H2_QUATS[1])], [q0], [q0], [q0]],
           "cylinder_centers": [[z3], [z3], [[-0.3, 0.3, 0.2]], [[0.3, 0.5, 0.6]], [[0.37, -0.21, 0.45]]],
           "cylinder_radii": [[[0.0]], [[0.0]], [[0.1]], [[0.15]], [[0.07]]],
           "cylinder_heights": [[[0.0]], [[0.0]], [[0.3]], [[0.12]], [[0.3]]],
           "cylinder_quats": [[q0], [q0], [list(H2_QUATS[2])], [list(H2_QUATS[3])], [q0]]}
    return {k: np.asarray(v, np.float32) for k, v in scn.items()}


def frame_defect(frame):
    """max |M M^T - I| of the stored 3x3 block."""
    M = np.asarray(frame, np.float64)[:3, :3]
    return float(np.abs(M @ M.T - np.eye(3)).max())


def h2_case(scene, per_label=16):
    """``scene``: the scene dict of ``h2_scene`` (with the frames the caller will hand to the device) -> points float32
    [5,N,3] (padded to one N with FAR_POINT rows, label ``far``) and the labels [5][N]."""
    scn = h2_scene()
    xs, labs = [], []
    for b, kind in enumerate(H2_KINDS):
        if kind == "cuboid":
            x, lab = regions(kind, scene["cub_frames"][b, 0], scn["cuboid_dims"][b, 0], 100 + b, per_label)
        else:
            x, lab = regions(kind, scene["cyl_frames"][b, 0],
                             (scn["cylinder_radii"][b, 0, 0], scn["cylinder_heights"][b, 0, 0]), 100 + b,
                             per_label if kind == "axis" else 2 * per_label)
        xs.append(x), labs.append(lab)
    N = max(len(x) for x in xs)
    pts = np.tile(np.asarray(FAR_POINT, np.float32), (len(xs), N, 1))
    for b, x in enumerate(xs):
        pts[b, :len(x)] = x
        labs[b] = labs[b] + ["far"] * (N - len(x))
    return pts, labs


def h2_keep(labels, leave_out):
    """The kept points of a region case: not left out -- but an ``axis_`` label is ON a switch by construction (rho == 0,
    where both sides state the zero radial part), so its points are kept whatever ``leave_out`` says of them; the
    generator holds them GAP away from every OTHER switch."""
    keep = ~np.asarray(leave_out)
    for b, row in enumerate(labels):
        for j, lab in enumerate(row):
            if lab.startswith("axis_"):
                keep[b, j] = True
    return keep


def tie_case():
    """Exact ties of the largest d INSIDE a primitive, by construction: a cube and a cylinder (radius = half height) at the
    origin of axis-aligned frames, where the float32 projection is exact, and points whose tied components are the same
    float.  The code takes the FIRST largest (torch.max on the CPU does; the reference's autograd splits such a
    gradient, which nobody follows).  -> scn (environment 0: the cube, 1: the cylinder), points float32 [2,N,3], and the
    expected gradient of loss_sum [2,N,3] (minus the unit step along the first tied axis, signed like the point)."""
    z3, q0 = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]
    scn = {"cuboid_centers": [[z3], [z3]], "cuboid_dims": [[[0.2, 0.2, 0.2]], [z3]], "cuboid_quats": [[q0], [q0]],
           "cylinder_centers": [[z3], [z3]], "cylinder_radii": [[[0.0]], [[0.1]]], "cylinder_heights": [[[0.0]], [[0.2]]],
           "cylinder_quats": [[q0], [q0]]}
    scn = {k: np.asarray(v, np.float32) for k, v in scn.items()}
    cube, want_cube, cyl, want_cyl = [], [], [], []
    for a in (0.05, 0.07, 0.093):
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                cube += [(s0 * a, s1 * a, 0.01), (s0 * a, 0.01, s1 * a), (0.01, s0 * a, s1 * a), (s0 * a, s1 * a, s0 * a)]
                want_cube += [(-s0, 0, 0), (-s0, 0, 0), (0, -s0, 0), (-s0, 0, 0)]
    for a in (0.0625, 0.03125):  # (powers of two: (1 / rho) * p is the unit step exactly)
        for s0 in (1.0, -1.0):
            for s1 in (1.0, -1.0):
                cyl += [(s0 * a, 0.0, s1 * a), (0.0, s0 * a, s1 * a)]  # rho == |z|: radial first
                want_cyl += [(-s0, 0, 0), (0, -s0, 0)]
    N = len(cube)
    pts = np.tile(np.asarray(FAR_POINT, np.float32), (2, N, 1))
    want = np.zeros((2, N, 3))
    pts[0], want[0] = np.asarray(cube, np.float32), want_cube
    pts[1, :len(cyl)], want[1, :len(cyl)] = np.asarray(cyl, np.float32), want_cyl
    return scn, pts, want


H2_MARGIN = 0.2  # every region point is within 0.06 sqrt(3) of the surface in local coordinates: all hinges active
LAUNCH_EDGES = tuple((B, N) for B in (1, 3) for N in (0, 1, 255, 256, 257))


def hinge_cases():
    """name -> (scn arrays, points float32 [B,N,3], margin): every input of the GPU hinge tests that is judged by the
    restatement (the region case ``h2`` is made by ``h2_case`` around the caller's frames)."""
    scn, pts = h1_case()
    small, small_pts = h1_case(B=3, N=257, M1=12, M2=4)
    cases = {"h1": (scn, pts, 0.03)}
    for B, N in LAUNCH_EDGES:
        # (from environment 1 on: environment 0's coplanar table tops put 2 % of its points on a tie of two distances,
        # which fits the cap among 1500 points of six scenes and not alone)
        cases[f"h3_B{B}_N{N}"] = slice_case(scn, pts, range(1, 1 + B), N) + (0.03,)
    cases["h3_no_cuboids"] = cylinders_case() + (0.03,)
    s, p = slice_case(scn, pts, range(3), 257)
    cases["h3_no_cylinders"] = (only_cuboids(s), p, 0.03)
    cases["h3_masked"] = (with_masked_rows(small), small_pts, 0.03)
    s, p = slice_case(scn, pts, range(3), 600)
    cases["h5_margin_0"] = (s, p, 0.0)
    cases["h5_margin_0.1"] = (s, p, 0.1)
    return cases


@functools.lru_cache(maxsize=None)
def point_match_case(n, seed=21, B=3):
    """input, target float32 [B,n]; about 1 % of the entries are equal exactly."""
    rng = np.random.default_rng(seed + n)
    a = rng.normal(scale=0.4, size=(B, n)).astype(np.float32)
    t = (a + rng.normal(scale=0.05, size=(B, n))).astype(np.float32)
    same = rng.random((B, n)) < 0.01
    if n >= 2:
        same[0, 1] = True
    t[same] = a[same]
    return a, t


@functools.lru_cache(maxsize=None)
def cloud_q(B=4, seed=31):
    """q float32 [B,7] inside the limits; row 1 all zeros, row 2 on the limits (lower for even joints, upper for odd)."""
    lim = fp.limits32(ft.JOINT_LIMITS_REAL)
    rng = np.random.default_rng(seed)
    q = (lim[:, 0] + rng.random((B, 7)).astype(np.float32) * (lim[:, 1] - lim[:, 0])).astype(np.float32)
    q = np.minimum(np.maximum(q, lim[:, 0]), lim[:, 1])
    q[1] = 0.0
    q[2] = np.where(np.arange(7) % 2 == 0, lim[:, 0], lim[:, 1])
    return q


@functools.lru_cache(maxsize=None)
def cloud_case(n, with_base_link, seed=41, B=4, link=None, repeats=False):
    """-> table_pts float32 [4096,3], table_link int32 [4096], subset int32 [n], g float32 [B,n,3].  ``link``: the subset
    holds rows of that link only (all of them, repeated to fill, where it owns fewer than n); ``repeats``: a subset drawn
    with replacement from 64 rows."""
    pts, lnk = ft.link_point_table(4096, with_base_link)
    rng = np.random.default_rng(seed + 7 * n + int(with_base_link))
    if link is not None:
        rows = np.nonzero(lnk == link)[0]
        assert len(rows) > 0, link
        sub = np.resize(rows, n) if len(rows) < n else rng.choice(rows, n, replace=False)
    elif repeats:
        sub = rng.choice(rng.choice(4096, 64, replace=False), n, replace=True)
    else:
        sub = rng.choice(4096, n, replace=False)
    g = rng.normal(size=(B, n, 3)).astype(np.float32)
    return np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(lnk, np.int32), sub.astype(np.int32), g


class CloudCase(collections.namedtuple("CloudCase", "name n base finger link repeats null_subset",
                                       defaults=(0.025, None, False, False))):
    """One input of the robot-cloud backward tests: n rows (of ``link`` only / drawn with repeats / the whole table with a
    NULL subset) of the table with or without the base link, at a finger opening."""


CLOUD_GROUPS = {
    "g1": [CloudCase("g1_base0", 1024, False), CloudCase("g1_base1", 1024, True)],
    "g2": [CloudCase(f"g2_link{l}", 256, l == 0, link=l) for l in LINKS],
    "g3": [CloudCase(f"g3_n{n}", n, False) for n in (0, 1, 255, 257)]
          + [CloudCase("g3_null_subset", 4096, False, null_subset=True), CloudCase("g3_repeats", 1024, True, repeats=True)],
    "g5": [CloudCase(f"g5_finger{f}{'_tips' if link else ''}", 64 if link else 1024, False, f, link)
           for f in (0.0, 0.025, 0.04) for link in (None, 12)],
}


@functools.lru_cache(maxsize=None)
def cloud_group(group):
    """-> {name: (case, (q, table_pts, table_link, subset, g), gq64, A)} and c32 over the whole group: the restatement is
    evaluated once for all the tests of a group, and the float32 figure is the largest over all of its inputs."""
    out, c32 = {}, 0.0
    q = cloud_q()
    for c in CLOUD_GROUPS[group]:
        tp, tl, sub, g = cloud_case(c.n, c.base, link=c.link, repeats=c.repeats)
        if c.null_subset:
            assert c.n == tp.shape[0]
            sub = None
        gq, A, c1 = cloud_grad_pair(q, c.finger, tp, tl, sub, g)
        out[c.name] = (c, (q, tp, tl, sub, g), gq, A)
        c32 = max(c32, c1)
    return out, c32
