"""Restatement of ``mpx_franka_plan_cloud`` on the CPU, in float64 by default, written from the contract in
include/mpinets_hip.h (not from csrc/cloud_field.hip).  What it shares with ``mpx_franka_plan`` is imported from
tests/float64_plan.py (candidates, the line, the metric, sphere centres, the jerk and self tests, the pick); what differs
is stated here: the environment term reads the distance field through ``float64_cloud_field.sample``, and environment
validity is the swept-sphere test against the cloud itself on the refined configurations, formed with the emulated fma.

Also here: the seeded inputs of tests/test_gpu_cloud_plan.py (the forced-detour wall as a cloud, the mixed scenes and
their clouds), so that tests/test_cloud_plan_host.py can run the same problems on the CPU.
"""
import numpy as np
import torch

import float64_cloud_field as fcf
import float64_plan as fp
from float64_ik import limits32
from mpinets_amd import franka_tables as ft

DEFAULTS = fp.DEFAULTS
FRAGILE = fp.FRAGILE  # [m], and cells for the face rule
UNDECIDED_CAP = 0.02  # share of candidates whose min_dist may come within DECIDE of the threshold
DECIDE = 1e-6         # [m]
VOXEL = 0.03


def truncation(point_radius=0.0, clearance=0.0, epsilon=DEFAULTS["epsilon"], voxel=VOXEL, with_base_link=False):
    """``robot.plan_cloud_truncation``, restated: max sphere radius + point_radius + clearance + epsilon + 2 voxels."""
    return float(ft.collision_sphere_table(with_base_link)[1].max()) + point_radius + max(clearance, 0.0) + epsilon + 2 * voxel


def default_grid(trunc, lo=fcf.REACH_LO, hi=fcf.REACH_HI, voxel=VOXEL):
    """``field.make_grid``, restated: node 0 on lo, spacing voxel, the last node on or past hi."""
    h = float(np.float32(voxel))
    n = [max(2, int(np.ceil((float(hi[a]) - float(lo[a])) / h - 1e-4)) + 1) for a in range(3)]
    return fcf.make_grid(n, lo, h, trunc)


def refine32(traj, substeps):
    """float32 [..,T,7] -> float32 [..,(T-1) substeps + 1,7]: fma((float)i / (float)substeps, q_{t+1} - q_t, q_t) as the
    device rounds it (the difference in float32, the fma's product and sum in float64, one rounding)."""
    q = np.asarray(traj, np.float32)
    a, b = q[..., :-1, None, :], q[..., 1:, None, :]
    f = (np.arange(substeps, dtype=np.float32) / np.float32(substeps))[:, None]
    body = (f.astype(np.float64) * (b - a).astype(np.float64) + a.astype(np.float64)).astype(np.float32)
    body[..., 0, :] = a[..., 0, :]
    return np.concatenate([body.reshape(q.shape[:-2] + (-1, 7)), q[..., -1:, :]], -2)


def obstacle_gradient(q, field, grid, K_T, point_radius=0.0, epsilon=0.05, clearance=0.0, with_base_link=False,
                      want_fragile=False):
    """q [B*K_T,7] (problem-major) -> g [B*K_T,7]; with ``want_fragile`` also bool [B*K_T]: a sphere with d within FRAGILE
    of 0 or epsilon, D within FRAGILE of trunc, or a centre within FRAGILE cells of a cell face."""
    dt = q.dtype
    x, R, t, radii, link = fp.sphere_centres(q, with_base_link)
    N, S = x.shape[:2]
    B = N // K_T
    pts = x.reshape(B, K_T * S, 3)
    # (the sampler takes float32 points; in float64 the centres are passed unrounded: widen by hand)
    D, n, inside, near = _sample_any(field, grid, pts, dt)
    D, n = D.reshape(N, S), n.reshape(N, S, 3)
    trunc = float(np.float32(grid["trunc"]))
    d = ((D - point_radius) - radii) - clearance
    live = D < trunc
    cp = torch.where(d < 0, -torch.ones_like(d), torch.where(d < epsilon, (d - epsilon) / epsilon, torch.zeros_like(d)))
    cp = torch.where(live, cp, torch.zeros_like(cp))
    w = n * cp[..., None]
    o, z = t[:, 1:8], R[:, 1:8, :, 2]
    cross = torch.cross(z[:, None].expand(N, S, 7, 3), x[:, :, None] - o[:, None], dim=-1)
    up = (torch.arange(7)[None, :] < link.clamp(max=7)[:, None]).to(dt)
    g = ((cross * w[:, :, None]).sum(-1) * up).sum(1)
    if want_fragile:
        # (The saturation switch and the faces matter only where c'(d) is not zero on both sides anyway, d < epsilon: with
        # the default truncation a sphere near saturation has d > epsilon + a cell, and taken literally "D within 1e-5 of
        # trunc" leaves out 8 % of the waypoints -- every cell with a saturated corner has samples that close.  D == trunc
        # exactly -- all eight corners saturated, or outside the grid -- is the same on both sides.)
        band = d < epsilon + FRAGILE
        fragile = (d.abs() < FRAGILE) | ((d - epsilon).abs() < FRAGILE) | \
                  (((D - trunc).abs() < FRAGILE) & (D != trunc) & band) | (near.reshape(N, S) & band)
        return g, fragile.any(-1)
    return g


def _sample_any(field, grid, pts, dt):
    """``fcf.sample`` on torch points of dtype ``dt`` WITHOUT rounding them to float32 first (the centres of a float64 run
    are float64 numbers)."""
    f = torch.as_tensor(np.asarray(field, np.float32)).to(dt)
    B, P = pts.shape[:2]
    n = torch.tensor([grid["nx"], grid["ny"], grid["nz"]])
    lo = torch.as_tensor(np.asarray(grid["lo"], np.float32)).to(dt)
    inv_h = torch.tensor(float(np.float32(1.0) / np.float32(grid["h"]))).to(dt)
    u = (pts - lo) * inv_h
    inside = torch.isfinite(pts).all(-1) & (u >= 0).all(-1) & (u <= (n - 1).to(dt)).all(-1)
    us = torch.where(inside[..., None], u, torch.zeros_like(u))
    i0 = torch.minimum(torch.floor(us).long(), n - 2)
    fr = us - i0.to(dt)
    fx, fy, fz = fr[..., 0], fr[..., 1], fr[..., 2]
    nx, ny = grid["nx"], grid["ny"]
    flat = f.reshape(B, -1)
    base = (i0[..., 2] * ny + i0[..., 1]) * nx + i0[..., 0]
    c = [[[torch.gather(flat, 1, base + (zz * ny + yy) * nx + xx) for xx in (0, 1)] for yy in (0, 1)] for zz in (0, 1)]
    fma = fcf._fma
    X = [[c[zz][yy][1] - c[zz][yy][0] for yy in (0, 1)] for zz in (0, 1)]
    a = [[fma(fx, X[zz][yy], c[zz][yy][0]) for yy in (0, 1)] for zz in (0, 1)]
    Y = [a[zz][1] - a[zz][0] for zz in (0, 1)]
    e = [fma(fy, Y[zz], a[zz][0]) for zz in (0, 1)]
    Z = e[1] - e[0]
    dist = fma(fz, Z, e[0])
    x0, x1 = fma(fy, X[0][1] - X[0][0], X[0][0]), fma(fy, X[1][1] - X[1][0], X[1][0])
    grad = torch.stack([inv_h * fma(fz, x1 - x0, x0), inv_h * fma(fz, Y[1] - Y[0], Y[0]), inv_h * Z], -1)
    trunc = torch.tensor(float(np.float32(grid["trunc"]))).to(dt)
    near = ((u.double() - torch.round(u.double())).abs() < FRAGILE).any(-1) & inside
    return torch.where(inside, dist, trunc), torch.where(inside[..., None], grad, torch.zeros_like(grad)), inside, near


def step(traj, L, field, grid, lo, hi, point_radius=0.0, step=DEFAULTS["step"], smooth_weight=DEFAULTS["smooth_weight"],
         epsilon=0.05, clearance=0.0, with_base_link=False, want_fragile=False):
    """One iteration on traj [B,K,T,7] (torch, its dtype) with L [B,T,7] and field float32 [B,nz,ny,nx] (None: no
    environment term) -> the next trajectory (and, with ``want_fragile``, bool [B,K,T-2])."""
    B, K, T, _ = traj.shape
    n = T - 2
    fragile = torch.zeros(B, K, max(n, 0), dtype=torch.bool)
    if n == 0:
        return (traj.clone(), fragile) if want_fragile else traj.clone()
    inner = traj[:, :, 1:-1]
    if field is not None:
        out = obstacle_gradient(inner.reshape(-1, 7), field, grid, K * n, point_radius, epsilon, clearance, with_base_link,
                                want_fragile)
        g, fr = out if want_fragile else (out, None)
        if want_fragile:
            fragile = fr.reshape(B, K, n)
        Mg = torch.einsum("tu,bkuj->bktj", fp.metric_inverse(n, traj.dtype), g.reshape(B, K, n, 7))
    else:
        Mg = torch.zeros_like(inner)
    new = inner - step * (smooth_weight * (inner - L[:, None, 1:-1]) + Mg)
    new = torch.minimum(torch.maximum(new, lo), hi)
    out = torch.cat([traj[:, :, :1], new, traj[:, :, -1:]], 2)
    return (out, fragile) if want_fragile else out


def cloud_min_distance(q, cloud, counts, K_R, point_radius, with_base_link=False):
    """q float64 [B*K_R,7] (problem-major) -> [B*K_R,S]: distance of every sphere centre to its environment's nearest
    usable point minus point_radius minus the sphere's radius (+inf without points), in float64."""
    x, _, _, radii, _ = fp.sphere_centres(q, with_base_link)
    N, S = x.shape[:2]
    B = N // K_R
    out = torch.full((N, S), float("inf"), dtype=torch.float64)
    cloud = np.asarray(cloud, np.float32)
    for b in range(B):
        n = cloud.shape[1] if counts is None else int(min(max(int(counts[b]), 0), cloud.shape[1]))
        p = fcf.usable(cloud[b], n)
        if p.shape[0] == 0:
            continue
        c = x[b * K_R:(b + 1) * K_R].reshape(-1, 3).double().numpy()
        d = fcf.nearest_distance(p, np.nan_to_num(c))  # (exact nearest neighbour, float64)
        out[b * K_R:(b + 1) * K_R] = torch.from_numpy(d).reshape(K_R, S) - point_radius - radii.double()
    return out


def validity(traj32, cloud, counts, point_radius=0.0, substeps=4, check_margin=1e-4, clearance=0.0, max_jerk=0.15,
             check_self=True, with_base_link=False):
    """traj32 float32 [B,K,T,7] (the waypoints as a float32 planner holds them) -> int32 [B,K] bits and float64 [B,K]:
    the smallest (distance - threshold) of the environment test (how decided bit 0 is)."""
    B, K, T, _ = traj32.shape
    bits = fp.validity(torch.from_numpy(np.asarray(traj32, np.float32)).double(), None, substeps, check_margin, clearance,
                       max_jerk, check_self, with_base_link)  # (no scene: the jerk and self bits)
    fine = refine32(traj32, substeps)
    Rn = fine.shape[2]
    reach = float(np.float32(clearance) + np.float32(check_margin))
    gap = cloud_min_distance(torch.from_numpy(fine.reshape(-1, 7)).double(), cloud, counts, K * Rn, point_radius,
                             with_base_link) - reach
    gap = gap.reshape(B, K, -1).amin(-1)
    bits = bits | (gap <= 0).to(torch.int32) * fp.BIT_ENV
    return bits, gap


def solve(q_start, q_goal, cloud, counts=None, field=None, grid=None, point_radius=0.0, limits=ft.JOINT_LIMITS_REAL, T=50,
          seed=0, env_offset=0, dtype=torch.float64, with_base_link=False, start=None, **options):
    """-> traj [B,T,7], status [B], choice [B], all_traj [B,K,T,7], all_status [B,K] (numpy), like
    ``robot.franka_plan_cloud`` with ``return_all``.  ``field`` None: built here by ``fcf.build_fast`` on the default grid
    with the default truncation."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    K = opt["candidates"]
    qs, qg = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    B = qs.shape[0]
    if field is None:
        grid = default_grid(truncation(point_radius, opt["clearance"], opt["epsilon"], VOXEL, with_base_link))
        field = fcf.build_fast(cloud, counts, grid)
    lim32 = limits32(limits)
    lim = torch.from_numpy(lim32).to(dtype)
    lo, hi = lim[:, 0], lim[:, 1]
    c0 = fp.candidates(qs, qg, limits, T, K, opt["spread"], seed, env_offset) if start is None else np.asarray(start, np.float32)
    traj, L = torch.from_numpy(c0).to(dtype), torch.from_numpy(fp.line(qs, qg, T)).to(dtype)
    ends = np.stack([c0[:, 0, 0], c0[:, 0, -1]], 1)[:, None]  # [B,1,2,7]
    bad = ~((ends >= lim32[:, 0]) & (ends <= lim32[:, 1])).all(-1).all(-1).all(-1)
    eb, _ = validity(np.nan_to_num(ends), cloud, counts, point_radius, 1, opt["check_margin"], opt["clearance"], np.inf,
                     opt["check_self"], with_base_link)
    status2 = bad | (eb[:, 0].numpy() != 0)
    for _ in range(opt["iterations"]):
        traj = step(traj, L, field, grid, lo, hi, point_radius, opt["step"], opt["smooth_weight"], opt["epsilon"],
                    opt["clearance"], with_base_link)
    all_traj = traj.numpy()
    bits, _ = validity(all_traj.astype(np.float32), cloud, counts, point_radius, opt["substeps"], opt["check_margin"],
                       opt["clearance"], opt["max_jerk"], opt["check_self"], with_base_link)
    all_bits = bits.numpy().astype(np.int32)
    out, status, choice = fp.pick(all_traj, all_bits)
    all_traj = all_traj.copy()
    out[status2], all_traj[status2], all_bits[status2] = np.nan, np.nan, fp.BIT_ENV | fp.BIT_SELF | fp.BIT_JERK
    status[status2], choice[status2] = 2, -1
    return out, status, choice, all_traj, all_bits


# ---- seeded inputs of the GPU tests ------------------------------------------------------------------------------------------

WALL_SPACING, WALL_POINT_RADIUS = 0.02, 0.02  # (a 2 cm lattice: no surface point farther than 1.42 cm from a lattice point)
DETOUR_B, DETOUR_SEED = 24, 77


def both_limits():
    return np.stack([np.maximum(ft.JOINT_LIMITS_REAL[:, 0], ft.JOINT_LIMITS_PUBLISHED[:, 0]),
                     np.minimum(ft.JOINT_LIMITS_REAL[:, 1], ft.JOINT_LIMITS_PUBLISHED[:, 1])], 1)


def cube_cloud(centre, side=0.1, spacing=WALL_SPACING):
    """centre float32 [B,3] -> float32 [B,N,3]: the surface lattice of a cube (the wall of test_gpu_plan.py's forced
    detour, drawn as a cloud)."""
    m = int(round(side / spacing)) + 1
    t = (np.arange(m, dtype=np.float64) * spacing - side / 2)
    g = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
    shell = g[(np.abs(np.abs(g) - side / 2) < 1e-9).any(-1)]
    return (np.asarray(centre, np.float64)[:, None] + shell[None]).astype(np.float32)


def detour_problems(B=DETOUR_B, seed=DETOUR_SEED):
    """The forced detour of tests/test_gpu_plan.py (first B of its rows: the same generator, the same seed): one 10 cm
    cube per problem, centred on the first link-4 collision sphere of the configuration halfway along the straight line.
    -> q_start, q_goal float32 [B,7], limits, cloud float32 [B,N,3], cube centres."""
    lim = both_limits()
    rng = np.random.default_rng(seed)
    qs, qg = ((lim[:, 0] + rng.random((256, 7)) * (lim[:, 1] - lim[:, 0])).astype(np.float32)[:B] for _ in range(2))
    mid = torch.from_numpy(fp.line(qs, qg, 3)[:, 1]).double()
    x, _, _, _, link = fp.sphere_centres(mid)
    centre = x[:, int(torch.nonzero(link == 4)[0, 0])].numpy().astype(np.float32)
    return qs, qg, lim, cube_cloud(centre), centre


def scene_cloud_points(scn, num_points, seed):
    """``scenes.sample_scene_clouds_host``: float32 [B,num_points,3] on the primitives' surfaces."""
    from mpinets_amd import scenes

    return scenes.sample_scene_clouds_host(scn, num_points, seed).astype(np.float32)
