"""Restatement of ``mpx_franka_roadmap_cloud`` and of ``mpx_franka_plan_cloud_seeded`` on the CPU, in float64 by default,
written from the contract in include/mpinets_hip.h (not from csrc/roadmap_cloud.hip).  Everything but the validity test is
tests/float64_roadmap.py's (the node draws, the lazy search, resampling and the corner filter); the validity test is stated
here: the self test of tests/float64_plan.py, and per collision sphere the field sampled at its centre
(tests/float64_cloud_plan.py's sampler, which takes centres of either precision unrounded) against
``check_margin + field_slack``.  ``dtype=np.float32`` runs the same statements in float32: the reference-against-reference
measurement that sets the band of the GPU edge-state test.  The seeded planner is ``float64_cloud_plan.solve`` through its
``start=`` argument.
"""
import numpy as np
import torch

import float64_cloud_plan as fcp
import float64_plan as fp
import float64_roadmap as fr
from float64_ik import limits32
from mpinets_amd import franka_tables as ft

DEFAULTS = fr.DEFAULTS
MAX_SPHERE_RADIUS = 0.08  # MPX_FRANKA_MAX_SPHERE_RADIUS


def slack_margin(check_margin, field_slack):
    """The right-hand side of the sphere rule, summed once in float32 as the host sums it."""
    return float(np.float32(check_margin) + np.float32(field_slack))


def margins(q, field_b, grid, point_radius=0.0, clearance=0.0, check_margin=1e-4, field_slack=0.0, check_self=True,
            with_base_link=False, want_samples=False):
    """q torch [N,7] (float64 or float32: the run's precision) against ONE environment's field float32 [nz,ny,nx] (None: no
    environment) -> env [N], self [N] (numpy float64): the smallest ``d - (check_margin + field_slack)`` over the spheres
    that are inside the grid and not saturated (+inf without one; the configuration is invalid when it is <= 0), and the
    smallest ``distance - (0.15 + radius + check_margin)`` of the self model (+inf without ``check_self``; invalid when < 0).
    ``want_samples``: also d [N,S] and live bool [N,S]."""
    dt = q.dtype
    x, _, t, radii, _ = fp.sphere_centres(q, with_base_link)
    N, S = x.shape[:2]
    env = torch.full((N,), float("inf"), dtype=dt)
    d = torch.full((N, S), float("inf"), dtype=dt)
    live = torch.zeros((N, S), dtype=torch.bool)
    if field_b is not None and N:
        D, _, inside, _ = fcp._sample_any(np.asarray(field_b, np.float32)[None], grid, x.reshape(1, N * S, 3), dt)
        D, inside = D.reshape(N, S), inside.reshape(N, S)
        live = inside & (D < float(np.float32(grid["trunc"])))
        d = ((D - point_radius) - radii) - clearance
        env = torch.where(live, d - slack_margin(check_margin, field_slack), torch.full_like(d, float("inf"))).amin(-1)
    own = torch.full((N,), float("inf"), dtype=dt)
    if check_self:
        for link, radius in ((7, 0.1), (9, 0.01), (12, 0.01), (13, 0.01)):
            c = t[:, link]
            dz = c[:, 2] - torch.clamp(c[:, 2], -0.3, 0.333)
            own = torch.minimum(own, torch.sqrt(c[:, 0] ** 2 + c[:, 1] ** 2 + dz ** 2) - (0.15 + radius + check_margin))
    out = env.double().numpy(), own.double().numpy()
    return out + (d.double().numpy(), live.numpy()) if want_samples else out


def field_validity(field_b, grid, dtype=np.float64, **rule):
    """-> ``is_valid(q [N,7] numpy) -> bool [N]`` of one problem, for ``float64_roadmap.search``."""
    tdt = torch.float32 if dtype == np.float32 else torch.float64

    def is_valid(q):
        q = torch.from_numpy(np.ascontiguousarray(np.nan_to_num(np.asarray(q)))).to(tdt)
        if q.shape[0] == 0:
            return np.zeros(0, bool)
        env, own = margins(q, field_b, grid, **rule)
        return (env > 0) & (own >= 0)
    return is_valid


def refused(grid, point_radius, field_slack, check_margin=DEFAULTS["check_margin"], clearance=0.0):
    """The host's truncation rule: obstacles between trunc and the threshold would be missed."""
    need = np.float32(MAX_SPHERE_RADIUS) + np.float32(point_radius) + np.float32(max(clearance, 0.0)) + \
        np.float32(slack_margin(check_margin, field_slack))
    return not float(np.float32(grid["trunc"])) > float(need)


def solve(q_start, q_goal, field=None, grid=None, point_radius=0.0, field_slack=0.0, limits=ft.JOINT_LIMITS_REAL, T=50,
          seed=0, env_offset=0, dtype=np.float64, with_base_link=False, **options):
    """-> traj [B,T,7] (NaN rows where status != 0), status [B], path [B,V] (-1 padded), hops [B], nodes float32 [B,V,7],
    edge_state uint8 [B,V,V], rounds [B]: like ``robot.franka_roadmap_cloud`` with ``return_graph``.  ``field`` float32
    [B,nz,ny,nx] on ``grid`` (a ``float64_cloud_field.make_grid`` dict), or None: no environment."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    V = opt["nodes"]
    qs, qg = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    B = qs.shape[0]
    lim = limits32(limits)
    nodes = fr.draw_nodes(qs, qg, limits, V, seed, env_offset)
    traj = np.full((B, T, 7), np.nan, dtype)
    status, hops, rounds = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    path = np.full((B, V), -1, np.int32)
    edge_state = np.zeros((B, V, V), np.uint8)
    for b in range(B):
        is_valid = field_validity(None if field is None else field[b], grid, dtype, point_radius=point_radius,
                                  clearance=opt["clearance"], check_margin=opt["check_margin"], field_slack=field_slack,
                                  check_self=opt["check_self"], with_base_link=with_base_link)
        ends = nodes[b, :2]
        inside = ((ends >= lim[:, 0]) & (ends <= lim[:, 1])).all(-1)  # (NaN fails)
        if not inside.all():
            status[b] = 2
            v = is_valid(nodes[b])
            v[:2] &= inside
            edge_state[b][np.arange(V), np.arange(V)] = np.where(v, fr.FREE, fr.BLOCKED)
            continue
        st, p, es, r = fr.search(nodes[b], is_valid, opt["resolution"], opt["connect_radius"], opt["max_rounds"], dtype)
        status[b], edge_state[b], rounds[b] = st, es, r
        if st == 0:
            hops[b] = len(p) - 1
            path[b, :len(p)] = p
            traj[b] = fr.seed_trajectory(nodes[b], p, T, opt["smooth_passes"], dtype)
    return traj, status, path, hops, nodes, edge_state, rounds


def graph_verdicts(nodes, edge_state, field_b, grid, band, resolution=DEFAULTS["resolution"], **rule):
    """The float64 verdict on the diagonal and on every TESTED edge of a given ``edge_state`` [V,V] over float32 ``nodes``
    [V,7] (a device's, or the restatement's own), from the float32 pieces of each edge -> (expected uint8 [V,V] on those
    entries, 0 elsewhere; in_band bool: some configuration that decides one of them has a sphere, or a self distance,
    within ``band`` of its threshold, so a float32 run may decide it the other way).  A NaN node counts as invalid."""
    nodes = np.asarray(nodes, np.float32)
    V = nodes.shape[0]
    W32 = fr.lengths(nodes, np.float32)
    want = np.zeros((V, V), np.uint8)
    edges = list(zip(*np.nonzero(np.triu(edge_state != fr.UNTESTED, 1))))
    configs = [fr.edge_configs(nodes[a], nodes[b], fr.pieces(W32[a, b], np.float32(resolution), np.float32), np.float32)
               for a, b in edges]
    q = np.concatenate([nodes] + configs, 0).astype(np.float64)
    env, own = margins(torch.from_numpy(np.nan_to_num(q)), field_b, grid, **rule)
    m = np.minimum(env, own)
    ok = (env > 0) & (own >= 0) & np.isfinite(q).all(-1)
    want[np.arange(V), np.arange(V)] = np.where(ok[:V], fr.FREE, fr.BLOCKED)
    in_band = bool((np.abs(m[:V]) <= band).any())
    at = V
    for (a, b), c in zip(edges, configs):
        me, oke = m[at:at + len(c)], ok[at:at + len(c)]
        at += len(c)
        want[a, b] = want[b, a] = fr.FREE if oke.all() else fr.BLOCKED
        if not (me < -band).any() and (np.abs(me) <= band).any():  # (a definite hit decides the edge whatever else is close)
            in_band = True
    return want, in_band


def solve_seeded(q_start, q_goal, seeds, cloud, counts=None, field=None, grid=None, point_radius=0.0,
                 limits=ft.JOINT_LIMITS_REAL, T=50, seed=0, env_offset=0, dtype=torch.float64, with_base_link=False, **options):
    """``mpx_franka_plan_cloud_seeded``: ``float64_cloud_plan.solve`` from the drawn candidates followed by ``seeds``
    [B,Ks,T,7] (interior clamped into the limits, endpoints replaced); a seed with a non-finite entry ends with NaN rows and
    bits 7 and cannot win.  -> what ``float64_cloud_plan.solve`` returns, over K + Ks candidates."""
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
    _, status, _, all_traj, all_bits = fcp.solve(qs, qg, cloud, counts, field, grid, point_radius, limits, T, seed, env_offset,
                                                 dtype, with_base_link, start=np.concatenate([drawn, sd], 1),
                                                 **dict(options, candidates=K + Ks))
    planned = status != 2
    kill = np.zeros((B, K + Ks), bool)
    kill[:, K:] = dead
    kill &= planned[:, None]
    all_bits[kill] = fp.BIT_ENV | fp.BIT_SELF | fp.BIT_JERK
    all_traj[kill] = np.nan
    traj, st, choice = fp.pick(all_traj, all_bits)
    traj[~planned], st[~planned], choice[~planned] = np.nan, 2, -1
    return traj, st, choice, all_traj, all_bits
