"""Restatement of ``mpx_gripper_roadmap_cloud`` on the CPU, in float64 by default, written from the contract in
include/mpinets_hip.h (not from csrc/gripper_roadmap_cloud.hip) and composed from what exists: everything but the environment
half of a pose's validity is tests/float64_gripper_roadmap.py's (the draws, ``place``, ``gripper_points``, ``lengths``,
``pieces``, ``edge_pose``, the lazy ``search``, ``resample``, ``dijkstra_cost``, the self test of ``margins``); the environment
half is stated here: per gripper sphere the field sampled at its centre (tests/float64_cloud_field.py's sampler on given nodal
values, through ``float64_cloud_plan._sample_any``, which takes centres of either precision unrounded) against
``check_margin + field_slack`` -- ``float64_roadmap_cloud.margins``' rule on the gripper's spheres.  ``dtype=np.float32`` runs
the same statements in float32: the reference-against-reference measurement behind ``CLOUD_BAND``
(tests/test_gripper_roadmap_cloud_host.py).

The scenarios of the GPU tests are built here, so that the CPU test that chooses their seed and the GPU tests use the same
problems: ``float64_gripper_roadmap.problems(64)`` against that module's wall and upright cylinder DRAWN AS CLOUDS (a lattice
of points on the obstacle's surface), and no cloud.
"""
import numpy as np
import torch

import float64_cloud_field as fcf
import float64_cloud_plan as fcp
import float64_gripper_roadmap as fg
from float64_roadmap import BLOCKED, FREE, UNTESTED
from float64_roadmap_cloud import MAX_SPHERE_RADIUS, slack_margin
from mpinets_amd import franka_tables as ft

DEFAULTS = fg.DEFAULTS
F32 = np.float32


# ---- validity ------------------------------------------------------------------------------------------------------------------
def margins(nodes, field_b, grid, point_radius=0.0, clearance=0.0, check_margin=1e-4, field_slack=0.0, check_self=True,
            finger=ft.FINGER_OPENING, dtype=np.float64, want_samples=False):
    """Poses (p, q) [N,7] against ONE environment's field float32 [nz,ny,nx] (None: no environment) -> env [N], own [N]
    (float64): the smallest ``d - (check_margin + field_slack)``, d = ((D - point_radius) - r_s) - clearance, over the gripper's
    spheres whose centre is inside the grid and where the field is not saturated (+inf without one; the pose is invalid when it
    is <= 0), and the self margin of ``float64_gripper_roadmap.margins`` (+inf without ``check_self``).  ``dtype`` is the
    arithmetic of the placement, the sample and d.  ``want_samples``: also d [N,G] and live bool [N,G]."""
    pts, radii, _, _ = fg.gripper_points(finger, dtype)
    nodes = np.asarray(nodes)
    N, G = len(nodes), len(radii)
    env, d, live = np.full(N, np.inf), np.full((N, G), np.inf), np.zeros((N, G), bool)
    if field_b is not None and N:
        tdt = torch.float32 if dtype == np.float32 else torch.float64
        x = torch.from_numpy(np.ascontiguousarray(fg.place(nodes, pts, dtype))).to(tdt).reshape(1, N * G, 3)
        D, _, inside, _ = fcp._sample_any(np.asarray(field_b, F32)[None], grid, x, tdt)
        D, inside = D.reshape(N, G).numpy(), inside.reshape(N, G).numpy()
        live = inside & (D < dtype(F32(grid["trunc"])))
        d = ((D - dtype(F32(point_radius))) - radii[None]) - dtype(F32(clearance))
        d = d.astype(np.float64)
        env = np.where(live, d - slack_margin(check_margin, field_slack), np.inf).min(-1)
    own = fg.margins(nodes, None, check_self=check_self, self_margin=check_margin, finger=finger, dtype=dtype)
    return (env, own, d, live) if want_samples else (env, own)


def validity(field_b, grid, dtype=np.float64, **rule):
    """-> ``is_valid(poses [N,7]) -> bool [N]`` of one problem, for ``float64_gripper_roadmap.search``."""
    def is_valid(poses):
        if len(poses) == 0:
            return np.zeros(0, bool)
        env, own = margins(poses, field_b, grid, dtype=dtype, **rule)
        return (env > 0) & (own > 0)
    return is_valid


def refused(grid, point_radius, field_slack, check_margin=DEFAULTS["check_margin"], clearance=0.0):
    """The host's truncation rule (the joint roadmap's, with MPX_FRANKA_MAX_SPHERE_RADIUS)."""
    need = F32(MAX_SPHERE_RADIUS) + F32(point_radius) + F32(max(clearance, 0.0)) + F32(slack_margin(check_margin, field_slack))
    return not float(F32(grid["trunc"])) > float(need)


def solve(start_pose, goal_pose, field=None, grid=None, point_radius=0.0, field_slack=0.0, W=8, bounds=None, seed=0,
          env_offset=0, dtype=np.float64, **options):
    """-> poses [B,W,4,4] (NaN rows where status != 0), status, path [B,V] (-1 padded), hops, nodes float32 [B,V,7],
    edge_state uint8 [B,V,V], rounds: like ``solvers.gripper_roadmap_cloud`` with ``return_graph``.  ``field`` float32
    [B,nz,ny,nx] or [nz,ny,nx] (one environment for every problem) on ``grid`` (a ``float64_cloud_field.make_grid`` dict), or
    None: no environment."""
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    opt = dict(DEFAULTS, **options)
    V = opt["nodes"]
    sp, gp = np.asarray(start_pose, F32), np.asarray(goal_pose, F32)
    B = sp.shape[0]
    bounds = fg.default_bounds(sp, gp) if bounds is None else np.broadcast_to(np.asarray(bounds, F32), (B, 2, 3))
    nodes, ok = fg.draw_nodes(sp, gp, bounds, V, seed, env_offset, opt["orient_spread"])
    ok[:, :2] &= fg.endpoints_ok(sp, gp, bounds)[:, None]
    poses = np.full((B, W, 4, 4), np.nan, dtype)
    status, hops, rounds = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    path = np.full((B, V), -1, np.int32)
    edge_state = np.zeros((B, V, V), np.uint8)
    for b in range(B):
        fb = None if field is None else (field if np.ndim(field) == 3 else field[b])
        is_valid = validity(fb, grid, dtype, point_radius=point_radius, clearance=opt["clearance"],
                            check_margin=opt["check_margin"], field_slack=field_slack, check_self=opt["check_self"])
        st, p, es, r = fg.search(nodes[b], ok[b], is_valid, opt["resolution"], opt["rot_weight"], opt["connect_radius"],
                                 opt["max_rounds"], dtype)
        status[b], edge_state[b], rounds[b] = st, es, r
        if st == 0:
            hops[b] = len(p) - 1
            path[b, :len(p)] = p
            poses[b] = fg.resample(nodes[b], p, W, opt["rot_weight"], dtype)
            poses[b, -1, :3] = gp[b, :3]
    return poses, status, path, hops, nodes, edge_state, rounds


def graph_verdicts(nodes, node_ok, edge_state, field_b, grid, band, resolution=DEFAULTS["resolution"],
                   rot_weight=DEFAULTS["rot_weight"], **rule):
    """``float64_gripper_roadmap.graph_verdicts`` with the field as the environment test, the band as
    ``float64_roadmap_cloud.graph_verdicts`` has it: the float64 verdict on the diagonal and on every TESTED edge of a given
    ``edge_state`` [V,V] over float32 ``nodes`` (a device's, or the restatement's own), the edge poses as float32 states them
    -> (expected uint8 [V,V] on those entries, 0 elsewhere; in_band: a pose that decides one of them has a sphere, or a self
    distance, within ``band`` of its threshold; the tested poses [N,7] float32)."""
    nodes = np.nan_to_num(np.asarray(nodes, F32))
    V = nodes.shape[0]
    W32 = fg.lengths(nodes, rot_weight, F32)
    want = np.zeros((V, V), np.uint8)
    edges = list(zip(*np.nonzero(np.triu(edge_state != UNTESTED, 1))))
    poses = [fg.edge_poses(nodes[a], nodes[b], fg.pieces(W32[a, b], F32(resolution), F32), F32) for a, b in edges]
    tested = np.concatenate([nodes] + poses, 0)
    env, own = margins(tested.astype(np.float64), field_b, grid, **rule)
    m = np.minimum(env, own)
    ok = np.asarray(node_ok, bool)
    want[np.arange(V), np.arange(V)] = np.where(ok & (m[:V] > 0), FREE, BLOCKED)
    in_band = bool((np.abs(m[:V][ok]) <= band).any())
    at = V
    for (a, b), q in zip(edges, poses):
        me, at = m[at:at + len(q)], at + len(q)
        want[a, b] = want[b, a] = FREE if (me > 0).all() else BLOCKED
        if not (me < -band).any() and (np.abs(me) <= band).any():  # (a definite hit decides the edge whatever else is close)
            in_band = True
    return want, in_band, tested


# ---- the scenarios of the GPU tests --------------------------------------------------------------------------------------------
ROADMAP_SEED = 5      # the Philox seed the GPU tests plan with: chosen on the CPU (tests/test_gripper_roadmap_cloud_host.py)
PITCH = 0.02          # [m] of the surface lattices
POINT_RADIUS = 0.015  # [m]: covers the largest gap to a lattice point, PITCH / sqrt(2) = 0.01414
KINDS = ("wall", "cylinder", "free")


def _steps(lo, hi, pitch):
    """lo .. hi in equal steps of at most ``pitch``, both ends included."""
    return np.linspace(lo, hi, int(np.ceil((hi - lo) / pitch - 1e-9)) + 1)


def surface_cloud(kind, pitch=PITCH):
    """``kind`` "wall" | "cylinder" -> float32 [N,3]: a lattice of points of pitch <= ``pitch`` on the surface of
    ``float64_gripper_roadmap``'s wall (the six faces of the box) or upright cylinder (rings round the side, and on each cap the
    square lattice inside the rim); None for "free"."""
    if kind == "free":
        return None
    c = np.float64(fg.WALL_CENTRE)
    if kind == "wall":
        half = np.float64(fg.WALL_DIMS) / 2
        ax = [_steps(-half[a], half[a], pitch) for a in range(3)]
        X, Y, Z = np.meshgrid(*ax, indexing="ij")
        on = (np.isin(X, ax[0][[0, -1]]) | np.isin(Y, ax[1][[0, -1]]) | np.isin(Z, ax[2][[0, -1]]))
        p = np.stack([X[on], Y[on], Z[on]], -1)
    else:
        assert kind == "cylinder"
        r, hh = fg.CYLINDER_RADIUS, fg.CYLINDER_HEIGHT / 2
        n = int(np.ceil(2 * np.pi * r / pitch))
        th = 2 * np.pi * np.arange(n) / n
        z = _steps(-hh, hh, pitch)
        side = np.stack([np.repeat(r * np.cos(th), len(z)), np.repeat(r * np.sin(th), len(z)), np.tile(z, n)], -1)
        a = _steps(-r, r, pitch)
        X, Y = np.meshgrid(a, a, indexing="ij")
        disc = X ** 2 + Y ** 2 < r ** 2
        caps = [np.stack([X[disc], Y[disc], np.full(int(disc.sum()), s * hh)], -1) for s in (-1.0, 1.0)]
        p = np.concatenate([side] + caps, 0)
    return (p + c).astype(F32)


def scenario_grid(point_radius=POINT_RADIUS):
    """The default grid (voxel 0.03) with ``plan_cloud_truncation(point_radius)``, as ``solvers.gripper_roadmap_cloud`` builds it."""
    return fcp.default_grid(fcp.truncation(point_radius))


def scenario_field(kind, grid=None):
    """-> (cloud float32 [N,3] or None, grid, field float32 [nz,ny,nx] or None): one environment, the same for every problem."""
    cloud = surface_cloud(kind)
    grid = scenario_grid() if grid is None else grid
    return cloud, grid, None if cloud is None else fcf.build_fast(cloud[None], None, grid)[0]
