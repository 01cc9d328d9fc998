"""Restatement of ``mpx_franka_follow_cloud`` on the CPU, in float64 by default, written from the contract in
include/mpinets_hip.h (not from csrc/follow_cloud.hip).  That contract is ``mpx_franka_follow``'s with two substitutions, and
so is this file: the step, the dense path, the retiming and the jerk / self / miss bits are tests/float64_follow.py's, run
unchanged; what ``float64_follow`` asks of ``float64_plan`` about the environment is answered here from the cloud instead --

* the obstacle term of one configuration is ``float64_cloud_plan.obstacle_gradient`` (the field sample with its gradient,
  ``d = ((D - point_radius) - r) - clearance``, active where ``D < trunc`` and ``d < epsilon``), with its fragile flag: ``d``
  within ``FRAGILE`` of 0 or epsilon, ``D`` within ``FRAGILE`` of trunc, a centre within the face rule of a cell face;
* the environment bit of a trajectory, and of a fresh rollout's start, is ``float64_cloud_plan``'s swept-sphere test against
  the cloud itself (``validity`` on the float32 waypoints, ``cloud_min_distance`` on the start) with
  ``reach = clearance + check_margin`` summed in float32.

The field is an ARRAY handed in (float32 [B,nz,ny,nx] and its grid dict): a GPU test hands over the field the device
built, a host test the one ``float64_cloud_field.build_fast`` builds.  ``dtype=torch.float32`` runs the same statements in
float32: the reference-against-reference measurement that sets the bars of the GPU tests.  The follower is a STAND-IN for
the reference's Geometric Fabrics expert, not Lula: this file restates the stand-in.

``problems`` builds the inputs the host and the GPU tests share: ``float64_follow.problems(32, seed)`` with the cube replaced
by ``float64_cloud_plan.cube_cloud`` at the same place.
"""
import contextlib
import functools

import numpy as np
import torch

import float64_cloud_field as fcf
import float64_cloud_plan as fcp
import float64_follow as ff
import float64_plan as fp
from mpinets_amd import franka_tables as ft

DEFAULTS = ff.DEFAULTS
FRAGILE = fcp.FRAGILE
BIT_ENV, BIT_MISS = fp.BIT_ENV, ff.BIT_MISS
POINT_RADIUS = fcp.WALL_POINT_RADIUS  # of the shared problems: the cube's lattice is 2 cm apart


class CloudScene(dict):
    """What stands where ``float64_follow`` takes its scene: ``field`` float32 [E,nz,ny,nx] (None: no obstacle term) on
    ``grid``, ``cloud`` float32 [E,N,3] (None: no environment test) with ``counts``, ``point_radius``, and ``env`` int [rows]: the
    environment of every row (default: row b reads environment b).  (A dict with the two keys ``float64_follow`` looks at to
    see whether there is an environment: there always is one to ask.)"""

    def __init__(self, field=None, grid=None, cloud=None, counts=None, point_radius=0.0, env=None):
        super().__init__(cub_dims=np.zeros((1, 1, 3), np.float32), cyl_radii=np.zeros((1, 0, 1), np.float32))
        self.field = None if field is None else np.ascontiguousarray(field, np.float32)
        self.grid, self.point_radius = grid, float(point_radius)
        self.cloud = None if cloud is None else np.asarray(cloud, np.float32)
        self.counts = None if counts is None else np.asarray(counts)
        self.env = None if env is None else np.asarray(env)

    def groups(self, rows):
        """-> [(environment, row indices)]; one group of all rows where row b reads environment b."""
        env = np.arange(rows) if self.env is None else self.env
        assert len(env) == rows
        return [(int(e), np.nonzero(env == e)[0]) for e in np.unique(env)]

    def row_cloud(self, rows):
        """-> cloud [rows,N,3] and counts [rows] (or None) by row."""
        env = np.arange(rows) if self.env is None else self.env
        return self.cloud[env], None if self.counts is None else self.counts[env]


class _CloudAnswers:
    """``float64_plan`` as ``float64_follow`` sees it while a ``CloudScene`` is the scene: the three questions about the
    environment are answered from the field and the cloud, everything else is ``float64_plan``'s."""

    def __getattr__(self, name):
        return getattr(fp, name)

    @staticmethod
    def obstacle_gradient(q, scene, K_T, epsilon=0.05, clearance=0.0, with_base_link=False, want_fragile=False):
        if not isinstance(scene, CloudScene):
            return fp.obstacle_gradient(q, scene, K_T, epsilon, clearance, with_base_link, want_fragile)
        assert K_T == 1
        g, fragile = torch.zeros_like(q), torch.zeros(q.shape[0], dtype=torch.bool)
        if scene.field is not None:
            if scene.env is None:  # one configuration per environment: one call
                g, fragile = fcp.obstacle_gradient(q, scene.field, scene.grid, 1, scene.point_radius, epsilon, clearance,
                                                   with_base_link, True)
            else:
                for e, idx in scene.groups(q.shape[0]):
                    g[idx], fragile[idx] = fcp.obstacle_gradient(q[idx], scene.field[e:e + 1], scene.grid, len(idx),
                                                                 scene.point_radius, epsilon, clearance, with_base_link, True)
        return (g, fragile) if want_fragile else g

    @staticmethod
    def config_bits(q, scene, K_R, reach, check_self, self_margin, with_base_link=False):
        if not isinstance(scene, CloudScene):
            return fp.config_bits(q, scene, K_R, reach, check_self, self_margin, with_base_link)
        assert K_R == 1
        bits = fp.config_bits(q, None, 1, reach, check_self, self_margin, with_base_link)
        if scene.cloud is not None:
            cloud, counts = scene.row_cloud(q.shape[0])
            gap = fcp.cloud_min_distance(q.double(), cloud, counts, 1, scene.point_radius, with_base_link) - reach
            bits = bits | (gap <= 0).any(-1).to(torch.int32) * BIT_ENV
        return bits


@contextlib.contextmanager
def _cloud_answers():
    saved, ff.fp = ff.fp, _CloudAnswers()
    try:
        yield
    finally:
        ff.fp = saved


def options(**given):
    return ff.options(**given)


def _reach(opt):
    return float(np.float32(opt["clearance"]) + np.float32(opt["check_margin"]))


def rollout(q_start, poses, scene, limits=ft.JOINT_LIMITS_REAL, v_init=None, progress=None, dtype=torch.float64,
            with_base_link=False, record_states=False, **given):
    """``float64_follow.rollout`` with ``scene`` a ``CloudScene``: the same dict.  (Its ``bad`` holds the cloud test of a fresh
    rollout's start, at ``reach`` = clearance + check_margin in float32.)"""
    assert isinstance(scene, CloudScene)
    with _cloud_answers():
        return ff.rollout(q_start, poses, scene, limits, v_init, progress, dtype, with_base_link, record_states, **given)


def verdict(traj, poses, scene, opt, with_base_link=False):
    """traj [B,T,7] -> int32 [B] bits and float64 [B]: ``float64_follow.verdict`` without a scene (jerk, self, miss, in
    float64) | BIT_ENV of ``float64_cloud_plan.validity`` on the float32 waypoints, and that test's smallest
    (distance - threshold)."""
    bits = ff.verdict(traj, poses, None, opt, with_base_link)
    gap = np.full(len(bits), np.inf)
    if scene.cloud is not None:
        cloud, counts = scene.row_cloud(len(bits))
        eb, g = fcp.validity(np.asarray(traj, np.float32)[:, None], cloud, counts, scene.point_radius, opt["substeps"],
                             opt["check_margin"], opt["clearance"], opt["max_jerk"], bool(opt["check_self"]), with_base_link)
        bits = bits | (eb[:, 0].numpy().astype(np.int32) & BIT_ENV)
        gap = g[:, 0].numpy()
    return bits.astype(np.int32), gap


def follow(q_start, poses, scene, limits=ft.JOINT_LIMITS_REAL, T=50, v_init=None, progress=None, dtype=torch.float64,
           with_base_link=False, record_states=False, **given):
    """Like ``robot.franka_follow_cloud(..., return_path=True, return_state=True)`` -> the ``rollout`` dict plus ``traj_any``,
    ``traj``, ``bits``, ``status`` and ``env_gap`` (how decided the environment bit is)."""
    out = rollout(q_start, poses, scene, limits, v_init, progress, dtype, with_base_link, record_states, **given)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    B = out["steps"].shape[0]
    ok = ~out["bad"]
    traj_any = np.full((B, T, 7), np.nan, npdt)
    bits, gap = np.full(B, 15, np.int32), np.full(B, np.inf)
    if ok.any():
        traj_any[ok] = ff.retime(out["path"][ok], out["arc"][ok], out["steps"][ok], T, npdt)
        env = np.arange(B) if scene.env is None else scene.env
        sub = CloudScene(scene.field, scene.grid, scene.cloud, scene.counts, scene.point_radius, env[ok])
        bits[ok], gap[ok] = verdict(traj_any[ok], np.asarray(poses, np.float32)[ok], sub, out["options"], with_base_link)
    traj = traj_any.copy()
    traj[bits != 0] = np.nan
    out.update(traj_any=traj_any, traj=traj, bits=bits, env_gap=gap,
               status=np.where(out["bad"], 2, (bits != 0).astype(np.int32)).astype(np.int32))
    return out


# ---- the inputs the host and the GPU tests share --------------------------------------------------------------------------
# ``problems``: ``float64_follow.problems(32, PROBLEM_SEED)`` with its cube drawn as a cloud.  The seed was chosen on the CPU,
# from the float64 restatement alone, so that the conditions of tests/test_follow_cloud_host.py hold: at most 25 % of the rows
# have a fragile step, and strictly fewer rows carry the environment bit with the default ``repel`` than with ``repel = 0``.
# The first condition is rare: a sphere's d passes within FRAGILE = 1e-5 m of epsilon on about one row in three (d moves
# about a millimetre a step and some twenty spheres enter or leave the band on a row), the stop test is approached at 0.3 mm
# a step, and about half the rows of a typical seed have a fragile step (seeds 15 .. 159: 11 to 22 of 32 rows).  Seeds 160 ..
# 1450 were scanned, each rollout abandoned at its ninth fragile row; 1059 and 1279 have 8 such rows, 1416 has 7.
PROBLEM_SEED = 1416


@functools.lru_cache(maxsize=None)
def problems(B=32, seed=PROBLEM_SEED):
    """-> q_start, q_goal float32 [B,7], guide float32 [B,8,4,4], cloud float32 [B,N,3] (the surface lattice of the cube of
    ``float64_follow.problems`` at the same place, 2 cm apart) and the cube centres [B,3]."""
    qs, qg, guide, scn = ff.problems(B, seed)
    centre = scn["cuboid_centers"][:, 0]
    return qs, qg, guide, fcp.cube_cloud(centre, ff.CUBOID_SIDE), centre


def default_field(cloud, counts=None, point_radius=POINT_RADIUS, **given):
    """The field ``robot.franka_follow_cloud`` builds with ``field=None``, on the CPU -> float32 [B,nz,ny,nx] and the grid."""
    opt = ff.options(**given)
    grid = fcp.default_grid(fcp.truncation(point_radius, opt["clearance"], opt["epsilon"], fcp.VOXEL))
    return fcf.build_fast(cloud, counts, grid), grid
