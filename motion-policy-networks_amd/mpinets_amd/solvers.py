"""The device solvers for the Franka: inverse kinematics, trajectory optimisation, the roadmap and the shortcutting of its
path, the gripper's SE(3) roadmap and the path follower, against primitives or a point cloud (csrc/ik.hip, plan.hip,
roadmap.hip, gripper_roadmap.hip, gripper_shortcut.hip, follow.hip, cloud_field.hip, roadmap_cloud.hip, follow_cloud.hip;
shortcut_kernel.inc).  Each wrapper is its entry's argument list: the inputs
(``_inputs``), the blocks of ``_operands`` (sphere table and primitives, or cloud; options / seed / env_offset) and the
outputs, in the header's order.  ``robot`` re-exports every name here."""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import franka_tables as ft
from ._operands import (cloud_args, limits_operand, merge_options, options_tail, scratch_for, sphere_primitive_args,
                        sphere_table)
from ._operands import sphere_table as _ik_sphere_table  # noqa: F401  (the name tests and tools reach it by)
from .field import DEFAULT_VOXEL, CloudField

IK_SEEDS = 64  # MPX_IK_SEEDS: starts per problem, one per lane
IK_SOLVED, IK_IN_COLLISION, IK_NOT_CONVERGED = 0, 1, 2  # status values of ``franka_ik``
IK_BIT_CONVERGED, IK_BIT_ENV_HIT, IK_BIT_SELF_HIT = 1, 2, 4  # per-start bits of ``return_all``
IK_DEFAULTS = dict(iterations=64, damping=0.05, step_clip=0.5, pos_tol=1e-3, rot_tol=float(np.radians(0.5)),
                   clearance=0.0)
_IK_DEFAULTS_BY_SELF = {s: dict(IK_DEFAULTS, check_self=s) for s in (False, True)}  # (``check_self``: each entry's own default)

PLAN_SOLVED, PLAN_NO_VALID_CANDIDATE, PLAN_BAD_ENDPOINT = 0, 1, 2  # status values of ``franka_plan``
PLAN_BIT_ENV_HIT, PLAN_BIT_SELF_HIT, PLAN_BIT_JERK = 1, 2, 4  # per-candidate bits of ``return_all``
# MPX_PLAN_DEFAULT_* (include/mpinets_hip.h; profiles/plan_timing.md holds the table behind iterations / step / smooth_weight)
PLAN_DEFAULTS = dict(candidates=8, iterations=20, step=2e-4, smooth_weight=20.0, epsilon=0.05, spread=0.5, substeps=4,
                     check_margin=1e-4, clearance=0.0, max_jerk=0.15, check_self=True)

ROADMAP_FOUND, ROADMAP_NO_PATH, ROADMAP_BAD_ENDPOINT = 0, 1, 2  # status values of ``franka_roadmap``
ROADMAP_EDGE_UNTESTED, ROADMAP_EDGE_FREE, ROADMAP_EDGE_BLOCKED = 0, 1, 2  # ``edge_state`` of ``return_graph``
# MPX_ROADMAP_DEFAULT_* (include/mpinets_hip.h; profiles/roadmap_timing.md holds the runs behind them)
ROADMAP_DEFAULTS = dict(nodes=64, resolution=0.05, connect_radius=float("inf"), max_rounds=64, smooth_passes=8,
                        check_margin=1e-4, clearance=0.0, check_self=True)

SHORTCUT_RETURNED, SHORTCUT_BAD_ROW = 0, 2  # status values of ``franka_shortcut`` (there is no 1: the input is the fallback)
# MPX_SHORTCUT_DEFAULT_* and the roadmap's values (include/mpinets_hip.h; profiles/shortcut_timing.md holds the runs behind them)
SHORTCUT_DEFAULTS = dict(points=64, passes=2, fanout=4, resolution=0.05, smooth_passes=8, check_margin=1e-4, clearance=0.0,
                         check_self=True)

# MPX_GRIPPER_ROADMAP_DEFAULT_* (include/mpinets_hip.h; profiles/gripper_roadmap_timing.md holds the runs behind them); the
# status and ``edge_state`` values are the roadmap's (``ROADMAP_FOUND`` ...)
GRIPPER_ROADMAP_DEFAULTS = dict(nodes=64, resolution=0.01, rot_weight=0.12, orient_spread=0.5, connect_radius=float("inf"),
                                max_rounds=256, check_margin=1e-4, clearance=0.0, check_self=True)
# MPX_SHORTCUT_DEFAULT_* and the gripper roadmap's values (include/mpinets_hip.h; profiles/gripper_shortcut_timing.md); the
# status values are the shortcut's (``SHORTCUT_RETURNED``, ``SHORTCUT_BAD_ROW``)
GRIPPER_SHORTCUT_DEFAULTS = dict(points=64, passes=2, fanout=4, resolution=0.01, rot_weight=0.12, check_margin=1e-4,
                                 clearance=0.0, check_self=True)
GRIPPER_ROADMAP_BOUNDS_PAD = 0.3  # [m] ``bounds=None``: the box hull of the two positions, grown by this much per side

TASK_PADDING, TASK_SURFACE, TASK_VOLUME = 0, 1, 2  # ``support_kind`` of ``task_candidates``
# MPX_TASK_DEFAULT_DRAWS and the NULL-options values (include/mpinets_hip.h); ``role`` is the wrapper's own argument
TASK_CANDIDATES_DEFAULTS = dict(draws=100, clearance=0.0, test_self=True, self_margin=0.0, role=0)

FOLLOW_VALID, FOLLOW_INVALID, FOLLOW_BAD_INPUT = 0, 1, 2  # status values of ``franka_follow``
FOLLOW_BIT_MISS = 8  # MPX_FOLLOW_BIT_MISS, beside PLAN_BIT_ENV_HIT / PLAN_BIT_SELF_HIT / PLAN_BIT_JERK in ``bits``
FOLLOW_MAX_STEPS = 4096  # MPX_FOLLOW_MAX_STEPS
# MPX_FOLLOW_DEFAULT_* (include/mpinets_hip.h; profiles/follow_timing.md holds the runs behind them).  ``lambda_`` is the C
# struct's ``lambda`` (``damping`` is the follower's viscous term, not the solve's)
FOLLOW_DEFAULTS = dict(dt=0.005, max_steps=1024, attract=144.0, damping=24.0, lambda_=0.05, step_clip=0.5, repel=40.0,
                       epsilon=0.05, clearance=0.0, limit_gain=50.0, limit_band=0.1, speed_limit=1.6999, switch_radius=0.15,
                       switch_steps=100, final_radius=0.005, final_steps=800, substeps=4, check_margin=1e-4, max_jerk=0.15,
                       check_self=True, miss_tol=0.05)

# without ``return_path``, ``franka_follow`` runs a large batch in slabs of problems whose dense path and arc stay below this
FOLLOW_PATH_BYTES = 512 << 20

PLAN_CLOUD_SCRATCH_BYTES = 256 << 20  # ``franka_plan_cloud`` runs a large batch in slabs of problems whose scratch stays below this


def _ik_options(who: str, options: dict, check_self: bool) -> _lib.IkOptions:
    """Keyword options of an IK entry over ``IK_DEFAULTS`` and its ``check_self`` default; ``lambda`` is ``damping``'s C name."""
    if "lambda" in options:
        options["damping"] = options.pop("lambda")
    return merge_options(who, _lib.IkOptions, _IK_DEFAULTS_BY_SELF[bool(check_self)], options)[0]


def _plan_options(who: str, options: dict):
    """Keyword options of a planning entry over ``PLAN_DEFAULTS`` -> the ``_lib.PlanOptions`` and the merged dict."""
    return merge_options(who, _lib.PlanOptions, PLAN_DEFAULTS, options)


def _roadmap_options(who: str, options: dict):
    """Keyword options of the roadmap over ``ROADMAP_DEFAULTS`` -> the ``_lib.RoadmapOptions`` and the merged dict."""
    return merge_options(who, _lib.RoadmapOptions, ROADMAP_DEFAULTS, options)


def _shortcut_options(who: str, options: dict):
    """Keyword options of the shortcut over ``SHORTCUT_DEFAULTS`` -> the ``_lib.ShortcutOptions`` and the merged dict."""
    return merge_options(who, _lib.ShortcutOptions, SHORTCUT_DEFAULTS, options)


def _gripper_roadmap_options(who: str, options: dict):
    """Keyword options of the gripper roadmap over ``GRIPPER_ROADMAP_DEFAULTS`` -> the ``_lib.GripperRoadmapOptions`` and the
    merged dict."""
    return merge_options(who, _lib.GripperRoadmapOptions, GRIPPER_ROADMAP_DEFAULTS, options)


def _gripper_shortcut_options(who: str, options: dict):
    """Keyword options of the gripper's shortcut over ``GRIPPER_SHORTCUT_DEFAULTS`` -> the ``_lib.GripperShortcutOptions`` and
    the merged dict."""
    return merge_options(who, _lib.GripperShortcutOptions, GRIPPER_SHORTCUT_DEFAULTS, options)


def _follow_options(who: str, options: dict):
    """Keyword options of the follower over ``FOLLOW_DEFAULTS`` -> the ``_lib.FollowOptions`` and the merged dict; ``lambda``
    is accepted for ``lambda_``."""
    if "lambda" in options:
        options["lambda_"] = options.pop("lambda")
    return merge_options(who, _lib.FollowOptions, FOLLOW_DEFAULTS, options)


def _inputs(first: torch.Tensor, rows: tuple, second: Optional[torch.Tensor], limits, *others):
    """What every solver starts from: ``first`` ``[B, *rows]`` (target poses, or ``q_start``), ``second`` ``[B,7]`` (``q_init``
    or None, or ``q_goal``), ``limits`` and the other tensors of the call, all on the current GPU -> B, the device, the two
    as contiguous float32 and the limits operand."""
    _lib.require_cuda(first, second, *others)
    assert first.ndim == 1 + len(rows) and first.shape[1:] == rows
    B, dev = first.size(0), first.device
    assert second is None or second.shape == (B, 7)
    return B, dev, _lib.f32c(first), None if second is None else _lib.f32c(second), limits_operand(limits, dev)


# The outputs of an entry, in its argument order: the call passes ``_ptrs`` of them, the caller gets them all or the first few.


def _ik_outputs(B: int, dev: torch.device, return_all: bool):  # -> q, status, all_q, all_status (None without return_all)
    return (torch.empty((B, 7), dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty((B, IK_SEEDS, 7), dtype=torch.float32, device=dev) if return_all else None,
            torch.empty((B, IK_SEEDS), dtype=torch.int32, device=dev) if return_all else None)


def _plan_outputs(B: int, K: int, T: int, dev: torch.device, return_all: bool):  # -> traj, status, choice, all_traj, all_status
    return (torch.empty((B, T, 7), dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev) if return_all else None,
            torch.empty((B, K, T, 7), dtype=torch.float32, device=dev) if return_all else None,
            torch.empty((B, K), dtype=torch.int32, device=dev) if return_all else None)


def _roadmap_outputs(B: int, rows0: tuple, V: int, dev: torch.device, return_graph: bool):
    """-> traj [B,T,7] (``rows0`` = (T, 7)) or poses [B,W,4,4] (``rows0`` = (W, 4, 4)), status, path, hops, nodes, edge_state, rounds"""
    return (torch.empty((B,) + rows0, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty((B, V), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty((B, V, 7), dtype=torch.float32, device=dev) if return_graph else None,
            torch.empty((B, V, V), dtype=torch.uint8, device=dev) if return_graph else None,
            torch.empty(B, dtype=torch.int32, device=dev) if return_graph else None)


def _shortcut_call(who: str, points: torch.Tensor, count: torch.Tensor, T: int, return_trace: bool, options: dict, others=(),
                   W: Optional[int] = None, goal_pose: Optional[torch.Tensor] = None):
    """What the shortcut wrappers start from and end with: the polylines ``[B,Pin,7]`` and ``count`` ``[B]`` on the current
    GPU, the options, the outputs in the entry's order -> ``run(entry, *environment)`` that calls ``entry`` and returns
    ``traj, status, points_out, count_out, length`` (with ``return_trace`` also ``chords, configs``), and the merged options.
    With ``W`` the gripper's form: ``mpx_gripper_shortcut_options``, ``poses`` [B,W,4,4] in the place of ``traj``, and ``W``
    and ``goal_pose`` ([B,4,4] or None) where the joint-space entries take ``T``."""
    _lib.require_cuda(points, count, goal_pose, *others)
    assert points.ndim == 3 and points.size(2) == 7 and count.shape == (points.size(0),)
    B, Pin, dev = points.size(0), points.size(1), points.device
    pts, cn = _lib.f32c(points), _lib.i32c(count)
    copt, o = (_shortcut_options if W is None else _gripper_shortcut_options)(who, options)
    P = max(int(o["points"]), 0)
    i32 = dict(dtype=torch.int32, device=dev)
    if W is None:
        rows0, head = (T, 7), (int(T),)
    else:
        assert goal_pose is None or tuple(goal_pose.shape) == (B, 4, 4)
        gp = None if goal_pose is None else _lib.f32c(goal_pose)
        rows0, head = (max(int(W), 0), 4, 4), (int(W), _lib.ptr(gp))
    out = (torch.empty((B,) + rows0, dtype=torch.float32, device=dev), torch.empty(B, **i32),
           torch.empty((B, P, 7), dtype=torch.float32, device=dev), torch.empty(B, **i32),
           torch.empty((B, 2), dtype=torch.float32, device=dev), torch.empty(B, **i32) if return_trace else None,
           torch.empty(B, **i32) if return_trace else None)

    def run(entry: str, finger: float, *environment):
        _lib.call(entry, pts.data_ptr(), cn.data_ptr(), B, Pin, *head, float(finger), *environment, ctypes.byref(copt),
                  *_ptrs(out))
        return out if return_trace else out[:5]

    return run, o, B, dev


def _ptrs(tensors):
    return [None if t is None else t.data_ptr() for t in tensors]


def franka_ik(target_poses: torch.Tensor, cuboids=None, cylinders=None, q_init: Optional[torch.Tensor] = None,
              limits=ft.JOINT_LIMITS_REAL, seed: int = 0, env_offset: int = 0, with_base_link: bool = False,
              return_all: bool = False, finger: float = ft.FINGER_OPENING, **options):
    """Batched collision-free inverse kinematics on the GPU (csrc/ik.hip: damped least squares, 64 starts per pose).

    :param target_poses: [B,4,4] right_gripper poses
    :param cuboids, cylinders: ``geometry.TorchCuboids`` / ``TorchCylinders`` (batch B) or None, as for
        ``FrankaCollisionSampler.check``
    :param limits: [7,2]; cast to float32 toward the inside of the interval, so every returned joint satisfies them as given
    :param q_init: [B,7] first start of every problem (default: the neutral pose); the other 63 are uniform in ``limits``,
        drawn from Philox keyed by (``seed``, ``env_offset`` + row, start)
    :param options: ``iterations`` (64), ``damping`` (0.05; the C struct's ``lambda``), ``step_clip`` (0.5 rad), ``pos_tol``
        (1e-3 m), ``rot_tol`` (radians; 0.5 degrees), ``clearance`` (0 m), ``check_self`` (default: on when primitives are
        passed, off in free space)
    :returns: ``q`` [B,7] (NaN rows where ``status`` != 0) and ``status`` int32 [B]: 0 solved, 1 every converged start
        collides, 2 nothing converged; with ``return_all`` also ``all_q`` [B,64,7] and ``all_status`` int32 [B,64] (bit 0
        converged, bit 1 environment hit, bit 2 self hit)."""
    B, dev, tp, qi, lim = _inputs(target_poses, (4, 4), q_init, limits)
    copt = _ik_options("franka_ik", options, check_self=cuboids is not None or cylinders is not None)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    out = _ik_outputs(B, dev, return_all)
    _lib.call("mpx_franka_ik", tp.data_ptr(), B, float(finger), lim.data_ptr(), _lib.ptr(qi), *prims,
              *options_tail(copt, seed, env_offset), *_ptrs(out))
    return out if return_all else out[:2]


def franka_ik_cloud(target_poses: torch.Tensor, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None,
                    point_radius: float = 0.0, q_init: Optional[torch.Tensor] = None, limits=ft.JOINT_LIMITS_REAL,
                    seed: int = 0, env_offset: int = 0, with_base_link: bool = False, return_all: bool = False,
                    finger: float = ft.FINGER_OPENING, **options):
    """``franka_ik`` against one POINT CLOUD per environment instead of primitives (``mpx_franka_ik_cloud``): the same 64
    starts and iterations, and the result is the lowest start that converges, is free of the cloud by
    ``FrankaCollisionSampler.check_cloud``'s test (``point_radius``, ``clearance`` from the options) and, with
    ``check_self`` (default: on), of the robot itself.

    :param cloud: [B,N,3] or [B,N,4] float32 on the GPU, any view whose last stride is 1 (``xyz[:, 2048:6144, :3]`` of the
        slab is read in place); ``counts`` optional int [B] as for ``check_cloud``
    :param point_radius: radius given to every point (>= 0)
    :returns: what ``franka_ik`` returns; bit 1 of ``all_status`` is the cloud verdict of a converged start (0 on the
        others, which are not tested)."""
    copt = _ik_options("franka_ik_cloud", options, check_self=True)
    B, dev, tp, qi, lim = _inputs(target_poses, (4, 4), q_init, limits, cloud, counts)
    points, held = cloud_args("franka_ik_cloud", cloud, counts, B, point_radius, null_without_points=True)
    sc, sr, sl = sphere_table(dev, with_base_link)
    out = _ik_outputs(B, dev, return_all)
    nbytes = int(_lib.load().mpx_franka_ik_cloud_scratch(B))
    buf = scratch_for(dev, nbytes)
    _lib.call("mpx_franka_ik_cloud", tp.data_ptr(), B, float(finger), lim.data_ptr(), _lib.ptr(qi), sc.data_ptr(),
              sr.data_ptr(), sl.data_ptr(), int(sc.size(0)), *points, *options_tail(copt, seed, env_offset), *_ptrs(out),
              buf.data_ptr(), nbytes)
    return out if return_all else out[:2]


def franka_plan(q_start: torch.Tensor, q_goal: torch.Tensor, cuboids=None, cylinders=None, T: int = 50, seed: int = 0,
                env_offset: int = 0, return_all: bool = False, limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False,
                finger: float = ft.FINGER_OPENING, seeds: Optional[torch.Tensor] = None, **options):
    """Batched collision-free trajectories from ``q_start`` to ``q_goal`` on the GPU (csrc/plan.hip): covariant gradient
    descent on ``T`` waypoints from ``candidates`` starting trajectories per problem (the straight line, and the line bent
    by Philox draws keyed by (``seed``, ``env_offset`` + row, candidate)), then a validity sweep of every candidate; the
    result is the lowest valid one.  A LOCAL optimiser, not the reference's AIT*: it can fail where a sampling planner
    succeeds, and "valid" means free by this engine's sphere model (``FrankaCollisionSampler`` / ``BatchedEvaluator``).

    :param q_start, q_goal: [B,7], inside ``limits`` and collision free (e.g. from ``franka_ik``)
    :param cuboids, cylinders: ``geometry.TorchCuboids`` / ``TorchCylinders`` (batch B) or None, as for ``franka_ik``
    :param limits: [7,2]; cast to float32 toward the inside of the interval, as ``franka_ik`` does
    :param seeds: None (``mpx_franka_plan``), or [B,Ks,T,7] caller-supplied starting trajectories (``mpx_franka_plan_seeded``,
        e.g. ``franka_roadmap``'s): candidates ``candidates`` .. ``candidates`` + Ks - 1, behind the drawn ones, which stay
        bit-equal; interior waypoints are clamped into ``limits``, the endpoints replaced, a seed with a non-finite entry
        is not optimised (NaN rows, bits 7); ``candidates`` + Ks <= 16.  ``all_traj`` / ``all_status`` then have K + Ks rows.
    :param options: the fields of ``mpx_plan_options``, see ``PLAN_DEFAULTS``
    :returns: ``traj`` [B,T,7] (NaN rows where ``status`` != 0; waypoints 0 and T-1 are bit-equal to the inputs) and
        ``status`` int32 [B]: 0 solved, 1 no valid candidate, 2 an endpoint is non-finite, outside the limits or in
        collision.  "In collision" is the validity sweep's own test, which adds ``check_margin`` (1e-4 m) to the sphere
        radii AND to the self-collision distances: an endpoint that ``FrankaCollisionSampler.check`` or
        ``mpx_trajectory_metrics`` accepts by less than that margin is refused with status 2.  With ``return_all`` also ``choice`` int32 [B], ``all_traj`` [B,K,T,7] and ``all_status`` int32 [B,K] (bit 0
        environment hit, bit 1 self hit, bit 2 jerk)."""
    B, dev, qs, qg, lim = _inputs(q_start, (7,), q_goal, limits)
    copt, o = _plan_options("franka_plan", options)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    entry, seeded, Ks = "mpx_franka_plan", (), 0
    if seeds is not None:
        _lib.require_cuda(seeds)
        assert seeds.ndim == 4 and seeds.size(0) == B and tuple(seeds.shape[2:]) == (int(T), 7)
        sd, Ks = _lib.f32c(seeds), seeds.size(1)
        entry, seeded = "mpx_franka_plan_seeded", (sd.data_ptr() if Ks else None, Ks)
    out = _plan_outputs(B, max(int(o["candidates"]), 0) + Ks, T, dev, return_all)
    _lib.call(entry, qs.data_ptr(), _lib.ptr(qg), B, int(T), float(finger), lim.data_ptr(), *prims,
              *options_tail(copt, seed, env_offset), *seeded, *_ptrs(out))
    return out if return_all else out[:2]


def franka_roadmap(q_start: torch.Tensor, q_goal: torch.Tensor, cuboids=None, cylinders=None, T: int = 50, seed: int = 0,
                   env_offset: int = 0, return_graph: bool = False, limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False,
                   finger: float = ft.FINGER_OPENING, **options):
    """A lazy probabilistic roadmap per problem on the GPU (csrc/roadmap.hip): ``nodes`` configurations (start, goal and
    Philox draws inside ``limits`` keyed by (``seed``, ``env_offset`` + row, node)) judged by ``franka_plan``'s validity test,
    the shortest start-goal path over the edges not known to be blocked, its untested edges tested every ``resolution`` rad,
    searched again until a path survives.  The path, resampled to ``T`` waypoints and rounded by ``smooth_passes`` passes
    of (1/4, 1/2, 1/4), is a seed for ``franka_plan(seeds=...)``: it is collision free as a polyline, not yet smooth enough.

    :param q_start, q_goal, cuboids, cylinders, limits: as for ``franka_plan``
    :param options: the fields of ``mpx_roadmap_options``, see ``ROADMAP_DEFAULTS``
    :returns: ``traj`` [B,T,7] (NaN rows where ``status`` != 0; a one-edge path is ``franka_plan``'s straight line bit for
        bit), ``status`` int32 [B] (0 path found, 1 none, 2 an endpoint is non-finite, outside the limits or in collision),
        ``path`` int32 [B,V] (node indices from 0 = start to 1 = goal, then -1) and ``hops`` int32 [B]; with
        ``return_graph`` also ``nodes`` [B,V,7], ``edge_state`` uint8 [B,V,V] (0 untested, 1 free, 2 blocked; the diagonal
        1 for a valid node, 2 for an invalid one) and ``rounds`` int32 [B]."""
    B, dev, qs, qg, lim = _inputs(q_start, (7,), q_goal, limits)
    copt, o = _roadmap_options("franka_roadmap", options)
    V = max(int(o["nodes"]), 0)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    out = _roadmap_outputs(B, (T, 7), V, dev, return_graph)
    _lib.call("mpx_franka_roadmap", qs.data_ptr(), _lib.ptr(qg), B, int(T), float(finger), lim.data_ptr(), *prims,
              *options_tail(copt, seed, env_offset), *_ptrs(out))
    return out if return_graph else out[:4]


def franka_shortcut(polylines: torch.Tensor, count: torch.Tensor, cuboids=None, cylinders=None, T: int = 50,
                    return_trace: bool = False, with_base_link: bool = False, finger: float = ft.FINGER_OPENING, **options):
    """Shortcut one joint-space polyline per problem on the GPU (csrc/shortcut_kernel.inc in roadmap.hip): ``passes``
    alternating forward / backward passes, each densifying the polyline to at most ``points`` points and walking it
    greedily -- from the current anchor to the furthest point whose chord is free by ``franka_roadmap``'s edge test, found
    by a ``fanout``-ary search.  Where the reference asks its planner for ``shortcut=True``; a stand-in by this engine's
    sphere model, not OMPL's simplifier.  Deterministic: no seed.

    :param polylines: [B,Pin,7] float32 (the C entry's ``points``; ``points`` here is the option P), ``count`` int [B]: the
        polyline of a row is its first ``count`` vertices (2 <= count <= Pin <= 256), e.g. ``nodes[path]`` of
        ``franka_roadmap(..., return_graph=True)``.  The caller vouches for its segments: they are not tested
    :param cuboids, cylinders: as for ``franka_roadmap``
    :param options: the fields of ``mpx_shortcut_options``, see ``SHORTCUT_DEFAULTS``
    :returns: ``traj`` [B,T,7] (``franka_roadmap``'s resampling and corner filter over the returned polyline; a one-edge
        result is ``franka_plan``'s line bit for bit; NaN rows where ``status`` != 0), ``status`` int32 [B] (0 a polyline is
        returned, 2 a bad row: count < 2, count > Pin or a non-finite vertex), ``points_out`` [B,P,7] (NaN rows beyond
        ``count_out``), ``count_out`` int32 [B] and ``length`` [B,2] (before, after); with ``return_trace`` also ``chords``
        and ``configs`` int32 [B], the chords and interior configurations tested."""
    run, o, B, dev = _shortcut_call("franka_shortcut", polylines, count, T, return_trace, options)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    return run("mpx_franka_shortcut", finger, *prims)


def _path_vertices(nodes: torch.Tensor, path: torch.Tensor, hops: torch.Tensor):
    """``nodes[path]`` of a roadmap's graph -> the polylines [B,V,7] (rows behind a path: node 0) and their vertex counts
    (0 where the roadmap found nothing: a bad row for the shortcut, whose NaN ``traj`` is the planner's NaN seed)."""
    idx = path.clamp(0, nodes.size(1) - 1).long()[:, :, None].expand(-1, -1, 7)
    return torch.gather(nodes, 1, idx), torch.where(hops > 0, hops + 1, torch.zeros_like(hops))


def _shortcut_arg(shortcut) -> Optional[dict]:
    """``shortcut`` of the global planners -> None (off) or the options dict."""
    if shortcut is None or shortcut is False:
        return None
    return {} if shortcut is True else dict(shortcut)


def franka_plan_global(q_start: torch.Tensor, q_goal: torch.Tensor, cuboids=None, cylinders=None, T: int = 50, seed: int = 0,
                       env_offset: int = 0, return_all: bool = False, limits=ft.JOINT_LIMITS_REAL,
                       with_base_link: bool = False, finger: float = ft.FINGER_OPENING, roadmap: Optional[dict] = None,
                       shortcut=None, **options):
    """``franka_roadmap``, then ``franka_plan`` with the roadmap's trajectory as one more candidate behind the drawn ones:
    a row ``franka_plan`` solves comes back identical, a row whose straight line is blocked gets a start that already
    goes round the obstacle.  Rows where the roadmap found nothing pass a NaN seed (bits 7).

    :param roadmap: options of ``franka_roadmap`` (``ROADMAP_DEFAULTS``); ``check_margin``, ``clearance`` and ``check_self``
        default to the planner's values in ``options``
    :param shortcut: None (the call above, unchanged), or True / a dict of ``franka_shortcut``'s options
        (``SHORTCUT_DEFAULTS``; the three shared ones and ``resolution`` / ``smooth_passes`` default to the roadmap's): the
        roadmap's path is shortcut and TWO seeds are passed, the shortcut trajectory (candidate ``candidates``) in front of
        the roadmap's (``candidates`` + 1).  The lowest valid candidate wins, so no row solved without ``shortcut`` is lost
    :param options: the fields of ``mpx_plan_options``; ``candidates`` (8) + 1 (with ``shortcut``: + 2) <= 16
    :returns: what ``franka_plan`` returns (``all_traj`` / ``all_status`` with the seeds last), then the roadmap's
        ``status`` int32 [B]."""
    _, o = _plan_options("franka_plan_global", options)
    shared = {k: o[k] for k in ("check_margin", "clearance", "check_self")}
    ropt = dict(shared, **(roadmap or {}))
    sopt = _shortcut_arg(shortcut)
    seed_traj, rm_status, path, hops, *graph = franka_roadmap(q_start, q_goal, cuboids, cylinders, T, seed, env_offset,
                                                              sopt is not None, limits, with_base_link, finger, **ropt)
    seeds = seed_traj[:, None]
    if sopt is not None:
        pts, cnt = _path_vertices(graph[0], path, hops)
        inherited = {k: ropt[k] for k in ("check_margin", "clearance", "check_self", "resolution", "smooth_passes") if k in ropt}
        short = franka_shortcut(pts, cnt, cuboids, cylinders, T, False, with_base_link, finger,
                                **{"points": max(SHORTCUT_DEFAULTS["points"], pts.size(1)), **inherited, **sopt})[0]
        seeds = torch.stack((short, seed_traj), 1)
    out = franka_plan(q_start, q_goal, cuboids, cylinders, T, seed, env_offset, return_all, limits, with_base_link, finger,
                      seeds=seeds, **options)
    return tuple(out) + (rm_status,)


def _gripper_inputs(start_pose: torch.Tensor, goal_pose: torch.Tensor, bounds, *others):
    """What both gripper roadmaps start from: the two pose batches [B,4,4] and the other tensors of the call on the current
    GPU -> B, the device, the poses as contiguous float32 and the position boxes [B,2,3] (``bounds`` None: the box hull of the
    two positions, grown by ``GRIPPER_ROADMAP_BOUNDS_PAD`` per side)."""
    _lib.require_cuda(start_pose, goal_pose, *others)
    assert start_pose.ndim == 3 and tuple(start_pose.shape[1:]) == (4, 4) and goal_pose.shape == start_pose.shape
    B, dev = start_pose.size(0), start_pose.device
    sp, gp = _lib.f32c(start_pose), _lib.f32c(goal_pose)
    if bounds is None:
        ends = torch.stack((sp[:, :3, 3], gp[:, :3, 3]), 1)
        box = torch.stack((ends.amin(1) - GRIPPER_ROADMAP_BOUNDS_PAD, ends.amax(1) + GRIPPER_ROADMAP_BOUNDS_PAD), 1)
    else:
        box = torch.as_tensor(bounds, dtype=torch.float32, device=dev)
        assert tuple(box.shape) in ((2, 3), (B, 2, 3))
        box = box.expand(B, 2, 3)
    return B, dev, sp, gp, _lib.f32c(box)


def gripper_roadmap(start_pose: torch.Tensor, goal_pose: torch.Tensor, cuboids=None, cylinders=None, W: int = 8, bounds=None,
                    seed: int = 0, env_offset: int = 0, return_graph: bool = False, with_base_link: bool = False,
                    finger: float = ft.FINGER_OPENING, **options):
    """A lazy probabilistic roadmap per problem for the free-flying gripper in SE(3) on the GPU (csrc/gripper_roadmap.hip):
    the pose path ``franka_follow`` is handed, planned through the scene for the gripper alone instead of being read off a
    joint-space plan.  A STAND-IN for the reference's OMPL end-effector planner (``gen_data.py:156-189``), NOT a port of it
    and without any claim of parity with AIT*; valid means free by this engine's sphere model (the hand and fingertip
    spheres of the table), not by PyBullet's meshes.  ``nodes`` poses (start, goal and Philox draws keyed by (``seed``,
    ``env_offset`` + row, node): positions in ``bounds``, orientations scattered by ``orient_spread`` about the start-goal
    arc, not uniform on SO(3)) are judged by ``franka_plan``'s clause; the search is ``franka_roadmap``'s over the metric
    sqrt(|dp|^2 + (``rot_weight`` x angle)^2), edges tested every ``resolution`` m.

    :param start_pose, goal_pose: [B,4,4] right_gripper poses, as ``franka_ik`` takes its targets
    :param cuboids, cylinders: as for ``franka_plan``
    :param W: guide poses per problem, 1 .. 64
    :param bounds: None (per problem the box hull of the two positions, grown by ``GRIPPER_ROADMAP_BOUNDS_PAD`` per side),
        [2,3] (lo, hi for every problem) or [B,2,3]
    :param options: the fields of ``mpx_gripper_roadmap_options``, see ``GRIPPER_ROADMAP_DEFAULTS``
    :returns: ``poses`` [B,W,4,4] (at equal steps of the path's metric length, the start not among them, the last one
        ``goal_pose``; NaN rows where ``status`` != 0) and ``status`` int32 [B] (0 path found, 1 none, 2 an endpoint pose is
        non-finite, outside ``bounds`` or invalid); with ``return_graph`` also ``path`` int32 [B,V], ``hops`` int32 [B],
        ``nodes`` [B,V,7] (position, quaternion x y z w), ``edge_state`` uint8 [B,V,V] and ``rounds`` int32 [B], as
        ``franka_roadmap`` returns them."""
    B, dev, sp, gp, box = _gripper_inputs(start_pose, goal_pose, bounds)
    copt, o = _gripper_roadmap_options("gripper_roadmap", options)
    V, W = max(int(o["nodes"]), 0), int(W)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    out = _roadmap_outputs(B, (max(W, 0), 4, 4), V, dev, return_graph)
    _lib.call("mpx_gripper_roadmap", sp.data_ptr(), gp.data_ptr(), B, W, box.data_ptr(), float(finger), *prims,
              *options_tail(copt, seed, env_offset), *_ptrs(out))
    return out if return_graph else out[:2]


def gripper_shortcut(polylines: torch.Tensor, count: torch.Tensor, cuboids=None, cylinders=None, W: int = 8,
                     goal_pose: Optional[torch.Tensor] = None, return_trace: bool = False, with_base_link: bool = False,
                     finger: float = ft.FINGER_OPENING, **options):
    """Shortcut one SE(3) polyline of the free-flying gripper per problem on the GPU (csrc/gripper_shortcut.hip):
    ``franka_shortcut``'s passes, densification and greedy ``fanout``-ary walk over ``gripper_roadmap``'s metric, nlerp edge
    pose and validity, then that roadmap's resampling to ``W`` guide poses.  Part of the same stand-in for the reference's
    end-effector planner, not a port of it.  Deterministic: no seed.

    :param polylines: [B,Pin,7] float32 (position, unit quaternion x y z w; the sign of a quaternion is free), ``count`` int
        [B]: the polyline of a row is its first ``count`` vertices (2 <= count <= Pin <= 256), e.g. ``nodes[path]`` of
        ``gripper_roadmap(..., return_graph=True)``.  The caller vouches for its segments: they are not tested
    :param cuboids, cylinders, W: as for ``gripper_roadmap``
    :param goal_pose: [B,4,4] whose rows 0-2 become the last guide pose bit for bit, or None: the last vertex's own frame
    :param options: the fields of ``mpx_gripper_shortcut_options``, see ``GRIPPER_SHORTCUT_DEFAULTS``
    :returns: ``poses`` [B,W,4,4] (NaN rows where ``status`` != 0), ``status`` int32 [B] (0 a polyline is returned, 2 a bad
        row: count < 2, count > Pin, a non-finite vertex or a quaternion that is not of unit length), ``points_out`` [B,P,7]
        (NaN rows beyond ``count_out``), ``count_out`` int32 [B] and ``length`` [B,2] (metric length before, after); with
        ``return_trace`` also ``chords`` and ``configs`` int32 [B], the chords and interior poses tested."""
    run, o, B, dev = _shortcut_call("gripper_shortcut", polylines, count, 0, return_trace, options, (), W, goal_pose)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    return run("mpx_gripper_shortcut", finger, *prims)


def _gripper_plan_shortcut(shortcut, ropt: dict, V: int) -> Optional[dict]:
    """``shortcut`` of ``gripper_plan`` / ``gripper_plan_cloud`` -> None (off) or the shortcut's options: what it shares with
    the roadmap defaults to the roadmap's values, ``points`` to max(64, nodes)."""
    sopt = _shortcut_arg(shortcut)
    if sopt is None:
        return None
    inherited = {k: ropt[k] for k in ("resolution", "rot_weight", "check_margin", "clearance", "check_self")}
    return {"points": max(GRIPPER_SHORTCUT_DEFAULTS["points"], V), **inherited, **sopt}


def _gripper_plan_result(poses, status, short, return_length: bool):
    """The roadmap's ``poses, status`` with the shortcut's poses in their place (``short``: its outputs, or None)."""
    if short is None:
        length = None
    else:
        poses, length = short[0], short[4]  # (a row without a path is a bad row of the shortcut: NaN)
    return (poses, status, length) if return_length else (poses, status)


def gripper_plan(start_pose: torch.Tensor, goal_pose: torch.Tensor, cuboids=None, cylinders=None, W: int = 8, bounds=None,
                 seed: int = 0, env_offset: int = 0, with_base_link: bool = False, finger: float = ft.FINGER_OPENING,
                 return_length: bool = False, roadmap: Optional[dict] = None, shortcut=True):
    """``gripper_roadmap`` with its graph, then ``gripper_shortcut`` over ``nodes[path]`` with the roadmap's ``goal_pose``:
    the guide poses of the shortened path.  As ``franka_plan_global`` is to ``franka_roadmap``.

    :param roadmap: options of ``gripper_roadmap`` (``GRIPPER_ROADMAP_DEFAULTS``)
    :param shortcut: True, or a dict of ``gripper_shortcut``'s options (``resolution``, ``rot_weight``, ``check_margin``,
        ``clearance`` and ``check_self`` default to the roadmap's, ``points`` to max(64, nodes)); None: the roadmap's poses
        bit for bit
    :returns: ``poses`` [B,W,4,4] and ``status`` int32 [B], the ROADMAP's (rows without a path are NaN); with
        ``return_length`` also ``length`` [B,2], the shortcut's (None without it)."""
    _, ropt = _gripper_roadmap_options("gripper_plan", dict(roadmap or {}))
    sopt = _gripper_plan_shortcut(shortcut, ropt, int(ropt["nodes"]))
    poses, status, *graph = gripper_roadmap(start_pose, goal_pose, cuboids, cylinders, W, bounds, seed, env_offset,
                                            sopt is not None, with_base_link, finger, **(roadmap or {}))
    short = None
    if sopt is not None:
        pts, cnt = _path_vertices(graph[2], graph[0], graph[1])
        short = gripper_shortcut(pts, cnt, cuboids, cylinders, W, goal_pose, False, with_base_link, finger, **sopt)
    return _gripper_plan_result(poses, status, short, return_length)


def task_candidates(support_boxes: torch.Tensor, support_kind: torch.Tensor, cuboids=None, cylinders=None, C: int = 8,
                    seed: int = 0, env_offset: int = 0, role: int = 0, exclude: Optional[torch.Tensor] = None,
                    with_base_link: bool = False, finger: float = ft.FINGER_OPENING, **options):
    """Task-oriented gripper pose candidates on the GPU (csrc/task_candidates.hip): per problem ``draws`` poses drawn ON the
    scene's supports the way the reference's generators pose their problems -- on a SURFACE a point of the top face, lifted
    onto the object it lies on and raised 1 to 12 cm, the gripper pointing down (roll 3pi/4..5pi/4, pitch +-pi/8, yaw
    +-pi/2; ``tabletop_environment.py:354-404``); in a VOLUME a uniform point, the gripper reaching along ``approach`` within
    +-pi/4 (``cubby_environment.py:440-549``) -- and the first ``C`` of them, in draw order, that are free for the
    free-flying gripper.  A restatement of those distributions: free means free by this engine's sphere model (the hand and
    fingertip spheres, ``gripper_roadmap``'s clause), not by PyBullet's meshes, and the IK half of the reference's test is
    ``franka_ik`` on the returned poses.  Draws are Philox keyed by (``seed``, ``env_offset`` + row, draw, ``role``).

    :param support_boxes: [B,S,12] float32 (``scenes.make_task_scenes``): centre, dims, unit quaternion w x y z, approach,
        weight; ``support_kind`` int [B,S]: 0 padding, ``TASK_SURFACE``, ``TASK_VOLUME``
    :param cuboids, cylinders: as for ``franka_plan`` (rotated about z only: a primitive's top is its centre z plus half its
        z extent)
    :param C: kept candidates per problem, 1 .. 16
    :param role: 0 a start, 1 a goal (independent draws); ``exclude``: int [B] or None, the support row not drawn from (-1:
        none) -- the goal call passes the start's support so that the two lie in different pockets
    :param options: the fields of ``mpx_task_candidates_options``, see ``TASK_CANDIDATES_DEFAULTS``
    :returns: ``poses`` [B,C,4,4], ``draw`` int32 [B,C] (the draw index of each kept candidate, strictly ascending),
        ``support`` int32 [B,C] and ``count`` int32 [B]; rows past ``count`` hold NaN poses and -1.  A problem without a live
        support has count 0."""
    if support_boxes.ndim != 3 or support_boxes.size(2) != 12 or tuple(support_kind.shape) != tuple(support_boxes.shape[:2]):
        raise _lib.MpxError(f"task_candidates: support_boxes must be [B,S,12] and support_kind [B,S], got "
                            f"{tuple(support_boxes.shape)} and {tuple(support_kind.shape)}")
    B, NS = support_boxes.shape[:2]
    dev = support_boxes.device
    if exclude is not None and tuple(exclude.shape) != (B,):
        raise _lib.MpxError(f"task_candidates: exclude must be [B={B}], got {tuple(exclude.shape)}")
    copt, _ = merge_options("task_candidates", _lib.TaskCandidatesOptions, TASK_CANDIDATES_DEFAULTS, dict(options, role=role))
    _lib.require_cuda(support_boxes, support_kind, exclude)  # (the refusals above need no device)
    sb, sk = _lib.f32c(support_boxes), _lib.i32c(support_kind)
    ex = None if exclude is None else _lib.i32c(exclude)
    prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
    Cn = max(int(C), 0)
    out = (torch.empty((B, Cn, 4, 4), dtype=torch.float32, device=dev), torch.empty((B, Cn), dtype=torch.int32, device=dev),
           torch.empty((B, Cn), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    _lib.call("mpx_task_candidates", sb.data_ptr(), sk.data_ptr(), B, NS, _lib.ptr(ex), int(C), float(finger), *prims,
              *options_tail(copt, seed, env_offset), *_ptrs(out))
    return out


def _at(p, row, b0):  # row b0 of a [B, ...] operand of 4-byte elements, by its address (``row`` None: not one per problem)
    return p if p is None or row is None else p + 4 * b0 * row


def _follow(who: str, q_start, poses, others: tuple, T, v_init, progress, return_path, return_state, limits, finger, options: dict,
            environment):
    """What ``franka_follow`` and ``franka_follow_cloud`` have in common, which is all but the environment: the inputs and
    options, the outputs, the slabs of problems that share one dense-path buffer of at most ``FOLLOW_PATH_BYTES`` and the
    call of ``mpx_<who>`` per slab.  ``environment(B, dev, o)`` (``o``: the merged options) -> the most problems its own
    operands allow in a slab, ``block(b0, n)`` -> (the environment arguments of problems b0 .. b0 + n - 1, between ``limits``
    and ``v_init``; what trails the outputs), and the tensors to hold until the last call returns."""
    _lib.require_cuda(poses, v_init, progress)
    assert poses.ndim == 4 and tuple(poses.shape[2:]) == (4, 4) and poses.size(0) == q_start.size(0)
    B, dev, qs, vi, lim = _inputs(q_start, (7,), v_init, limits, *others)
    copt, o = _follow_options(who, options)
    W, rows = poses.size(1), min(max(int(o["max_steps"]), 0), FOLLOW_MAX_STEPS) + 1  # (out of range: the call refuses)
    ps = _lib.f32c(poses)
    pg = None
    if progress is not None:
        assert progress.shape == (B, 3)
        pg = _lib.i32c(progress)
    bound, block, held = environment(B, dev, o)  # (``held`` stays in this local until the last call has returned)

    def f32(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    def i32(*shape):
        return torch.empty(shape, dtype=torch.int32, device=dev)

    slab = max(B, 1) if return_path else max(1, min(max(B, 1), FOLLOW_PATH_BYTES // (32 * rows), bound))
    path, arc = f32(B if return_path else min(B, slab), rows, 7), f32(B if return_path else min(B, slab), rows)
    traj, status, bits, steps = f32(B, T, 7), i32(B), i32(B), i32(B)
    traj_any = f32(B, T, 7) if return_path else None
    state = (f32(B, 7), f32(B, 7), i32(B, 3)) if return_state else (None, None, None)
    outs = tuple(zip(_ptrs((path, arc, status, bits, steps, traj, traj_any) + state),  # 4-byte elements per problem behind each
                     (rows * 7 if return_path else 0, rows if return_path else 0, 1, 1, 1, T * 7, T * 7, 7, 7, 3)))
    for b0 in range(0, max(B, 1), slab):
        n = min(slab, B - b0)
        env, trailing = block(b0, n)
        _lib.call("mpx_" + who, _at(qs.data_ptr(), 7, b0), _at(ps.data_ptr(), W * 16, b0), n, W, int(T), float(finger),
                  lim.data_ptr(), *env, _at(_lib.ptr(vi), 7, b0), _at(_lib.ptr(pg), 3, b0), ctypes.byref(copt),
                  *(_at(p, row, b0) for p, row in outs), *trailing)
    out = (traj, status, bits, steps)
    if return_path:
        out += (traj_any, path, arc)
    return out + state if return_state else out


def franka_follow(q_start: torch.Tensor, poses: torch.Tensor, cuboids=None, cylinders=None, T: int = 50,
                  v_init: Optional[torch.Tensor] = None, progress: Optional[torch.Tensor] = None, return_path: bool = False,
                  return_state: bool = False, limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False,
                  finger: float = ft.FINGER_OPENING, **options):
    """Follow a path of end-effector poses with a reactive joint-space controller on the GPU, retime the dense path to ``T``
    waypoints of constant arc-length spacing and judge them (csrc/follow.hip).  A STAND-IN for the Geometric Fabrics
    expert of the reference's data generator (``gen_data.py:156-307``), NOT Lula and without any claim of parity with it:
    a damped second-order system driven by ``franka_ik``'s damped-least-squares direction toward the current guide pose,
    ``franka_plan``'s obstacle gradient, a joint-limit barrier and viscous damping under a joint speed limit.  No
    randomness: row b depends on row b's inputs alone.

    :param q_start: [B,7], inside ``limits`` and collision free.  A start that fails ``franka_plan``'s configuration test is
        refused with status 2 ONLY when ``progress`` is None (a fresh rollout): whenever ``progress`` is given, an all-zero
        one included, that test is skipped, because a continued rollout may stand where its dense path grazed an obstacle
    :param poses: [B,W,4,4] right_gripper guide poses, 1 <= W <= 64, followed in order (switch inside ``switch_radius`` or
        after ``switch_steps``; finished inside ``final_radius`` of the last or after ``final_steps`` on it)
    :param cuboids, cylinders, limits: as for ``franka_plan``
    :param v_init: [B,7] joint velocities (default: zeros); ``progress``: int32 [B,3] = (guide pose, steps spent on it,
        finished flag) (default: zeros).  Pass the ``q_end``, ``v_end``, ``progress_end`` of ``return_state`` back in to
        continue a rollout: the entry is then a controller stepped ``max_steps`` at a time.
    :param options: the fields of ``mpx_follow_options``, see ``FOLLOW_DEFAULTS``
    :returns: ``traj`` [B,T,7] (NaN rows where ``status`` != 0), ``status`` int32 [B] (0 valid, 1 followed but ``bits`` != 0,
        2 bad input: no steps, bits 15), ``bits`` int32 [B] (``PLAN_BIT_ENV_HIT``, ``PLAN_BIT_SELF_HIT``, ``PLAN_BIT_JERK``,
        ``FOLLOW_BIT_MISS``) and ``steps`` int32 [B]; with ``return_path`` also ``traj_any`` [B,T,7] (the status-1 rows
        too), ``path`` [B,max_steps+1,7] and ``arc`` [B,max_steps+1] (rows 0 .. ``steps`` are written, the rest is not);
        with ``return_state`` then ``q_end``, ``v_end`` [B,7] and ``progress_end`` int32 [B,3].  The entry writes the dense
        path whether or not it is returned (32 (max_steps + 1) bytes a problem: 33 kB with the defaults).  With
        ``return_path`` all of it is allocated, 269 MB at B = 8192; without, the batch runs in slabs of problems that
        share one buffer of at most ``FOLLOW_PATH_BYTES`` (rows do not depend on one another: the result is the same)."""
    def environment(B, dev, o):
        prims, held = sphere_primitive_args(cuboids, cylinders, B, dev, with_base_link)
        M1, M2 = prims[6], prims[10]
        prim_rows = (0, 0, 0, None, M1 * 16, M1 * 3, None, M2 * 16, M2, M2, None)  # floats per problem behind each pointer
        return max(B, 1), lambda b0, n: ([_at(p, row, b0) for p, row in zip(prims, prim_rows)], ()), held

    return _follow("franka_follow", q_start, poses, (), T, v_init, progress, return_path, return_state, limits, finger, options,
                   environment)


def plan_cloud_truncation(point_radius: float = 0.0, clearance: float = 0.0, epsilon: float = PLAN_DEFAULTS["epsilon"],
                          voxel: float = 0.03, with_base_link: bool = False) -> float:
    """The truncation ``franka_plan_cloud`` builds its field with: the largest sphere radius + ``point_radius`` +
    ``clearance`` + ``epsilon`` is the farthest a sphere centre can be from a point and still be repelled; two more cells
    keep every corner of a cell inside that band below saturation."""
    rmax = float(ft.collision_sphere_table(with_base_link)[1].max())
    return rmax + float(point_radius) + max(float(clearance), 0.0) + float(epsilon) + 2.0 * float(voxel)


def _plan_cloud_field(who: str, cloud, cn, field, B: int, point_radius: float, clearance: float, epsilon: float,
                      with_base_link: bool):
    """The ``CloudField`` a cloud entry reads: ``field`` checked against the batch, or (None) one built on the default grid
    with ``plan_cloud_truncation(point_radius, clearance, epsilon, voxel)``."""
    if field is None:
        field = CloudField.build(cloud, cn, truncation=plan_cloud_truncation(point_radius, clearance, epsilon, DEFAULT_VOXEL,
                                                                            with_base_link))
    _lib.require_cuda(field.values)
    if field.values.size(0) != B or not field.values.is_contiguous():
        raise _lib.MpxError(f"{who}: the field holds {field.values.size(0)} environments, the batch {B}")
    return field


def franka_plan_cloud(q_start: torch.Tensor, q_goal: torch.Tensor, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None,
                      field=None, point_radius: float = 0.0, T: int = 50, seed: int = 0, env_offset: int = 0,
                      return_all: bool = False, limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False,
                      finger: float = ft.FINGER_OPENING, seeds: Optional[torch.Tensor] = None, **options):
    """``franka_plan`` against one POINT CLOUD per environment instead of primitives (csrc/cloud_field.hip): the same
    candidates, metric, jerk and self tests and lowest-valid-candidate rule.  The obstacle term of an iteration reads a
    truncated distance field of the cloud (``field.CloudField``, built here when ``field`` is None); whether a candidate is
    free is decided by ``FrankaCollisionSampler.check_cloud``'s kernel on its refined configurations, with this
    ``point_radius`` and ``clearance + check_margin`` -- the field steers, the exact test judges.

    :param cloud: [B,N,3] or [B,N,4] float32 on the GPU, any view whose last stride is 1 (``xyz[:, 2048:6144, :3]`` of the
        slab is read in place); ``counts`` optional int [B] as for ``check_cloud``
    :param field: a ``CloudField`` of this cloud (batch B), or None: one is built on the default grid with
        ``plan_cloud_truncation(point_radius, clearance, epsilon, voxel)``
    :param point_radius: radius given to every point (>= 0), in the cost and in the validity test
    :param seeds: None (``mpx_franka_plan_cloud``), or [B,Ks,T,7] caller-supplied starting trajectories
        (``mpx_franka_plan_cloud_seeded``, e.g. ``franka_roadmap_cloud``'s), on ``franka_plan``'s terms: candidates
        ``candidates`` .. ``candidates`` + Ks - 1, behind the drawn ones, which stay bit-equal; a seed with a non-finite entry
        is not optimised (NaN rows, bits 7); ``candidates`` + Ks <= 16.  ``all_traj`` / ``all_status`` then have K + Ks rows.
    :returns: what ``franka_plan`` returns.  A batch whose scratch would exceed ``PLAN_CLOUD_SCRATCH_BYTES`` runs in slabs
        of problems (the draws are keyed by the global row: the result does not depend on the slabbing)."""
    B, dev, qs, qg, lim = _inputs(q_start, (7,), q_goal, limits, cloud, counts)
    copt, o = _plan_options("franka_plan_cloud", options)
    _, cn = cloud_args("franka_plan_cloud", cloud, counts, B, point_radius)  # (the refusals, and the counts for the field)
    field = _plan_cloud_field("franka_plan_cloud", cloud, cn, field, B, point_radius, o["clearance"], o["epsilon"], with_base_link)
    sc, sr, sl = sphere_table(dev, with_base_link)
    entry, sd, Ks = "mpx_franka_plan_cloud", None, 0
    if seeds is not None:
        _lib.require_cuda(seeds)
        assert seeds.ndim == 4 and seeds.size(0) == B and tuple(seeds.shape[2:]) == (int(T), 7)
        entry, sd, Ks = "mpx_franka_plan_cloud_seeded", _lib.f32c(seeds), seeds.size(1)
    K, sub = max(int(o["candidates"]), 0) + Ks, int(o["substeps"])
    out = _plan_outputs(B, K, T, dev, return_all)
    lib = _lib.load()
    per = int(lib.mpx_franka_plan_cloud_scratch(1, int(T), K, sub))
    slab = max(B, 1) if per <= 0 else max(1, min(max(B, 1), PLAN_CLOUD_SCRATCH_BYTES // per))  # (per <= 0: the call refuses)
    nodes = field.values[0].numel() if B else 0
    for b0 in range(0, max(B, 1), slab):
        n = min(slab, B - b0)
        nbytes = max(int(lib.mpx_franka_plan_cloud_scratch(n, int(T), K, sub)), 0)
        buf = scratch_for(dev, nbytes)  # (fetched per call: CloudField.build above, or another entry, may have regrown it)

        def at(t, row):  # pointer to row b0 of a [B, ...] operand
            return None if t is None else t.data_ptr() + b0 * row * t.element_size()

        seeded = () if seeds is None else (at(sd, Ks * T * 7) if Ks else None, Ks)
        _lib.call(entry, at(qs, 7), at(qg, 7), n, int(T), float(finger), lim.data_ptr(), sc.data_ptr(),
                  sr.data_ptr(), sl.data_ptr(), int(sc.size(0)), at(field.values, nodes), ctypes.byref(field.grid),
                  *cloud_args("franka_plan_cloud", cloud, cn, B, point_radius, row=b0)[0],
                  *options_tail(copt, seed, int(env_offset) + b0), *seeded,
                  *(at(t, row) for t, row in zip(out, (T * 7, 1, 1, K * T * 7, K))), buf.data_ptr(), nbytes)
    return out if return_all else out[:2]


def franka_follow_cloud(q_start: torch.Tensor, poses: torch.Tensor, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None,
                        field=None, point_radius: float = 0.0, T: int = 50, v_init: Optional[torch.Tensor] = None,
                        progress: Optional[torch.Tensor] = None, return_path: bool = False, return_state: bool = False,
                        limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False, finger: float = ft.FINGER_OPENING,
                        **options):
    """``franka_follow`` against one POINT CLOUD per environment instead of primitives (csrc/follow_cloud.hip): the same
    stand-in controller (NOT Lula's Geometric Fabrics, no parity claimed), steps, retiming, jerk, self and miss tests.  The
    obstacle term of a step reads a truncated distance field of the cloud (``field.CloudField``, built here when ``field`` is
    None); whether the retimed trajectory is free is decided by ``FrankaCollisionSampler.check_cloud``'s kernel on its
    refined configurations, with this ``point_radius`` and ``clearance + check_margin`` -- the field steers, the exact test
    judges, as in ``franka_plan_cloud``.  A fresh rollout's ``q_start`` is judged by that test too (status 2); with
    ``progress`` given it is not, as for ``franka_follow``.

    :param cloud: [B,N,3] or [B,N,4] float32 on the GPU, any view whose last stride is 1 (``xyz[:, 2048:6144, :3]`` of the
        slab is read in place); ``counts`` optional int [B] as for ``check_cloud`` (a row with count 0 has no environment test)
    :param field: a ``CloudField`` of this cloud (batch B), or None: one is built on the default grid with
        ``plan_cloud_truncation(point_radius, clearance, epsilon, voxel)``
    :param point_radius: radius given to every point (>= 0), in the obstacle term and in the verdict
    :param options: the fields of ``mpx_follow_options``, see ``FOLLOW_DEFAULTS``
    :returns: what ``franka_follow`` returns.  Without ``return_path`` the batch runs in slabs of problems whose dense path
        stays below ``FOLLOW_PATH_BYTES`` and whose scratch stays below ``PLAN_CLOUD_SCRATCH_BYTES`` (rows do not depend on
        one another: the result is the same)."""
    who = "franka_follow_cloud"

    def environment(B, dev, o):
        _, cn = cloud_args(who, cloud, counts, B, point_radius)  # (the refusals, and the counts for the field)
        fld = _plan_cloud_field(who, cloud, cn, field, B, point_radius, o["clearance"], o["epsilon"], with_base_link)
        sc, sr, sl = sphere_table(dev, with_base_link)
        lib, sub = _lib.load(), int(o["substeps"])
        per = int(lib.mpx_franka_follow_cloud_scratch(1, int(T), sub))
        nodes = fld.values[0].numel() if B else 0

        def block(b0, n):
            nbytes = max(int(lib.mpx_franka_follow_cloud_scratch(n, int(T), sub)), 0)
            buf = scratch_for(dev, nbytes)  # (fetched per call: CloudField.build above, or another entry, may have regrown it)
            return ((sc.data_ptr(), sr.data_ptr(), sl.data_ptr(), int(sc.size(0)), _at(fld.values.data_ptr(), nodes, b0),
                     ctypes.byref(fld.grid), *cloud_args(who, cloud, cn, B, point_radius, row=b0)[0]), (buf.data_ptr(), nbytes))

        return PLAN_CLOUD_SCRATCH_BYTES // per if per > 0 else max(B, 1), block, None  # (per <= 0: the call refuses)

    return _follow(who, q_start, poses, (cloud, counts), T, v_init, progress, return_path, return_state, limits, finger, options,
                   environment)


def franka_roadmap_cloud(q_start: torch.Tensor, q_goal: torch.Tensor, cloud: Optional[torch.Tensor],
                         counts: Optional[torch.Tensor] = None, field=None, point_radius: float = 0.0, field_slack: float = 0.0,
                         T: int = 50, seed: int = 0, env_offset: int = 0, return_graph: bool = False,
                         limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False, finger: float = ft.FINGER_OPENING,
                         **options):
    """``franka_roadmap`` against one POINT CLOUD per environment (csrc/roadmap_cloud.hip): the same nodes (the same seed
    draws the same nodes), edges, search, statuses and seed trajectory, with the cloud's truncated distance field as the
    validity test.  A collision sphere blocks a configuration when its centre is inside the grid, the field is not
    saturated there and ``((D - point_radius) - r) - clearance <= check_margin + field_slack``; outside the grid and where
    the field is saturated it counts as free.  The field is an APPROXIMATION: the trilinear interpolant is within
    (sqrt(3)/2) x voxel of the true distance, so a row may get status 2 or 1 where ``check_cloud`` would not object, and a
    path found here may graze the cloud.  The roadmap only seeds ``franka_plan_cloud(seeds=...)``, which judges by the exact
    test; ``franka_plan_global_cloud`` runs the two.

    :param cloud: as for ``franka_plan_cloud``; only used to build the field.  None with ``field`` None: no environment
        (every edge that passes the self test is free)
    :param field: a ``CloudField`` of the cloud (batch B), or None: one is built on the default grid with
        ``plan_cloud_truncation(point_radius, clearance)``
    :param field_slack: >= 0 [m], added to the threshold: 0 uses the field as it is (unbiased), ``0.866 * voxel`` makes the
        roadmap conservative
    :param options: the fields of ``mpx_roadmap_options``, see ``ROADMAP_DEFAULTS``
    :returns: what ``franka_roadmap`` returns."""
    B, dev, qs, qg, lim = _inputs(q_start, (7,), q_goal, limits, cloud, counts)
    copt, o = _roadmap_options("franka_roadmap_cloud", options)
    V = max(int(o["nodes"]), 0)
    if cloud is not None or field is not None:
        cn = None if cloud is None else cloud_args("franka_roadmap_cloud", cloud, counts, B, point_radius)[1]
        field = _plan_cloud_field("franka_roadmap_cloud", cloud, cn, field, B, point_radius, o["clearance"],
                                  PLAN_DEFAULTS["epsilon"], with_base_link)
    sc, sr, sl = sphere_table(dev, with_base_link)
    out = _roadmap_outputs(B, (T, 7), V, dev, return_graph)
    _lib.call("mpx_franka_roadmap_cloud", qs.data_ptr(), _lib.ptr(qg), B, int(T), float(finger), lim.data_ptr(), sc.data_ptr(),
              sr.data_ptr(), sl.data_ptr(), int(sc.size(0)), None if field is None else field.values.data_ptr(),
              None if field is None else ctypes.byref(field.grid), float(point_radius), float(field_slack),
              *options_tail(copt, seed, env_offset), *_ptrs(out))
    return out if return_graph else out[:4]


def franka_shortcut_cloud(polylines: torch.Tensor, count: torch.Tensor, cloud: Optional[torch.Tensor],
                          counts: Optional[torch.Tensor] = None, field=None, point_radius: float = 0.0, field_slack: float = 0.0,
                          T: int = 50, return_trace: bool = False, with_base_link: bool = False,
                          finger: float = ft.FINGER_OPENING, **options):
    """``franka_shortcut`` against one POINT CLOUD per environment (csrc/shortcut_kernel.inc in roadmap_cloud.hip): the same
    passes, densification, greedy walk and outputs, with ``franka_roadmap_cloud``'s validity test -- the cloud's truncated
    distance field, ``point_radius``, ``field_slack``, "outside the grid or saturated: free".  The field approximates the
    distance, so the result only seeds ``franka_plan_cloud(seeds=...)``, which judges by the exact test.

    :param polylines, count: as for ``franka_shortcut``
    :param cloud, counts, field, point_radius, field_slack: as for ``franka_roadmap_cloud`` (None and None: no environment)
    :param options: the fields of ``mpx_shortcut_options``, see ``SHORTCUT_DEFAULTS``
    :returns: what ``franka_shortcut`` returns."""
    who = "franka_shortcut_cloud"
    run, o, B, dev = _shortcut_call(who, polylines, count, T, return_trace, options, (cloud, counts))
    if cloud is not None or field is not None:
        cn = None if cloud is None else cloud_args(who, cloud, counts, B, point_radius)[1]
        field = _plan_cloud_field(who, cloud, cn, field, B, point_radius, o["clearance"], PLAN_DEFAULTS["epsilon"],
                                  with_base_link)
    sc, sr, sl = sphere_table(dev, with_base_link)
    return run("mpx_franka_shortcut_cloud", finger, sc.data_ptr(), sr.data_ptr(), sl.data_ptr(), int(sc.size(0)),
               None if field is None else field.values.data_ptr(), None if field is None else ctypes.byref(field.grid),
               float(point_radius), float(field_slack))


def gripper_roadmap_cloud(start_pose: torch.Tensor, goal_pose: torch.Tensor, cloud: Optional[torch.Tensor],
                          counts: Optional[torch.Tensor] = None, field=None, point_radius: float = 0.0, field_slack: float = 0.0,
                          W: int = 8, bounds=None, seed: int = 0, env_offset: int = 0, return_graph: bool = False,
                          with_base_link: bool = False, finger: float = ft.FINGER_OPENING, **options):
    """``gripper_roadmap`` against one POINT CLOUD per environment (csrc/gripper_roadmap_cloud.hip): the guide poses
    ``franka_follow_cloud`` is handed where a captured cloud has no primitives to plan the gripper through.  The same
    stand-in (NOT a port of the reference's OMPL planner), the same nodes (the same seed draws the same nodes, bit for bit),
    metric, edges, search, statuses and guide poses, with the cloud's truncated distance field as the environment test.  A
    gripper sphere blocks a pose when its centre is inside the grid, the field is not saturated there and
    ``((D - point_radius) - r) - clearance <= check_margin + field_slack``; outside the grid and where the field is
    saturated it counts as free.  The field is an APPROXIMATION: the trilinear interpolant is within (sqrt(3)/2) x voxel of
    the true distance, so a row may get status 2 or 1 where ``check_cloud`` would not object, and a guide pose may graze
    the cloud.  Nothing here is an exact verdict: the exact judge is ``check_cloud`` on whatever trajectory the follower
    produces along these poses.

    :param start_pose, goal_pose, W, bounds: as for ``gripper_roadmap``
    :param cloud, counts: as for ``franka_roadmap_cloud``; only used to build the field.  None with ``field`` None: no
        environment (every pose that passes the self test is valid)
    :param field: a ``CloudField`` of the cloud (batch B), or None: one is built on the default grid with
        ``plan_cloud_truncation(point_radius, clearance)`` at the follower's default ``epsilon``
    :param field_slack: >= 0 [m], added to the threshold: 0 uses the field as it is (unbiased), ``0.866 * voxel`` makes the
        roadmap conservative
    :param options: the fields of ``mpx_gripper_roadmap_options``, see ``GRIPPER_ROADMAP_DEFAULTS``
    :returns: what ``gripper_roadmap`` returns."""
    who = "gripper_roadmap_cloud"
    B, dev, sp, gp, box = _gripper_inputs(start_pose, goal_pose, bounds, cloud, counts)
    copt, o = _gripper_roadmap_options(who, options)
    V, W = max(int(o["nodes"]), 0), int(W)
    if cloud is not None or field is not None:
        cn = None if cloud is None else cloud_args(who, cloud, counts, B, point_radius)[1]
        field = _plan_cloud_field(who, cloud, cn, field, B, point_radius, o["clearance"], FOLLOW_DEFAULTS["epsilon"],
                                  with_base_link)
    sc, sr, sl = sphere_table(dev, with_base_link)
    out = _roadmap_outputs(B, (max(W, 0), 4, 4), V, dev, return_graph)
    _lib.call("mpx_gripper_roadmap_cloud", sp.data_ptr(), gp.data_ptr(), B, W, box.data_ptr(), float(finger), sc.data_ptr(),
              sr.data_ptr(), sl.data_ptr(), int(sc.size(0)), None if field is None else field.values.data_ptr(),
              None if field is None else ctypes.byref(field.grid), float(point_radius), float(field_slack),
              *options_tail(copt, seed, env_offset), *_ptrs(out))
    return out if return_graph else out[:2]


def gripper_shortcut_cloud(polylines: torch.Tensor, count: torch.Tensor, cloud: Optional[torch.Tensor],
                           counts: Optional[torch.Tensor] = None, field=None, point_radius: float = 0.0,
                           field_slack: float = 0.0, W: int = 8, goal_pose: Optional[torch.Tensor] = None,
                           return_trace: bool = False, with_base_link: bool = False, finger: float = ft.FINGER_OPENING,
                           **options):
    """``gripper_shortcut`` against one POINT CLOUD per environment (csrc/gripper_shortcut_cloud.hip): the same passes,
    densification, greedy walk, outputs and guide poses, with ``gripper_roadmap_cloud``'s validity test -- the cloud's
    truncated distance field, ``point_radius``, ``field_slack``, "outside the grid or saturated: free".  The field
    approximates the distance, so a guide pose may graze the cloud: the exact judge is ``check_cloud`` on what the follower
    produces.

    :param polylines, count, W, goal_pose: as for ``gripper_shortcut``
    :param cloud, counts, field, point_radius, field_slack: as for ``gripper_roadmap_cloud`` (None and None: no environment)
    :param options: the fields of ``mpx_gripper_shortcut_options``, see ``GRIPPER_SHORTCUT_DEFAULTS``
    :returns: what ``gripper_shortcut`` returns."""
    who = "gripper_shortcut_cloud"
    run, o, B, dev = _shortcut_call(who, polylines, count, 0, return_trace, options, (cloud, counts), W, goal_pose)
    if cloud is not None or field is not None:
        cn = None if cloud is None else cloud_args(who, cloud, counts, B, point_radius)[1]
        field = _plan_cloud_field(who, cloud, cn, field, B, point_radius, o["clearance"], FOLLOW_DEFAULTS["epsilon"],
                                  with_base_link)
    sc, sr, sl = sphere_table(dev, with_base_link)
    return run("mpx_gripper_shortcut_cloud", finger, sc.data_ptr(), sr.data_ptr(), sl.data_ptr(), int(sc.size(0)),
               None if field is None else field.values.data_ptr(), None if field is None else ctypes.byref(field.grid),
               float(point_radius), float(field_slack))


def gripper_plan_cloud(start_pose: torch.Tensor, goal_pose: torch.Tensor, cloud: Optional[torch.Tensor],
                       counts: Optional[torch.Tensor] = None, field=None, point_radius: float = 0.0, field_slack: float = 0.0,
                       W: int = 8, bounds=None, seed: int = 0, env_offset: int = 0, with_base_link: bool = False,
                       finger: float = ft.FINGER_OPENING, return_length: bool = False, roadmap: Optional[dict] = None,
                       shortcut=True):
    """``gripper_roadmap_cloud`` with its graph, then ``gripper_shortcut_cloud`` over ``nodes[path]`` with the roadmap's
    ``goal_pose``, both reading ONE field of the cloud (built here when ``field`` is None), at the same ``point_radius`` and
    ``field_slack``.  ``roadmap``, ``shortcut`` and what is returned: as for ``gripper_plan``."""
    who = "gripper_plan_cloud"
    _, ropt = _gripper_roadmap_options(who, dict(roadmap or {}))
    sopt = _gripper_plan_shortcut(shortcut, ropt, int(ropt["nodes"]))
    if cloud is not None and field is None and sopt is not None:  # (one field for both; the roadmap alone builds its own)
        B = start_pose.size(0)
        _lib.require_cuda(start_pose, cloud, counts)
        cn = cloud_args(who, cloud, counts, B, point_radius)[1]
        field = _plan_cloud_field(who, cloud, cn, None, B, point_radius, max(ropt["clearance"], sopt["clearance"]),
                                  FOLLOW_DEFAULTS["epsilon"], with_base_link)
    poses, status, *graph = gripper_roadmap_cloud(start_pose, goal_pose, cloud, counts, field, point_radius, field_slack, W,
                                                  bounds, seed, env_offset, sopt is not None, with_base_link, finger,
                                                  **(roadmap or {}))
    short = None
    if sopt is not None:
        pts, cnt = _path_vertices(graph[2], graph[0], graph[1])
        short = gripper_shortcut_cloud(pts, cnt, cloud, counts, field, point_radius, field_slack, W, goal_pose, False,
                                       with_base_link, finger, **sopt)
    return _gripper_plan_result(poses, status, short, return_length)


def franka_plan_global_cloud(q_start: torch.Tensor, q_goal: torch.Tensor, cloud: torch.Tensor,
                             counts: Optional[torch.Tensor] = None, field=None, point_radius: float = 0.0, T: int = 50,
                             seed: int = 0, env_offset: int = 0, return_all: bool = False, limits=ft.JOINT_LIMITS_REAL,
                             with_base_link: bool = False, finger: float = ft.FINGER_OPENING, field_slack: float = 0.0,
                             roadmap: Optional[dict] = None, shortcut=None, **options):
    """``franka_roadmap_cloud``, then ``franka_plan_cloud`` with the roadmap's trajectory as one more candidate behind the
    drawn ones, both reading ONE field of the cloud (built here when ``field`` is None): a row ``franka_plan_cloud`` solves
    comes back identical, a row whose straight line is blocked gets a start that already goes round the obstacle.  Rows
    where the roadmap found nothing pass a NaN seed (bits 7).  Valid is still decided by the exact cloud test alone.

    :param roadmap: options of ``franka_roadmap_cloud`` (``ROADMAP_DEFAULTS``); ``check_margin``, ``clearance`` and
        ``check_self`` default to the planner's values in ``options``
    :param shortcut: None (the call above, unchanged), or True / a dict of ``franka_shortcut_cloud``'s options, on
        ``franka_plan_global``'s terms: two seeds, the shortcut trajectory in front of the roadmap's, through the same field
        at the same ``point_radius`` and ``field_slack``
    :param options: the fields of ``mpx_plan_options``; ``candidates`` (8) + 1 (with ``shortcut``: + 2) <= 16
    :returns: what ``franka_plan_cloud`` returns (``all_traj`` / ``all_status`` with the seeds last), then the roadmap's
        ``status`` int32 [B]."""
    _, o = _plan_options("franka_plan_global_cloud", options)
    B = q_start.size(0)
    _lib.require_cuda(q_start, cloud, counts)
    _, cn = cloud_args("franka_plan_global_cloud", cloud, counts, B, point_radius)
    field = _plan_cloud_field("franka_plan_global_cloud", cloud, cn, field, B, point_radius, o["clearance"], o["epsilon"],
                              with_base_link)
    shared = {k: o[k] for k in ("check_margin", "clearance", "check_self")}
    ropt = dict(shared, **(roadmap or {}))
    sopt = _shortcut_arg(shortcut)
    seed_traj, rm_status, path, hops, *graph = franka_roadmap_cloud(q_start, q_goal, cloud, counts, field, point_radius,
                                                                    field_slack, T, seed, env_offset, sopt is not None, limits,
                                                                    with_base_link, finger, **ropt)
    seeds = seed_traj[:, None]
    if sopt is not None:
        pts, cnt = _path_vertices(graph[0], path, hops)
        inherited = {k: ropt[k] for k in ("check_margin", "clearance", "check_self", "resolution", "smooth_passes") if k in ropt}
        short = franka_shortcut_cloud(pts, cnt, cloud, counts, field, point_radius, field_slack, T, False, with_base_link,
                                      finger, **{"points": max(SHORTCUT_DEFAULTS["points"], pts.size(1)), **inherited, **sopt})[0]
        seeds = torch.stack((short, seed_traj), 1)
    out = franka_plan_cloud(q_start, q_goal, cloud, counts, field, point_radius, T, seed, env_offset, return_all, limits,
                            with_base_link, finger, seeds=seeds, **options)
    return tuple(out) + (rm_status,)
