"""Robot-geometry seam: drop-in equivalents of the robofin classes the reference imports.

Reference call sites (implementations are in un-vendored robofin v0.0.1):
  ``FrankaSampler``            mpinets/model.py:250,267  run_inference.py:64-69,111-116,169,264-265
  ``FrankaCollisionSampler``   mpinets/model.py:268-271,300
  ``FrankaRobot/FrankaRealRobot`` (``JOINT_LIMITS``, ``DOF``, ``fk``)  mpinets/utils.py:50-51,84-85,
                               run_inference.py:176-178, data_loader.py:155-157

All arithmetic runs in ``libmpinets_hip.so`` (csrc/franka.hip).  The kinematic tables are this
repo's (``franka_tables.py``) -- see that file for what is [EXT-RECALL] and what is in-repo data.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import franka_tables as ft
from ._operands import cloud_operand, counts_operand, limits_operand, scratch_for


class _SE3Lite:
    """The few SE3 attributes the reference reads from ``FrankaRobot.fk`` (run_inference.py:180-186)."""

    def __init__(self, matrix: np.ndarray):
        self.matrix = np.asarray(matrix, dtype=np.float64)

    @property
    def xyz(self):
        return self.matrix[:3, 3]

    _xyz = xyz

    @property
    def rotation(self):
        return self.matrix[:3, :3]


class FrankaRobot:
    JOINT_LIMITS = ft.JOINT_LIMITS_PUBLISHED
    DOF = ft.DOF
    NEUTRAL = ft.DEFAULT_Q

    @classmethod
    def within_limits(cls, q) -> bool:
        q = np.asarray(q)
        return bool(np.all(q >= cls.JOINT_LIMITS[:, 0]) and np.all(q <= cls.JOINT_LIMITS[:, 1]))

    @staticmethod
    def fk(q, eff_frame: str = "right_gripper", device: Union[str, torch.device] = "cuda:0") -> _SE3Lite:
        """Single-configuration FK on the GPU; returns an SE3-like with ``.matrix`` / ``.xyz``."""
        qt = torch.as_tensor(np.asarray(q, dtype=np.float32)).reshape(1, 7).to(device)
        frames = franka_fk(qt)[0, ft.LINK_ID[eff_frame]].cpu().numpy().astype(np.float64)
        m = np.eye(4)
        m[:3, :3] = frames[:9].reshape(3, 3)
        m[:3, 3] = frames[9:]
        return _SE3Lite(m)

    @classmethod
    def ik(cls, pose, q_init=None, seed: int = 0, device: Union[str, torch.device] = "cuda:0", **options):
        """One right_gripper pose (4x4, or an SE3-like with ``.matrix``) -> a numpy ``[7]`` inside ``cls.JOINT_LIMITS``
        that reaches it, or ``None`` (robofin's ``ik`` returns a list of solutions; ``franka_ik(..., return_all=True)``
        gives every start's result)."""
        return cls.collision_free_ik(pose, None, None, q_init=q_init, seed=seed, device=device,
                                     **{"check_self": False, **options})

    @classmethod
    def collision_free_ik(cls, pose, cuboids=None, cylinders=None, q_init=None, seed: int = 0,
                          device: Union[str, torch.device] = "cuda:0", cloud=None, counts=None, point_radius: float = 0.0,
                          **options):
        """robofin's ``collision_free_ik(sim, arm, selfcc, pose, retries)`` for one pose: the lowest of 64 starts that
        reaches ``pose`` and is free of ``cuboids`` / ``cylinders`` (``geometry.TorchCuboids`` / ``TorchCylinders`` with a
        batch of one, standing in for the PyBullet ``sim`` / ``arm``) and of the self-collision model (``selfcc``:
        ``check_self=True`` here whether or not primitives are passed; ``check_self=False`` turns it off).  The result
        satisfies ``cls.within_limits``.  Returns a numpy ``[7]`` or ``None``.

        ``cloud`` (``[N,3]``, ``[N,4]`` or ``[1,N,.]``, numpy or tensor; ``counts`` and ``point_radius`` as for
        ``franka_ik_cloud``) asks the same of a point cloud instead; a cloud together with primitives is a ``ValueError``."""
        if cloud is not None and (cuboids is not None or cylinders is not None):
            raise ValueError("collision_free_ik: pass primitives or a cloud, not both")
        m = np.asarray(getattr(pose, "matrix", pose), dtype=np.float32).reshape(1, 4, 4)
        dev = torch.device(device)
        qi = None if q_init is None else torch.as_tensor(np.asarray(q_init, dtype=np.float32)).reshape(1, 7).to(dev)
        if cloud is not None:
            pc = cloud if torch.is_tensor(cloud) else torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32))
            pc = pc.to(dev, dtype=torch.float32)
            if pc.ndim == 2:
                pc = pc.unsqueeze(0)
            if pc.ndim != 3 or pc.size(0) != 1 or pc.size(2) not in (3, 4):
                raise ValueError(f"collision_free_ik: cloud must be [N,3], [N,4] or [1,N,.], got {tuple(pc.shape)}")
            cn = None if counts is None else torch.as_tensor(counts, dtype=torch.int32).reshape(1).to(dev)
            q, status = franka_ik_cloud(torch.from_numpy(m).to(dev), pc, cn, point_radius, q_init=qi, limits=cls.JOINT_LIMITS,
                                        seed=seed, **{"check_self": True, **options})
            return q[0].cpu().numpy().astype(np.float64) if int(status[0]) == 0 else None
        q, status = franka_ik(torch.from_numpy(m).to(dev), cuboids, cylinders, q_init=qi, limits=cls.JOINT_LIMITS,
                              seed=seed, **{"check_self": True, **options})
        return q[0].cpu().numpy().astype(np.float64) if int(status[0]) == 0 else None


class FrankaRealRobot(FrankaRobot):
    JOINT_LIMITS = ft.JOINT_LIMITS_REAL


def franka_fk(q: torch.Tensor, finger: float = ft.FINGER_OPENING) -> torch.Tensor:
    """q [B,7] -> frames [B,15,12] (R row-major 3x3, then t) for ``franka_tables.LINK_NAMES``."""
    _lib.require_cuda(q)
    assert q.ndim == 2 and q.size(1) == 7
    qc = _lib.f32c(q)
    out = torch.empty((q.size(0), ft.NUM_FRAMES, 12), dtype=torch.float32, device=q.device)
    _lib.call("mpx_franka_fk", _lib.ptr(qc), q.size(0), float(finger), _lib.ptr(out))
    return out


IK_SEEDS = 64  # MPX_IK_SEEDS: starts per problem, one per lane
IK_SOLVED, IK_IN_COLLISION, IK_NOT_CONVERGED = 0, 1, 2  # status values of ``franka_ik``
IK_BIT_CONVERGED, IK_BIT_ENV_HIT, IK_BIT_SELF_HIT = 1, 2, 4  # per-start bits of ``return_all``
IK_DEFAULTS = dict(iterations=64, damping=0.05, step_clip=0.5, pos_tol=1e-3, rot_tol=float(np.radians(0.5)),
                   clearance=0.0)
_ik_tables: dict = {}


def _ik_sphere_table(device: torch.device, with_base_link: bool):
    key = (device, bool(with_base_link))
    if key not in _ik_tables:
        c, r, l, _ = ft.collision_sphere_table(with_base_link)
        _ik_tables[key] = tuple(torch.from_numpy(a).to(device) for a in (c, r, l))
    return _ik_tables[key]


def _ik_options(who: str, options: dict, check_self: bool) -> _lib.IkOptions:
    """Keyword options of an IK entry over ``IK_DEFAULTS`` and its ``check_self`` default; ``lambda`` is ``damping``'s C name."""
    opts = IK_DEFAULTS
    if options:  # (most calls pass none: nothing to merge)
        opts = dict(IK_DEFAULTS, check_self=check_self)
        if "lambda" in options:
            options["damping"] = options.pop("lambda")
        if not options.keys() <= opts.keys():
            raise TypeError(f"{who}: unknown option(s) {sorted(options.keys() - opts.keys())}")
        opts.update(options)
        check_self = opts["check_self"]
    return _lib.IkOptions(int(opts["iterations"]), float(opts["damping"]), float(opts["step_clip"]), float(opts["pos_tol"]),
                          float(opts["rot_tol"]), float(opts["clearance"]), int(bool(check_self)))


def _ik_outputs(B: int, dev: torch.device, return_all: bool):  # -> q, status, all_q, all_status (None without return_all)
    return (torch.empty((B, 7), dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty((B, IK_SEEDS, 7), dtype=torch.float32, device=dev) if return_all else None,
            torch.empty((B, IK_SEEDS), dtype=torch.int32, device=dev) if return_all else None)


def _primitive_operands(cuboids, cylinders, B: Optional[int] = None):
    """-> cub frames, dims, M1, cyl frames, radii, heights, M2; the caller holds the tensors (maybe copies) until its call returns."""
    cf = cd = yf = yr = yh = None
    M1 = M2 = 0
    if cuboids is not None:
        assert B is None or cuboids.centers.size(0) == B
        M1 = cuboids.centers.size(1)
        cf, cd = cuboids.inv_frames, _lib.f32c(cuboids.dims)
    if cylinders is not None:
        assert B is None or cylinders.centers.size(0) == B
        M2 = cylinders.centers.size(1)
        yf, yr, yh = cylinders.inv_frames, _lib.f32c(cylinders.radii), _lib.f32c(cylinders.heights)
    return cf, cd, M1, yf, yr, yh, M2


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
    _lib.require_cuda(target_poses, q_init)
    assert target_poses.ndim == 3 and target_poses.shape[1:] == (4, 4)
    B, dev = target_poses.size(0), target_poses.device
    tp = _lib.f32c(target_poses)
    lim = limits_operand(limits, dev)
    assert q_init is None or q_init.shape == (B, 7)
    qi = None if q_init is None else _lib.f32c(q_init)
    copt = _ik_options("franka_ik", options, check_self=cuboids is not None or cylinders is not None)
    cf, cd, M1, yf, yr, yh, M2 = _primitive_operands(cuboids, cylinders, B)
    sc, sr, sl = _ik_sphere_table(dev, with_base_link) if M1 + M2 > 0 else (None, None, None)
    S = 0 if sc is None else int(sc.size(0))
    q, status, all_q, all_status = _ik_outputs(B, dev, return_all)
    _lib.call("mpx_franka_ik", _lib.ptr(tp), B, float(finger), _lib.ptr(lim), _lib.ptr(qi), _lib.ptr(sc), _lib.ptr(sr),
              _lib.ptr(sl), S, _lib.ptr(cf), _lib.ptr(cd), M1, _lib.ptr(yf), _lib.ptr(yr), _lib.ptr(yh), M2,
              ctypes.byref(copt), int(seed) & (2 ** 64 - 1), int(env_offset), _lib.ptr(q), _lib.ptr(status),
              _lib.ptr(all_q), _lib.ptr(all_status))
    return (q, status, all_q, all_status) if return_all else (q, status)


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
    _lib.require_cuda(target_poses, q_init, cloud, counts)
    assert target_poses.ndim == 3 and target_poses.shape[1:] == (4, 4)
    B, dev = target_poses.size(0), target_poses.device
    tp = _lib.f32c(target_poses)
    lim = limits_operand(limits, dev)
    assert q_init is None or q_init.shape == (B, 7)
    qi = None if q_init is None else _lib.f32c(q_init)
    N, cbs, cps = cloud_operand("franka_ik_cloud", cloud, B)
    cn = counts_operand(counts, B)
    sc, sr, sl = _ik_sphere_table(dev, with_base_link)
    S = int(sc.size(0))
    q, status, all_q, all_status = _ik_outputs(B, dev, return_all)
    nbytes = int(_lib.load().mpx_franka_ik_cloud_scratch(B))
    buf = scratch_for(dev, nbytes)
    _lib.call("mpx_franka_ik_cloud", _lib.ptr(tp), B, float(finger), _lib.ptr(lim), _lib.ptr(qi), _lib.ptr(sc), _lib.ptr(sr),
              _lib.ptr(sl), S, _lib.ptr(cloud) if N else None, cbs, cps, N, _lib.ptr(cn), float(point_radius),
              ctypes.byref(copt), int(seed) & (2 ** 64 - 1), int(env_offset), _lib.ptr(q), _lib.ptr(status), _lib.ptr(all_q),
              _lib.ptr(all_status), _lib.ptr(buf), nbytes)
    return (q, status, all_q, all_status) if return_all else (q, status)


PLAN_SOLVED, PLAN_NO_VALID_CANDIDATE, PLAN_BAD_ENDPOINT = 0, 1, 2  # status values of ``franka_plan``
PLAN_BIT_ENV_HIT, PLAN_BIT_SELF_HIT, PLAN_BIT_JERK = 1, 2, 4  # per-candidate bits of ``return_all``
# MPX_PLAN_DEFAULT_* (include/mpinets_hip.h; profiles/plan_timing.md holds the table behind iterations / step / smooth_weight)
PLAN_DEFAULTS = dict(candidates=8, iterations=20, step=2e-4, smooth_weight=20.0, epsilon=0.05, spread=0.5, substeps=4,
                     check_margin=1e-4, clearance=0.0, max_jerk=0.15, check_self=True)


def _plan_options(who: str, options: dict):
    """The keyword options of a planning entry over ``PLAN_DEFAULTS`` (which holds the planners' ``check_self`` default) ->
    the ``_lib.PlanOptions`` and the merged dict, read-only: its values as the caller gave them, not yet float32."""
    if not options.keys() <= PLAN_DEFAULTS.keys():
        raise TypeError(f"{who}: unknown option(s) {sorted(options.keys() - PLAN_DEFAULTS.keys())}")
    o = dict(PLAN_DEFAULTS, **options) if options else PLAN_DEFAULTS  # (most calls pass none: nothing to merge)
    return _lib.PlanOptions(int(o["candidates"]), int(o["iterations"]), float(o["step"]), float(o["smooth_weight"]),
                            float(o["epsilon"]), float(o["spread"]), int(o["substeps"]), float(o["check_margin"]),
                            float(o["clearance"]), float(o["max_jerk"]), int(bool(o["check_self"]))), o


def _plan_outputs(B: int, K: int, T: int, dev: torch.device, return_all: bool):  # -> traj, status, choice, all_traj, all_status
    return (torch.empty((B, T, 7), dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev) if return_all else None,
            torch.empty((B, K, T, 7), dtype=torch.float32, device=dev) if return_all else None,
            torch.empty((B, K), dtype=torch.int32, device=dev) if return_all else None)


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
    _lib.require_cuda(q_start, q_goal)
    assert q_start.ndim == 2 and q_start.size(1) == 7 and q_goal.shape == q_start.shape
    B, dev = q_start.size(0), q_start.device
    qs, qg = _lib.f32c(q_start), _lib.f32c(q_goal)
    lim = limits_operand(limits, dev)
    copt, o = _plan_options("franka_plan", options)
    cf, cd, M1, yf, yr, yh, M2 = _primitive_operands(cuboids, cylinders, B)
    sc, sr, sl = _ik_sphere_table(dev, with_base_link) if M1 + M2 > 0 else (None, None, None)
    S = 0 if sc is None else int(sc.size(0))
    if seeds is None:
        traj, status, choice, all_traj, all_status = _plan_outputs(B, max(int(o["candidates"]), 0), T, dev, return_all)
        _lib.call("mpx_franka_plan", _lib.ptr(qs), _lib.ptr(qg), B, int(T), float(finger), _lib.ptr(lim), _lib.ptr(sc),
                  _lib.ptr(sr), _lib.ptr(sl), S, _lib.ptr(cf), _lib.ptr(cd), M1, _lib.ptr(yf), _lib.ptr(yr), _lib.ptr(yh), M2,
                  ctypes.byref(copt), int(seed) & (2 ** 64 - 1), int(env_offset), _lib.ptr(traj), _lib.ptr(status),
                  _lib.ptr(choice), _lib.ptr(all_traj), _lib.ptr(all_status))
        return (traj, status, choice, all_traj, all_status) if return_all else (traj, status)
    _lib.require_cuda(seeds)
    assert seeds.ndim == 4 and seeds.size(0) == B and tuple(seeds.shape[2:]) == (int(T), 7)
    sd, Ks = _lib.f32c(seeds), seeds.size(1)
    traj, status, choice, all_traj, all_status = _plan_outputs(B, max(int(o["candidates"]), 0) + Ks, T, dev, return_all)
    _lib.call("mpx_franka_plan_seeded", _lib.ptr(qs), _lib.ptr(qg), B, int(T), float(finger), _lib.ptr(lim), _lib.ptr(sc),
              _lib.ptr(sr), _lib.ptr(sl), S, _lib.ptr(cf), _lib.ptr(cd), M1, _lib.ptr(yf), _lib.ptr(yr), _lib.ptr(yh), M2,
              ctypes.byref(copt), int(seed) & (2 ** 64 - 1), int(env_offset), _lib.ptr(sd) if Ks else None, Ks,
              _lib.ptr(traj), _lib.ptr(status), _lib.ptr(choice), _lib.ptr(all_traj), _lib.ptr(all_status))
    return (traj, status, choice, all_traj, all_status) if return_all else (traj, status)


ROADMAP_FOUND, ROADMAP_NO_PATH, ROADMAP_BAD_ENDPOINT = 0, 1, 2  # status values of ``franka_roadmap``
ROADMAP_EDGE_UNTESTED, ROADMAP_EDGE_FREE, ROADMAP_EDGE_BLOCKED = 0, 1, 2  # ``edge_state`` of ``return_graph``
# MPX_ROADMAP_DEFAULT_* (include/mpinets_hip.h; profiles/roadmap_timing.md holds the runs behind them)
ROADMAP_DEFAULTS = dict(nodes=64, resolution=0.05, connect_radius=float("inf"), max_rounds=64, smooth_passes=8,
                        check_margin=1e-4, clearance=0.0, check_self=True)


def _roadmap_options(who: str, options: dict):
    if not options.keys() <= ROADMAP_DEFAULTS.keys():
        raise TypeError(f"{who}: unknown option(s) {sorted(options.keys() - ROADMAP_DEFAULTS.keys())}")
    o = dict(ROADMAP_DEFAULTS, **options) if options else ROADMAP_DEFAULTS
    return _lib.RoadmapOptions(int(o["nodes"]), float(o["resolution"]), float(o["connect_radius"]), int(o["max_rounds"]),
                               int(o["smooth_passes"]), float(o["check_margin"]), float(o["clearance"]),
                               int(bool(o["check_self"]))), o


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
    _lib.require_cuda(q_start, q_goal)
    assert q_start.ndim == 2 and q_start.size(1) == 7 and q_goal.shape == q_start.shape
    B, dev = q_start.size(0), q_start.device
    qs, qg = _lib.f32c(q_start), _lib.f32c(q_goal)
    lim = limits_operand(limits, dev)
    copt, o = _roadmap_options("franka_roadmap", options)
    V = max(int(o["nodes"]), 0)
    cf, cd, M1, yf, yr, yh, M2 = _primitive_operands(cuboids, cylinders, B)
    sc, sr, sl = _ik_sphere_table(dev, with_base_link) if M1 + M2 > 0 else (None, None, None)
    S = 0 if sc is None else int(sc.size(0))
    traj = torch.empty((B, T, 7), dtype=torch.float32, device=dev)
    status, hops = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2))
    path = torch.empty((B, V), dtype=torch.int32, device=dev)
    nodes = torch.empty((B, V, 7), dtype=torch.float32, device=dev) if return_graph else None
    edge_state = torch.empty((B, V, V), dtype=torch.uint8, device=dev) if return_graph else None
    rounds = torch.empty(B, dtype=torch.int32, device=dev) if return_graph else None
    _lib.call("mpx_franka_roadmap", _lib.ptr(qs), _lib.ptr(qg), B, int(T), float(finger), _lib.ptr(lim), _lib.ptr(sc),
              _lib.ptr(sr), _lib.ptr(sl), S, _lib.ptr(cf), _lib.ptr(cd), M1, _lib.ptr(yf), _lib.ptr(yr), _lib.ptr(yh), M2,
              ctypes.byref(copt), int(seed) & (2 ** 64 - 1), int(env_offset), _lib.ptr(traj), _lib.ptr(status),
              _lib.ptr(path), _lib.ptr(hops), _lib.ptr(nodes), _lib.ptr(edge_state), _lib.ptr(rounds))
    return (traj, status, path, hops, nodes, edge_state, rounds) if return_graph else (traj, status, path, hops)


def franka_plan_global(q_start: torch.Tensor, q_goal: torch.Tensor, cuboids=None, cylinders=None, T: int = 50, seed: int = 0,
                       env_offset: int = 0, return_all: bool = False, limits=ft.JOINT_LIMITS_REAL,
                       with_base_link: bool = False, finger: float = ft.FINGER_OPENING, roadmap: Optional[dict] = None,
                       **options):
    """``franka_roadmap``, then ``franka_plan`` with the roadmap's trajectory as one more candidate behind the drawn ones:
    a row ``franka_plan`` solves comes back identical, a row whose straight line is blocked gets a start that already
    goes round the obstacle.  Rows where the roadmap found nothing pass a NaN seed (bits 7).

    :param roadmap: options of ``franka_roadmap`` (``ROADMAP_DEFAULTS``); ``check_margin``, ``clearance`` and ``check_self``
        default to the planner's values in ``options``
    :param options: the fields of ``mpx_plan_options``; ``candidates`` (8) + 1 <= 16
    :returns: what ``franka_plan`` returns (``all_traj`` / ``all_status`` with ``candidates`` + 1 rows, the seed last), then
        the roadmap's ``status`` int32 [B]."""
    _, o = _plan_options("franka_plan_global", options)
    shared = {k: o[k] for k in ("check_margin", "clearance", "check_self")}
    seed_traj, rm_status, _, _ = franka_roadmap(q_start, q_goal, cuboids, cylinders, T, seed, env_offset, False, limits,
                                                with_base_link, finger, **dict(shared, **(roadmap or {})))
    out = franka_plan(q_start, q_goal, cuboids, cylinders, T, seed, env_offset, return_all, limits, with_base_link, finger,
                      seeds=seed_traj[:, None], **options)
    return tuple(out) + (rm_status,)


PLAN_CLOUD_SCRATCH_BYTES = 256 << 20  # ``franka_plan_cloud`` runs a large batch in slabs of problems whose scratch stays below this


def plan_cloud_truncation(point_radius: float = 0.0, clearance: float = 0.0, epsilon: float = PLAN_DEFAULTS["epsilon"],
                          voxel: float = 0.03, with_base_link: bool = False) -> float:
    """The truncation ``franka_plan_cloud`` builds its field with: the largest sphere radius + ``point_radius`` +
    ``clearance`` + ``epsilon`` is the farthest a sphere centre can be from a point and still be repelled; two more cells
    keep every corner of a cell inside that band below saturation."""
    rmax = float(ft.collision_sphere_table(with_base_link)[1].max())
    return rmax + float(point_radius) + max(float(clearance), 0.0) + float(epsilon) + 2.0 * float(voxel)


def franka_plan_cloud(q_start: torch.Tensor, q_goal: torch.Tensor, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None,
                      field=None, point_radius: float = 0.0, T: int = 50, seed: int = 0, env_offset: int = 0,
                      return_all: bool = False, limits=ft.JOINT_LIMITS_REAL, with_base_link: bool = False,
                      finger: float = ft.FINGER_OPENING, **options):
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
    :returns: what ``franka_plan`` returns.  A batch whose scratch would exceed ``PLAN_CLOUD_SCRATCH_BYTES`` runs in slabs
        of problems (the draws are keyed by the global row: the result does not depend on the slabbing)."""
    from .field import DEFAULT_VOXEL, CloudField

    _lib.require_cuda(q_start, q_goal, cloud, counts)
    assert q_start.ndim == 2 and q_start.size(1) == 7 and q_goal.shape == q_start.shape
    B, dev = q_start.size(0), q_start.device
    qs, qg = _lib.f32c(q_start), _lib.f32c(q_goal)
    lim = limits_operand(limits, dev)
    copt, o = _plan_options("franka_plan_cloud", options)
    N, cbs, cps = cloud_operand("franka_plan_cloud", cloud, B)
    cn = counts_operand(counts, B)
    if field is None:
        field = CloudField.build(cloud, cn, truncation=plan_cloud_truncation(point_radius, o["clearance"], o["epsilon"],
                                                                            DEFAULT_VOXEL, with_base_link))
    _lib.require_cuda(field.values)
    if field.values.size(0) != B or not field.values.is_contiguous():
        raise _lib.MpxError(f"franka_plan_cloud: the field holds {field.values.size(0)} environments, the batch {B}")
    sc, sr, sl = _ik_sphere_table(dev, with_base_link)
    S = int(sc.size(0))
    K = max(int(o["candidates"]), 0)
    traj, status, choice, all_traj, all_status = _plan_outputs(B, K, T, dev, return_all)
    lib = _lib.load()
    per = int(lib.mpx_franka_plan_cloud_scratch(1, int(T), K, int(o["substeps"])))
    slab = max(B, 1) if per <= 0 else max(1, min(max(B, 1), PLAN_CLOUD_SCRATCH_BYTES // per))  # (per <= 0: the call refuses)
    nodes = field.values[0].numel() if B else 0
    for b0 in range(0, max(B, 1), slab):
        n = min(slab, B - b0)
        nbytes = max(int(lib.mpx_franka_plan_cloud_scratch(n, int(T), K, int(o["substeps"]))), 0)
        buf = scratch_for(dev, nbytes)  # (fetched per call: CloudField.build above, or another entry, may have regrown it)

        def at(t, row):  # pointer to row b0 of a [B, ...] operand
            return None if t is None else t.data_ptr() + b0 * row * t.element_size()

        _lib.call("mpx_franka_plan_cloud", at(qs, 7), at(qg, 7), n, int(T), float(finger), _lib.ptr(lim), _lib.ptr(sc),
                  _lib.ptr(sr), _lib.ptr(sl), S, at(field.values, nodes), ctypes.byref(field.grid), at(cloud, cbs), cbs, cps, N,
                  at(cn, 1), float(point_radius), ctypes.byref(copt), int(seed) & (2 ** 64 - 1), int(env_offset) + b0,
                  at(traj, T * 7), at(status, 1), at(choice, 1), at(all_traj, K * T * 7), at(all_status, K), _lib.ptr(buf),
                  nbytes)
    return (traj, status, choice, all_traj, all_status) if return_all else (traj, status)


def frames_to_matrix(frames: torch.Tensor) -> torch.Tensor:
    """[...,12] -> [...,4,4]."""
    m = torch.zeros(frames.shape[:-1] + (4, 4), dtype=frames.dtype, device=frames.device)
    m[..., :3, :3] = frames[..., :9].reshape(frames.shape[:-1] + (3, 3))
    m[..., :3, 3] = frames[..., 9:]
    m[..., 3, 3] = 1
    return m


class _SampleFn(torch.autograd.Function):
    """``FrankaSampler.sample`` under autograd (the reference differentiates robofin's torch FK, loss.py:142-147)."""

    @staticmethod
    def forward(ctx, q, sampler, subset, n_out):
        out = torch.empty((q.size(0), n_out, 3), dtype=torch.float32, device=q.device)
        qc = _lib.f32c(q.detach())
        sampler.sample_into(qc, out, subset)
        ctx.sampler, ctx.subset, ctx.n_out = sampler, subset, n_out
        ctx.save_for_backward(qc)
        return out

    @staticmethod
    def backward(ctx, g):
        (qc,) = ctx.saved_tensors
        s, g = ctx.sampler, _lib.f32c(g)
        gq = torch.empty_like(qc)
        _lib.call("mpx_franka_cloud_grad", _lib.ptr(qc), qc.size(0), s.finger, _lib.ptr(s.table_pts),
                  _lib.ptr(s.table_link), _lib.ptr(ctx.subset), ctx.n_out, _lib.ptr(g), g.stride(0), g.stride(1),
                  _lib.ptr(gq))
        return gq, None, None, None


class FrankaSampler:
    """Robot-surface point clouds by FK of a per-link point table.

    ``FrankaSampler(device, num_fixed_points=None, use_cache=False, with_base_link=True)`` as in
    the reference's call sites.  ``sample(q, num_points)`` draws ONE random column subset per call
    from the host ``np.random`` stream and shares it across the batch, like robofin
    (SURVEY.md row a8); ``num_fixed_points`` freezes that subset at construction
    (``loss.py:142-153`` usage).  ``sample_into`` is the engine's zero-copy form used by rollouts.
    """

    def __init__(self, device, num_fixed_points: Optional[int] = None, use_cache: bool = False,
                 with_base_link: bool = True, point_table: Optional[Tuple[np.ndarray, np.ndarray]] = None,
                 finger: float = ft.FINGER_OPENING):
        # ``FrankaSampler("cpu", use_cache=True)`` is how the reference builds its host-side clouds
        # (run_inference.py:262, data_loader.py:101): accepted as a HOST-FACING handle -- inputs and results are CPU
        # tensors, the arithmetic still runs in the HIP library on the current GPU (there is no CPU implementation;
        # without a GPU this raises).
        self.io_device = torch.device(device)
        if self.io_device.type == "cuda":
            self.device = self.io_device
        else:
            if not torch.cuda.is_available():
                raise _lib.MpxError("FrankaSampler needs a GPU (the HIP engine has no CPU fallback)")
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.with_base_link = with_base_link
        self.num_fixed_points = num_fixed_points
        self.finger = float(finger)
        pts, links = point_table if point_table is not None else ft.link_point_table(4096, with_base_link)
        self.table_pts = torch.as_tensor(np.ascontiguousarray(pts, dtype=np.float32)).to(self.device)
        self.table_link = torch.as_tensor(np.ascontiguousarray(links, dtype=np.int32)).to(self.device)
        self.eef_table = torch.as_tensor(ft.end_effector_point_table()).to(self.device)
        self.num_table_points = int(self.table_pts.size(0))
        self._fixed = None
        if num_fixed_points is not None:
            self._fixed = self._draw(num_fixed_points)

    # -- subsets ------------------------------------------------------------------------------
    def _draw(self, n: int, total: Optional[int] = None) -> torch.Tensor:
        total = self.num_table_points if total is None else total
        idx = np.random.choice(total, n, replace=False).astype(np.int32)
        return torch.from_numpy(idx).to(self.device)

    def draw_subset(self, num_points: int) -> torch.Tensor:
        """A device index tensor usable with ``sample_into`` (one host RNG call, no sync later)."""
        return self._draw(num_points)

    # -- reference API ------------------------------------------------------------------------
    def sample(self, q: torch.Tensor, num_points: Optional[int] = None) -> torch.Tensor:
        """q [B,7] (or [7]) joint angles -> [B,P,3]."""
        if q.ndim == 1:
            q = q.unsqueeze(0)
        if self.io_device.type != "cuda":  # host-facing handle: compute on the GPU, hand the result back
            assert not (torch.is_grad_enabled() and q.requires_grad), "differentiable sampling needs the GPU handle"
            q = q.to(self.device, dtype=torch.float32)
        _lib.require_cuda(q)
        if self._fixed is not None:
            subset = self._fixed
        elif num_points is None:
            subset = None
        else:
            subset = self._draw(num_points)
        n_out = self.num_table_points if subset is None else int(subset.numel())
        if torch.is_grad_enabled() and q.requires_grad:
            return _SampleFn.apply(q, self, subset, n_out)
        out = torch.empty((q.size(0), n_out, 3), dtype=torch.float32, device=q.device)
        self.sample_into(q, out, subset)
        return out.to(self.io_device)

    def sample_into(self, q: torch.Tensor, out: torch.Tensor, subset: Optional[torch.Tensor]) -> None:
        """Write ``out[:, :n, :3]`` in place; ``out`` may be the xyz slab itself ([B,N,4] or [B,n,3])."""
        assert q.ndim == 2 and q.size(1) == 7 and out.ndim == 3 and out.size(0) == q.size(0)
        assert out.dtype == torch.float32 and out.stride(2) == 1
        n_out = self.num_table_points if subset is None else int(subset.numel())
        assert out.size(1) >= n_out
        qc = _lib.f32c(q)
        _lib.call("mpx_franka_cloud", _lib.ptr(qc), q.size(0), self.finger, _lib.ptr(self.table_pts),
                  _lib.ptr(self.table_link), _lib.ptr(subset), n_out, _lib.ptr(out), out.stride(0), out.stride(1))

    def sample_end_effector(self, poses: torch.Tensor, num_points: int, frame: str = "right_gripper",
                            subset: Optional[torch.Tensor] = None) -> torch.Tensor:
        """poses [B,4,4] of ``frame`` -> gripper points [B,num_points,3] (run_inference.py:66-69).  ``subset`` (optional,
        int32 indices into the gripper table): use these rows instead of drawing ``num_points`` of them."""
        if poses.ndim == 2:
            poses = poses.unsqueeze(0)
        poses = poses.to(self.device, dtype=torch.float32)  # (no-op for the GPU handle)
        _lib.require_cuda(poses)
        assert poses.shape[1:] == (4, 4)
        table = self.eef_table if frame == "right_gripper" else torch.as_tensor(
            ft.end_effector_point_table(frame=frame)).to(self.device)
        if subset is None:
            subset = self._draw(num_points, total=int(table.size(0)))
        subset = subset.to(device=self.device, dtype=torch.int32).contiguous()
        assert subset.numel() == num_points
        out = torch.empty((poses.size(0), num_points, 3), dtype=torch.float32, device=poses.device)
        pc = _lib.f32c(poses)
        _lib.call("mpx_pose_cloud", _lib.ptr(pc), poses.size(0), _lib.ptr(table), _lib.ptr(subset), num_points,
                  _lib.ptr(out), out.stride(0), out.stride(1))
        return out.to(self.io_device)

    def end_effector_pose(self, q: torch.Tensor, frame: str = "right_gripper") -> torch.Tensor:
        """q [B,7] -> [B,4,4] (model.py:275)."""
        if q.ndim == 1:
            q = q.unsqueeze(0)
        return frames_to_matrix(franka_fk(q.to(self.device, dtype=torch.float32), self.finger)[:, ft.LINK_ID[frame]]).to(self.io_device)


class FrankaCollisionSampler:
    """Collision-sphere model of the arm (model.py:268-271,300)."""

    def __init__(self, device, with_base_link: bool = False, finger: float = ft.FINGER_OPENING):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MpxError("FrankaCollisionSampler needs a GPU device (no CPU fallback)")
        c, r, l, groups = ft.collision_sphere_table(with_base_link)
        self.centers = torch.from_numpy(c).to(self.device)
        self.radii = torch.from_numpy(r).to(self.device)
        self.links = torch.from_numpy(l).to(self.device)
        self.groups = groups
        self.num_spheres = int(c.shape[0])
        self.finger = float(finger)

    def sphere_centers(self, q: torch.Tensor) -> torch.Tensor:
        """q [B,7] -> [B,S,3] in table order (grouped by radius)."""
        _lib.require_cuda(q)
        qc = _lib.f32c(q)
        out = torch.empty((q.size(0), self.num_spheres, 3), dtype=torch.float32, device=q.device)
        _lib.call("mpx_franka_spheres", _lib.ptr(qc), q.size(0), self.finger, _lib.ptr(self.centers),
                  _lib.ptr(self.links), self.num_spheres, _lib.ptr(out))
        return out

    def compute_spheres(self, q: torch.Tensor) -> List[Tuple[float, torch.Tensor]]:
        """-> [(radius, centres [B,S_r,3]), ...] like robofin's ``compute_spheres``."""
        allc = self.sphere_centers(q)
        return [(r, allc[:, s:s + n]) for r, s, n in self.groups]

    def check(self, q: torch.Tensor, cuboids, cylinders, return_sdf: bool = False):
        """Fused swept-sphere collision check of trajectories (model.py:293-314).

        :param q: [B,T,7] (or [B,7]) joint angles
        :param cuboids: ``geometry.TorchCuboids`` or None;  :param cylinders: ``TorchCylinders`` or None
        :returns: ``has_collision`` bool [B] (and ``min_sdf`` [B,T,S] when ``return_sdf``)
        """
        if q.ndim == 2:
            q = q.unsqueeze(1)
        _lib.require_cuda(q)
        B, T, _ = q.shape
        qc = _lib.f32c(q)
        flags = torch.zeros(B, dtype=torch.int32, device=q.device)
        msdf = torch.empty((B, T, self.num_spheres), dtype=torch.float32, device=q.device) if return_sdf else None
        cf, cd, M1, yf, yr, yh, M2 = _primitive_operands(cuboids, cylinders)
        _lib.call("mpx_franka_collision", _lib.ptr(qc), B, T, self.finger, _lib.ptr(self.centers),
                  _lib.ptr(self.radii), _lib.ptr(self.links), self.num_spheres, _lib.ptr(cf), _lib.ptr(cd), M1,
                  _lib.ptr(yf), _lib.ptr(yr), _lib.ptr(yh), M2, _lib.ptr(flags), _lib.ptr(msdf))
        has = flags != 0
        return (has, msdf) if return_sdf else has

    def check_cloud(self, q: torch.Tensor, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None,
                    point_radius: float = 0.0, clearance: float = 0.0, return_distance: bool = False,
                    return_nearest: bool = False):
        """Swept-sphere check of trajectories against one POINT CLOUD per environment (csrc/cloud_collision.hip): the
        scene as the policy sees it -- a depth cloud, a captured cloud, the scene rows of the xyz slab -- with no
        primitives behind it.

        :param q: [B,T,7] (or [B,7]) joint angles
        :param cloud: [B,N,3] or [B,N,4] float32 on the GPU; any view whose last stride is 1 is read in place
            (``xyz[:, 2048:6144, :3]`` of the slab), rows with a NaN or infinite coordinate are ignored
        :param counts: optional int [B]: only the first ``counts[b]`` rows of environment b exist (clamped to [0, N])
        :param point_radius: radius given to every point, >= 0.  The test is sphere-CENTRE to POINT distance
            ``<= (r_s + point_radius) + clearance``: a surface sampled at spacing h can pass between its points, and this
            is the caller's way to close that gap.  No default is right for every cloud; 0 is the bare points.
        :returns: ``has_collision`` bool [B]; then ``min_dist`` [B,T,S] (distance of every sphere centre to the surface
            of its nearest point's ball, +inf without points) when ``return_distance`` and ``nearest`` int32 [B,T,S]
            (that point's row, lowest on a tie, -1 without points) when ``return_nearest``
        """
        if q.ndim == 2:
            q = q.unsqueeze(1)
        _lib.require_cuda(q, cloud, counts)
        B, T, _ = q.shape
        N, cbs, ps = cloud_operand("check_cloud", cloud, B, empty_batch_any_stride=False)
        qc = _lib.f32c(q)
        cn = counts_operand(counts, B)
        flags = torch.zeros(B, dtype=torch.int32, device=q.device)
        S = self.num_spheres
        dist = torch.empty((B, T, S), dtype=torch.float32, device=q.device) if return_distance else None
        near = torch.empty((B, T, S), dtype=torch.int32, device=q.device) if return_nearest else None
        _lib.call("mpx_franka_cloud_collision", _lib.ptr(qc), B, T, self.finger, _lib.ptr(self.centers),
                  _lib.ptr(self.radii), _lib.ptr(self.links), S, _lib.ptr(cloud), cbs, ps, N,
                  _lib.ptr(cn), float(point_radius), float(clearance), _lib.ptr(flags), _lib.ptr(dist), _lib.ptr(near))
        out = (flags != 0,) + ((dist,) if return_distance else ()) + ((near,) if return_nearest else ())
        return out if len(out) > 1 else out[0]

    def check_cloud_each(self, q: torch.Tensor, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None,
                         point_radius: float = 0.0, clearance: float = 0.0, active: Optional[torch.Tensor] = None):
        """``check_cloud`` with one verdict per WAYPOINT (``mpx_franka_cloud_collision_each``): the same cloud and stride
        rules, the same test.

        :param q: [B,T,7] (or [B,7]) joint angles
        :param active: optional bool / int [B,T]: waypoints with a zero are not tested (their q is not read) and come back
            False
        :returns: ``hit`` bool [B,T]: ``hit[b,t]`` is what ``check_cloud`` answers for the single configuration ``q[b,t]``
            against environment b's cloud; ``hit.any(1)`` is ``check_cloud(q, cloud)``
        """
        if q.ndim == 2:
            q = q.unsqueeze(1)
        _lib.require_cuda(q, cloud, counts, active)
        B, T, _ = q.shape
        N, cbs, ps = cloud_operand("check_cloud_each", cloud, B, empty_batch_any_stride=False)
        qc = _lib.f32c(q)
        cn = counts_operand(counts, B)
        ac = None
        if active is not None:
            assert active.shape == (B, T)
            ac = _lib.i32c(active)
        hit = torch.empty((B, T), dtype=torch.int32, device=q.device)
        _lib.call("mpx_franka_cloud_collision_each", _lib.ptr(qc), B, T, self.finger, _lib.ptr(self.centers),
                  _lib.ptr(self.radii), _lib.ptr(self.links), self.num_spheres, _lib.ptr(cloud), cbs, ps, N,
                  _lib.ptr(cn), float(point_radius), float(clearance), _lib.ptr(ac), _lib.ptr(hit))
        return hit != 0
