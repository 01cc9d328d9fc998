"""Robot-geometry seam: drop-in equivalents of the robofin classes the reference imports.

Reference call sites (implementations are in un-vendored robofin v0.0.1):
  ``FrankaSampler``            mpinets/model.py:250,267  run_inference.py:64-69,111-116,169,264-265
  ``FrankaCollisionSampler``   mpinets/model.py:268-271,300
  ``FrankaRobot/FrankaRealRobot`` (``JOINT_LIMITS``, ``DOF``, ``fk``)  mpinets/utils.py:50-51,84-85,
                               run_inference.py:176-178, data_loader.py:155-157

All arithmetic runs in ``libmpinets_hip.so`` (csrc/franka.hip).  The kinematic tables are this
repo's (``franka_tables.py``) -- see that file for what is [EXT-RECALL] and what is in-repo data.

This module holds those classes, ``franka_fk`` and ``frames_to_matrix``.  The device solvers (``franka_ik``, ``franka_plan``,
``franka_roadmap``, ... and their constants and option helpers) live in ``solvers.py``; every name of theirs that this
module used to define is re-exported below, so ``robot.franka_plan`` is ``solvers.franka_plan``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import franka_tables as ft
from ._operands import cloud_args, sphere_primitive_args
from .solvers import (FOLLOW_BAD_INPUT, FOLLOW_BIT_MISS, FOLLOW_DEFAULTS, FOLLOW_INVALID, FOLLOW_MAX_STEPS,  # noqa: F401
                      FOLLOW_PATH_BYTES, FOLLOW_VALID, _follow_options, franka_follow, franka_follow_cloud)
from .solvers import (GRIPPER_ROADMAP_BOUNDS_PAD, GRIPPER_ROADMAP_DEFAULTS, _gripper_roadmap_options,  # noqa: F401
                      gripper_roadmap, gripper_roadmap_cloud)
from .solvers import (GRIPPER_SHORTCUT_DEFAULTS, _gripper_shortcut_options, gripper_plan, gripper_plan_cloud,  # noqa: F401
                      gripper_shortcut, gripper_shortcut_cloud)
from .solvers import (SHORTCUT_BAD_ROW, SHORTCUT_DEFAULTS, SHORTCUT_RETURNED, _shortcut_options, franka_shortcut,  # noqa: F401
                      franka_shortcut_cloud)
from .solvers import TASK_CANDIDATES_DEFAULTS, TASK_SURFACE, TASK_VOLUME, task_candidates  # noqa: F401
from .solvers import (IK_BIT_CONVERGED, IK_BIT_ENV_HIT, IK_BIT_SELF_HIT, IK_DEFAULTS, IK_IN_COLLISION,  # noqa: F401
                      IK_NOT_CONVERGED, IK_SEEDS, IK_SOLVED, PLAN_BAD_ENDPOINT, PLAN_BIT_ENV_HIT, PLAN_BIT_JERK,
                      PLAN_BIT_SELF_HIT, PLAN_CLOUD_SCRATCH_BYTES, PLAN_DEFAULTS, PLAN_NO_VALID_CANDIDATE, PLAN_SOLVED,
                      ROADMAP_BAD_ENDPOINT, ROADMAP_DEFAULTS, ROADMAP_EDGE_BLOCKED, ROADMAP_EDGE_FREE, ROADMAP_EDGE_UNTESTED,
                      ROADMAP_FOUND, ROADMAP_NO_PATH, _ik_options, _ik_outputs, _ik_sphere_table, _plan_options,
                      _plan_outputs, _roadmap_options, franka_ik, franka_ik_cloud, franka_plan, franka_plan_cloud,
                      franka_plan_global, franka_plan_global_cloud, franka_roadmap, franka_roadmap_cloud,
                      plan_cloud_truncation)


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
        common = dict(q_init=qi, limits=cls.JOINT_LIMITS, seed=seed, **{"check_self": True, **options})
        if cloud is None:
            q, status = franka_ik(torch.from_numpy(m).to(dev), cuboids, cylinders, **common)
        else:
            pc = cloud if torch.is_tensor(cloud) else torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32))
            pc = pc.to(dev, dtype=torch.float32)
            if pc.ndim == 2:
                pc = pc.unsqueeze(0)
            if pc.ndim != 3 or pc.size(0) != 1 or pc.size(2) not in (3, 4):
                raise ValueError(f"collision_free_ik: cloud must be [N,3], [N,4] or [1,N,.], got {tuple(pc.shape)}")
            cn = None if counts is None else torch.as_tensor(counts, dtype=torch.int32).reshape(1).to(dev)
            q, status = franka_ik_cloud(torch.from_numpy(m).to(dev), pc, cn, point_radius, **common)
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
        prims, held = sphere_primitive_args(cuboids, cylinders, table=(self.centers, self.radii, self.links))
        _lib.call("mpx_franka_collision", qc.data_ptr(), B, T, self.finger, *prims, flags.data_ptr(), _lib.ptr(msdf))
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
        points, held = cloud_args("check_cloud", cloud, counts, B, point_radius, empty_batch_any_stride=False)
        qc = _lib.f32c(q)
        flags = torch.zeros(B, dtype=torch.int32, device=q.device)
        S = self.num_spheres
        dist = torch.empty((B, T, S), dtype=torch.float32, device=q.device) if return_distance else None
        near = torch.empty((B, T, S), dtype=torch.int32, device=q.device) if return_nearest else None
        _lib.call("mpx_franka_cloud_collision", qc.data_ptr(), B, T, self.finger, self.centers.data_ptr(),
                  self.radii.data_ptr(), self.links.data_ptr(), S, *points, float(clearance), flags.data_ptr(),
                  _lib.ptr(dist), _lib.ptr(near))
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
        points, held = cloud_args("check_cloud_each", cloud, counts, B, point_radius, empty_batch_any_stride=False)
        qc = _lib.f32c(q)
        ac = None
        if active is not None:
            assert active.shape == (B, T)
            ac = _lib.i32c(active)
        hit = torch.empty((B, T), dtype=torch.int32, device=q.device)
        _lib.call("mpx_franka_cloud_collision_each", qc.data_ptr(), B, T, self.finger, self.centers.data_ptr(),
                  self.radii.data_ptr(), self.links.data_ptr(), self.num_spheres, *points, float(clearance), _lib.ptr(ac),
                  hit.data_ptr())
        return hit != 0
