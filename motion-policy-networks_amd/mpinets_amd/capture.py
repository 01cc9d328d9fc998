"""Cleaning of captured point clouds on the device: crop, robot removal, outlier removal, draw (csrc/cloud_clean.hip).

The reference's real-robot planner (``interactive_demo/mpinets_ros/nodes/planning_node.py:78-151``) asserts that the
obstacle cloud it is given is already ``[4096, 3]``: "You must downsample obstacle PC before passing to planner. While
you're at it, filter the outliers out as well".  Its own ``clean_point_cloud`` (``:187-228``) crops the capture to two
workspace boxes and draws 4096 rows with ``np.random.choice`` on the host; removing the robot's own points and the
outliers is left to the reader.  ``clean_point_clouds`` does all four for a batch of captures with one call of
``mpx_cloud_clean``; ``clean_point_cloud`` keeps the reference's signature.

Every row gets a ``reason``: 0 kept, 1 non-existent / non-finite, 2 outside the workspace, 3 robot, 4 outlier -- the
first stage it fails (include/mpinets_hip.h has the arithmetic of each).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._operands import cloud_operand, counts_operand, scratch_for
from .robot import FrankaCollisionSampler
from .solvers import franka_follow_cloud, franka_ik_cloud, franka_plan_cloud, franka_plan_global_cloud

# planning_node.py:201-221: the task table and the mount table, rows of (lo x, lo y, lo z, hi x, hi y, hi z); a point is
# inside when it is STRICTLY inside one of them
REFERENCE_WORKSPACE = np.array([[0.25, -0.3, -0.05, 1.35, 1.6, 0.35],
                                [-0.35, -0.5, -0.05, 0.30, 0.5, 0.05]], dtype=np.float32)
REASONS = ("kept", "non-existent or non-finite", "outside the workspace", "robot", "outlier")
MAX_POINTS = 4096  # SEL_MAX_OUT: what one workgroup's select can draw

_samplers: Dict[int, FrankaCollisionSampler] = {}
_boxes: Dict[Tuple[int, bytes], torch.Tensor] = {}


def _boxes_on(device: torch.device, boxes) -> Tuple[Optional[torch.Tensor], int]:
    if boxes is None:
        return None, 0
    if isinstance(boxes, torch.Tensor):
        t = _lib.f32c(boxes.to(device))
    else:
        a = np.ascontiguousarray(boxes, dtype=np.float32)
        key = (device.index, a.tobytes())
        t = _boxes.get(key)
        if t is None:
            if len(_boxes) > 64:
                _boxes.clear()
            t = _boxes[key] = torch.from_numpy(a.copy()).to(device)
    if t.ndim != 2 or t.size(1) != 6:
        raise _lib.MpxError(f"clean_point_clouds: boxes must be [n, 6] (lo xyz, hi xyz), got {tuple(t.shape)}")
    return (t, t.size(0)) if t.size(0) else (None, 0)


@torch.no_grad()
def clean_point_clouds(cloud: torch.Tensor, num_points: int = 4096, *, counts: Optional[torch.Tensor] = None,
                       boxes=REFERENCE_WORKSPACE, q: Optional[torch.Tensor] = None,
                       collision_sampler: Optional[FrankaCollisionSampler] = None, robot_margin: float = 0.0,
                       outlier_radius: float = 0.0, min_neighbors: int = 0, seed: int = 0, env_offset: int = 0,
                       out: Optional[torch.Tensor] = None, return_index: bool = False, return_reason: bool = False):
    """Crop, remove the robot, remove outliers and draw ``num_points`` rows of every captured cloud.

    :param cloud: float32 [B,N,3] or [B,N,4] on the GPU; any view whose last stride is 1 is read in place
    :param counts: optional int [B]: only the first ``counts[b]`` rows of environment b exist (clamped to [0, N])
    :param boxes: [n,6] (lo xyz, hi xyz), n <= 8, shared by the batch: a row is kept when it is strictly inside one of them.
        ``None``: no crop.  Default: the reference's two workspace boxes
    :param q: [B,7] joint angles at capture time: rows within ``radius + robot_margin`` of a collision sphere's centre
        are removed.  ``collision_sampler`` defaults to ``FrankaCollisionSampler(device, with_base_link=True)`` -- a
        capture shows the base.  A ``robot_margin`` above ``point_radius + clearance`` of a later ``check_cloud`` with the
        same sampler makes the cleaned cloud free of hits at ``q`` by construction
    :param outlier_radius, min_neighbors: a row is kept when at least ``min_neighbors`` OTHER rows that passed the crop
        and the robot stage lie within ``outlier_radius`` of it (one pass).  ``min_neighbors=0``: off
    :param seed, env_offset: row b draws as global environment ``env_offset + b`` (sharded batches)
    :param out: where to write, e.g. the slab's scene rows ``xyz[:, 2048:6144]``: only columns 0-2 of its first
        ``num_points`` rows are written
    :returns: ``[B,num_points,3]``, a uniform subset of the kept rows in uniform order; then ``src_index`` int32
        ``[B,num_points]`` (the rows' indices in ``cloud``) when ``return_index`` and ``reason`` uint8 ``[B,N]`` when
        ``return_reason``.  ``num_points=0`` filters only and returns ``(reason, counts)``.  The kept rows per environment
        stay in ``clean_point_clouds.last_counts``.
    :raises ValueError: like ``np.random.choice`` when an environment keeps fewer than ``num_points`` rows
    """
    _lib.require_cuda(cloud, counts, q, out)
    N, cbs, ps = cloud_operand("clean_point_clouds", cloud, empty_batch_any_stride=False)
    B, dev = cloud.size(0), cloud.device
    num_points = int(num_points)
    if not 0 <= num_points <= MAX_POINTS:
        raise _lib.MpxError(f"clean_point_clouds: num_points must be in [0, {MAX_POINTS}], got {num_points}")
    cn = counts_operand(counts, B)
    bx, n_boxes = _boxes_on(dev, boxes)
    sc = sr = None
    S = 0
    if q is not None:
        cs = collision_sampler
        if cs is None:
            cs = _samplers.get(dev.index)
            if cs is None:
                cs = _samplers[dev.index] = FrankaCollisionSampler(dev, with_base_link=True)
        assert q.shape == (B, 7)
        sc, sr, S = cs.sphere_centers(q), cs.radii, cs.num_spheres
    obs = ops = 0
    if num_points > 0:
        if out is None:
            out = torch.empty((B, num_points, 3), dtype=torch.float32, device=dev)
        assert out.dtype == torch.float32 and out.size(0) == B and out.size(1) >= num_points and out.size(2) >= 3
        assert out.stride(2) == 1
        obs, ops = out.stride(0), out.stride(1) if out.size(1) > 1 else max(out.stride(1), 3)
    want_reason = return_reason or num_points == 0
    reason = torch.empty((B, N), dtype=torch.uint8, device=dev) if want_reason else None
    index = torch.empty((B, num_points), dtype=torch.int32, device=dev) if return_index and num_points > 0 else None
    count = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = int(_lib.load().mpx_cloud_clean_scratch(B, N))
    scratch = scratch_for(dev, nbytes)
    _lib.call("mpx_cloud_clean", _lib.ptr(cloud), cbs, ps, N, _lib.ptr(cn), B, _lib.ptr(bx), n_boxes,
              _lib.ptr(sc), _lib.ptr(sr), S, float(robot_margin), float(outlier_radius), int(min_neighbors), num_points,
              int(seed) & (2 ** 64 - 1), int(env_offset), _lib.ptr(out) if num_points else None, obs, ops, _lib.ptr(index),
              _lib.ptr(reason), _lib.ptr(count), _lib.ptr(scratch), nbytes)
    clean_point_clouds.last_counts = count
    if num_points == 0:
        return reason, count
    if B > 0:
        host = count.cpu()
        b = int(host.argmin().item())
        if int(host[b].item()) < num_points:
            raise ValueError("Cannot take a larger sample than population when 'replace=False' "
                             f"(environment {b} keeps {int(host[b].item())} of its rows, {num_points} requested)")
    res = (out[:, :num_points, :3],) + ((index,) if return_index else ()) + ((reason,) if return_reason else ())
    return res if len(res) > 1 else res[0]


clean_point_clouds.last_counts = None


def clean_point_cloud(xyz: np.ndarray, rgba: np.ndarray, **kw) -> Tuple[np.ndarray, np.ndarray]:
    """The reference's ``clean_point_cloud(xyz, rgba)`` (planning_node.py:187-228): NumPy ``[N,3]`` and ``[N,4]`` ->
    ``(xyz [num_points,3], rgba [num_points,4])``.  With its defaults it is the reference's crop to the two workspace
    boxes and the draw of 4096 rows without replacement; every keyword of ``clean_point_clouds`` is passed on (``q`` as
    ``[7]`` or ``[1,7]``).  The subset is drawn on the device from ``seed`` (the reference uses NumPy's global state)."""
    if not torch.cuda.is_available():
        raise _lib.MpxError("clean_point_cloud needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    pts = np.ascontiguousarray(xyz, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3 or len(rgba) != len(pts):
        raise ValueError(f"clean_point_cloud: xyz must be [N,3] and rgba [N,...], got {pts.shape} and {np.shape(rgba)}")
    for bad in ("out", "return_index", "return_reason", "counts"):
        if bad in kw:
            raise TypeError(f"clean_point_cloud() takes no {bad!r}: use clean_point_clouds")
    if kw.get("q") is not None:
        kw["q"] = torch.as_tensor(np.asarray(kw["q"], dtype=np.float32).reshape(1, 7)).to(dev)
    cloud = torch.from_numpy(pts).to(dev).unsqueeze(0)
    got, index = clean_point_clouds(cloud, kw.pop("num_points", 4096), return_index=True, **kw)
    index = index[0].cpu().numpy()
    return got[0].cpu().numpy(), np.asarray(rgba)[index]


@torch.no_grad()
def plan_to_poses(cloud: torch.Tensor, q_start: torch.Tensor, target_poses: torch.Tensor, *,
                  counts: Optional[torch.Tensor] = None, point_radius: float = 0.0, T: int = 50, seed: int = 0,
                  env_offset: int = 0, field=None, ik_options: Optional[dict] = None,
                  plan_options: Optional[dict] = None, global_plan: bool = False,
                  roadmap_options: Optional[dict] = None, follow: bool = False, follow_poses: int = 8,
                  follow_options: Optional[dict] = None, follow_guide: str = "plan",
                  gripper_options: Optional[dict] = None, shortcut=False, follow_shortcut=False) -> dict:
    """From a cloud and a target pose to a checked trajectory: ``robot.franka_ik_cloud`` for the goal configuration, then
    ``robot.franka_plan_cloud`` from ``q_start`` to it, both against the same ``cloud`` (``counts``, ``point_radius``).  The
    optimiser-based counterpart of the reference demo's ``Planner.plan(q0, target_pose, obstacle_pc)``
    (``interactive_demo/mpinets_ros/nodes/planning_node.py``), for a batch.

    :param cloud: [B,N,3] or [B,N,4] float32 on the GPU (e.g. what ``clean_point_clouds`` returns, or the slab's scene rows)
    :param q_start: [B,7];  :param target_poses: [B,4,4] right_gripper poses
    :param field: a ``CloudField`` of the cloud for the planner, or None (built there)
    :param ik_options, plan_options: keyword options of the two calls (``franka_ik_cloud`` / ``franka_plan_cloud``)
    :param global_plan: False (every key and bit as before), or True: the trajectory comes from
        ``robot.franka_plan_global_cloud`` -- a lazy roadmap through the cloud's distance field seeds one more candidate, so a
        target behind an obstacle is not lost to a blocked straight line; ``roadmap_options`` are that roadmap's
    :param shortcut: False (as before), or True / a dict of ``robot.franka_shortcut_cloud``'s options (needs
        ``global_plan``): the roadmap's path is shortcut through the same field and seeds one candidate more, in front of
        the roadmap's own (``franka_plan_global_cloud(shortcut=...)``)
    :returns: dict of ``q_goal`` [B,7] (NaN rows where ``ik_status`` != 0), ``ik_status`` int32 [B], ``trajectory``
        [B,T,7] (NaN rows where ``plan_status`` != 0), ``plan_status`` int32 [B] -- 2 for every row without a goal: the
        planner refuses a NaN endpoint -- and ``valid`` bool [B]: both statuses 0; with ``global_plan`` also ``roadmap_status``
        int32 [B] (``franka_roadmap_cloud``'s).
    :param follow: False (what is returned is what it was), or True: the plan's right_gripper poses at ``follow_poses``
        waypoints (round(i (T-1) / W), i = 1..W) are also followed from ``q_start`` by ``robot.franka_follow_cloud`` -- the
        stand-in reactive controller, NOT Geometric Fabrics -- against the same cloud, counts, ``point_radius`` and ONE field
        (built here when ``field`` is None and shared with the planner); ``follow_options`` are its keyword options.  Adds
        ``followed_trajectory`` [B,T,7] (NaN rows where ``follow_status`` != 0), ``follow_status`` int32 [B] (2 for every row
        without a plan: its guide is NaN), ``follow_bits`` and ``follow_steps`` int32 [B].  The same call with
        ``max_steps`` and the returned state of ``franka_follow_cloud`` is the controller stepped against that cloud.
    :param follow_guide: "plan" (every key and bit as before: the follower's guide is read off the plan), or "gripper"
        (needs ``follow``): the guide is ``robot.gripper_roadmap_cloud``'s -- a roadmap for the free-flying gripper through
        the cloud's distance field, a stand-in for the reference's OMPL end-effector planner, NOT a port -- from the
        right_gripper pose of ``q_start`` to that of ``q_goal``, at ``follow_poses`` poses, against the same cloud, counts,
        ``point_radius`` and the one shared field, keyed by ``seed`` / ``env_offset``; ``gripper_options`` are its keyword
        options (``field_slack`` among them).  A row without an IK goal has a NaN goal pose and gets status 2.  Adds
        ``follow_guide_poses`` [B,W,4,4] (NaN rows without a path) and ``follow_guide_status`` int32 [B].  The guide no longer
        needs the optimiser: a row whose plan failed but whose IK succeeded can come back with a ``followed_trajectory``
        (``follow_status`` 0, free by ``check_cloud``'s test); ``valid`` keeps its meaning (both the IK and the plan).
    :param follow_shortcut: False (every key and bit as before), or True / a dict of ``robot.gripper_shortcut_cloud``'s
        options (needs ``follow_guide="gripper"``): the gripper roadmap's path is shortcut on the device through the same
        field (``robot.gripper_plan_cloud``) before it is resampled; ``follow_guide_poses`` are then the shortcut's,
        ``follow_guide_status`` stays the roadmap's."""
    if follow_guide not in ("plan", "gripper"):
        raise ValueError(f"follow_guide must be 'plan' or 'gripper', got {follow_guide!r}")
    if follow_guide == "gripper" and not follow:
        raise ValueError("follow_guide='gripper' chooses the follower's guide: it needs follow=True")
    if follow_shortcut and follow_guide != "gripper":
        raise ValueError("follow_shortcut shortens the gripper roadmap's path: it needs follow_guide='gripper'")
    if shortcut and not global_plan:
        raise ValueError("shortcut shortens the roadmap's path: it needs global_plan=True")
    if follow and field is None:  # (one field for the planner and the follower)
        from ._operands import cloud_args
        from .field import DEFAULT_VOXEL, CloudField
        from .solvers import FOLLOW_DEFAULTS, PLAN_DEFAULTS, plan_cloud_truncation

        eps = max(float((plan_options or {}).get("epsilon", PLAN_DEFAULTS["epsilon"])),
                  float((follow_options or {}).get("epsilon", FOLLOW_DEFAULTS["epsilon"])))
        clr = max(float((plan_options or {}).get("clearance", 0.0)), float((follow_options or {}).get("clearance", 0.0)))
        _, cn = cloud_args("plan_to_poses", cloud, counts, q_start.size(0), point_radius)
        field = CloudField.build(cloud, cn, truncation=plan_cloud_truncation(point_radius, clr, eps, DEFAULT_VOXEL))
    q_goal, ik_status = franka_ik_cloud(target_poses, cloud, counts, point_radius, seed=seed, env_offset=env_offset,
                                        **(ik_options or {}))
    extra = {}
    if global_plan:
        traj, plan_status, extra["roadmap_status"] = franka_plan_global_cloud(
            q_start, q_goal, cloud, counts, field=field, point_radius=point_radius, T=T, seed=seed, env_offset=env_offset,
            roadmap=roadmap_options, shortcut=shortcut or None, **(plan_options or {}))
    else:
        traj, plan_status = franka_plan_cloud(q_start, q_goal, cloud, counts, field=field, point_radius=point_radius, T=T,
                                              seed=seed, env_offset=env_offset, **(plan_options or {}))
    if follow:
        from . import franka_tables as ft
        from .robot import franka_fk, frames_to_matrix

        B, W = q_start.size(0), int(follow_poses)
        at = [int(round(i * (int(T) - 1) / W)) for i in range(1, W + 1)]
        gripper = ft.LINK_ID["right_gripper"]
        if follow_guide == "gripper":
            from .solvers import gripper_plan_cloud, gripper_roadmap_cloud

            ends = frames_to_matrix(franka_fk(torch.cat([q_start, q_goal]))[:, gripper])  # (a row without a goal: NaN, status 2)
            if follow_shortcut:
                ropt = dict(gripper_options or {})
                guide, extra["follow_guide_status"] = gripper_plan_cloud(
                    ends[:B].contiguous(), ends[B:].contiguous(), cloud, counts, field=field, point_radius=point_radius,
                    field_slack=ropt.pop("field_slack", 0.0), W=W, seed=seed, env_offset=env_offset, roadmap=ropt,
                    shortcut=follow_shortcut)
            else:
                guide, extra["follow_guide_status"] = gripper_roadmap_cloud(
                    ends[:B].contiguous(), ends[B:].contiguous(), cloud, counts, field=field, point_radius=point_radius, W=W,
                    seed=seed, env_offset=env_offset, **(gripper_options or {}))
            extra["follow_guide_poses"] = guide
        else:
            guide = frames_to_matrix(franka_fk(traj[:, at].reshape(-1, 7))[:, gripper]).reshape(B, W, 4, 4)
        extra["followed_trajectory"], extra["follow_status"], extra["follow_bits"], extra["follow_steps"] = franka_follow_cloud(
            q_start, guide, cloud, counts, field=field, point_radius=point_radius, T=T, **(follow_options or {}))
    return dict({"q_goal": q_goal, "ik_status": ik_status, "trajectory": traj, "plan_status": plan_status,
                 "valid": (ik_status == 0) & (plan_status == 0)}, **extra)
