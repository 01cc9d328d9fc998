"""Time collision-free IK against point clouds (``robot.franka_ik_cloud``) and the per-waypoint cloud check under it
(``FrankaCollisionSampler.check_cloud_each``) on the GPU, next to what stood there before.

For B in --envs (default 1 64 1024 8192) mixed tabletop / cubby / dresser scenes (M1 = 40, M2 = 16), their 4096-point
scene clouds read in place from the slab, the drawn target poses of ``make_problem_batch``, ``point_radius`` = half the
clouds' mean nearest-neighbour spacing:

  * ``franka_ik`` in free space (self test on) and against the primitives the clouds were drawn from;
  * ``franka_ik_cloud`` with and without ``return_all``;
  * ``check_cloud_each`` alone on the solver's ``[B,64,7]`` starts -- every start, and ``active`` = converged as the IK
    calls it -- and on ``[B,50,7]`` straight-line trajectories, next to flags-only ``check_cloud`` on the same
    trajectories (each with the bounding-box cull, the default);
  * the BASELINE for the new IK, the composition a user could write before it: ``franka_ik(return_all=True)``, 64
    ``check_cloud`` calls (one per start, on one transposed copy of the starts), the pick with torch on the device.
    Timed in the same loop as ``franka_ik_cloud(return_all=True)``, alternating; their results are compared bit for bit;
  * solved shares against the cloud and against the primitives.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as
tools/cloud_plan_timing.py.  The timed calls are the Python entry points as a user makes them (wrapper host work included).

    python tools/ik_cloud_timing.py [--envs 1 64 1024 8192]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ik_timing import timed  # noqa: E402

MIXED = ("tabletop", "cubby", "dresser")


def timed_alternating(fns, warm=3, reps=10):
    """Like ``timed`` for several callables measured in one loop, one after the other within every repetition."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v), "reps": reps} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 64, 1024, 8192])
    args = ap.parse_args()
    from mpinets_amd import robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders
    from mpinets_amd.robot import FrankaCollisionSampler

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    res = {"options": dict(robot.IK_DEFAULTS, check_self=True), "cases": {}}
    sampler = FrankaCollisionSampler(dev)
    for B in args.envs:
        prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        poses = prob["target_pose"]
        cloud = prob["xyz"][:, 2048:6144, :3]
        few = cloud[:min(B, 8)].contiguous()
        d = torch.cdist(few, few)
        d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
        spacing = float(d.amin(-1).mean())
        pr = 0.5 * spacing
        out = {"mean_nearest_neighbour_spacing_m": spacing, "point_radius_m": pr}

        def baseline():
            q, st, aq, ast = robot.franka_ik(poses, return_all=True, check_self=True)
            starts = aq.transpose(0, 1).contiguous()  # [64,B,7]
            hit = torch.stack([sampler.check_cloud(starts[s], cloud, point_radius=pr) for s in range(robot.IK_SEEDS)], 1)
            conv = (ast & 1) != 0
            bits = ast | ((hit & conv).int() << 1)
            free = bits == 1
            winner = free.int().argmax(1)
            found = free.any(1)
            qw = aq[torch.arange(B, device=dev), winner]
            q = torch.where(found[:, None], qw, torch.full_like(qw, float("nan")))
            status = torch.where(found, 0, torch.where(conv.any(1), 1, 2)).int()
            return q, status, aq, bits

        new = lambda: robot.franka_ik_cloud(poses, cloud, point_radius=pr, return_all=True)  # noqa: E731
        a, b = baseline(), new()
        out["baseline_equals_new"] = all(torch.equal(torch.nan_to_num(x.float(), nan=-9.0), torch.nan_to_num(y.float(), nan=-9.0))
                                         for x, y in zip(a, b))
        out.update(timed_alternating({"baseline_ik_64_check_cloud_pick": baseline, "ik_cloud_return_all": new}))
        out["baseline_over_new"] = out["baseline_ik_64_check_cloud_pick"]["median_ms"] / out["ik_cloud_return_all"]["median_ms"]
        out["ik_cloud"] = timed(lambda: robot.franka_ik_cloud(poses, cloud, point_radius=pr))
        out["ik_free_space"] = timed(lambda: robot.franka_ik(poses, check_self=True))
        out["ik_free_space_return_all"] = timed(lambda: robot.franka_ik(poses, check_self=True, return_all=True))
        out["ik_primitives"] = timed(lambda: robot.franka_ik(poses, cub, cyl))
        q, st, aq, ast = b
        conv = (ast & 1) != 0
        out["converged_share_of_starts"] = float(conv.float().mean())
        out["cloud_hit_share_of_converged_starts"] = float(((ast & 2) != 0)[conv].float().mean()) if bool(conv.any()) else None
        out["each_on_B_64_all_starts"] = timed(lambda: sampler.check_cloud_each(aq, cloud, point_radius=pr))
        out["each_on_B_64_active_converged"] = timed(lambda: sampler.check_cloud_each(aq, cloud, point_radius=pr, active=conv))
        traj = torch.from_numpy(scenes.linear_trajectories(B, 50, 1)).to(dev)
        out["each_on_B_50"] = timed(lambda: sampler.check_cloud_each(traj, cloud, point_radius=pr))
        out["flags_on_B_50"] = timed(lambda: sampler.check_cloud(traj, cloud, point_radius=pr))
        out["waypoints_hit_share_B_50"] = float(sampler.check_cloud_each(traj, cloud, point_radius=pr).float().mean())
        out["share_solved_cloud"] = float((st == 0).float().mean())
        out["share_solved_primitives"] = float((robot.franka_ik(poses, cub, cyl)[1] == 0).float().mean())
        out["share_solved_free_space"] = float((robot.franka_ik(poses, check_self=True)[1] == 0).float().mean())
        res["cases"][str(B)] = out
        print(json.dumps({str(B): out}), file=sys.stderr, flush=True)
        del prob
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
