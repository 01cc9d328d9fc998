"""Time the gripper's SE(3) roadmap against point clouds (csrc/gripper_roadmap_cloud.hip, ``robot.gripper_roadmap_cloud``) on
the GPU beside the primitive form, and record what it does to the cloud hybrid expert, on the inputs of
tools/gripper_roadmap_timing.py.

For B in --envs (default 8192) mixed tabletop / cubby / dresser problems (M1 = 40, M2 = 16, start and goal posed by
``make_problem_batch(collision_free=True)``), the cloud being the slab's own scene rows at the expert's point radius:

  * ``CloudField.build`` of those rows on the default grid: milliseconds per call, timed on its own;
  * ``robot.gripper_roadmap_cloud`` (W = 8, defaults, that ONE prebuilt field) and ``robot.gripper_roadmap`` (the primitives
    of the same rows), from the right_gripper pose of ``q`` to that of ``q_goal``: milliseconds per call, the two entries
    ALTERNATING in one process, and the status, hops and rounds histograms of both;
  * ``robot.franka_plan_global_cloud`` and ``robot.franka_follow_cloud`` along the GLOBAL guide (eight waypoints of the cloud
    plan, as ``make_problem_batch(hybrid=True, hybrid_against="cloud")`` builds it) and along the GRIPPER_CLOUD guide (the
    roadmap's poses): the follower's status split and the ``hybrid_valid`` share under both, on the same batch.

The planner is a stand-in for the reference's OMPL end-effector planner, not a port: the numbers say what this roadmap costs
and finds, nothing about AIT*.  There is no pass bar: the cloud form is a new capability and the primitive form is context.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as
tools/gripper_roadmap_timing.py.  The timed calls are the Python entry points as a user makes them (wrapper host work and
output allocations included).  The kernels' register and LDS figures are read from the built library's code object
(tests/test_code_objects.py's reader).

    python tools/gripper_roadmap_cloud_timing.py [--envs 8192]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from ik_timing import timed  # noqa: E402

MIXED = ("tabletop", "cubby", "dresser")
WARMUP, REPEATS = 3, 10


def kernel_figures():
    from test_code_objects import LIB, kernel_metadata

    out = {}
    for key in ("gripper_roadmap_cloud_kernel", "gripper_roadmap_kernel"):
        (f,) = [f for n, f in kernel_metadata(LIB).items() if key in n]
        out[key] = {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                                      ".private_segment_fixed_size", ".group_segment_fixed_size")}
    return out


def alternating(calls):
    """name -> thunk, each timed with HIP events, the thunks taking turns: WARMUP untimed rounds, then REPEATS timed ones ->
    name -> dict(ms_median, ms_min, ms_max)."""
    for _ in range(WARMUP):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(REPEATS):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: dict(ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v)) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192])
    args = ap.parse_args()
    from mpinets_amd import franka_tables as ft, robot, scenes
    from mpinets_amd.field import DEFAULT_VOXEL, CloudField
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    torch.cuda.set_device(0)
    W, pr = scenes.HYBRID_GUIDE_POSES, scenes.EXPERT_CLOUD_POINT_RADIUS
    res = {"options": dict(robot.GRIPPER_ROADMAP_DEFAULTS, connect_radius="inf"), "W": W, "point_radius": pr,
           "kernels": kernel_figures(), "cases": {}}
    gripper = ft.LINK_ID["right_gripper"]
    max_rounds = robot.GRIPPER_ROADMAP_DEFAULTS["max_rounds"]

    def hist(x, n=0):
        return torch.bincount(x.long(), minlength=n).tolist()

    def graph_figures(gst, hops, rounds, posed):
        found = posed & (gst == 0)
        return dict(status_0_1_2=hist(gst[posed], 3), hops=hist(hops[found]), rounds=hist(rounds[posed]),
                    rounds_mean=float(rounds[posed].float().mean()), rounds_max=int(rounds[posed].max()),
                    out_of_rounds=int((posed & (gst == 1) & (rounds == max_rounds)).sum()),
                    share_found=float(found.sum() / posed.sum()))

    for B in args.envs:
        prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True,
                                         collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        cloud = prob["xyz"][:, 2048:6144, :3]  # the slab's own scene rows, read in place
        qs, qg, posed = prob["q"], prob["q_goal"], prob["valid"]  # (unposed rows have a NaN goal: status 2 in every entry)
        ends = robot.frames_to_matrix(robot.franka_fk(torch.cat([qs, qg]))[:, gripper])
        sp, gp = ends[:B].contiguous(), ends[B:].contiguous()
        trunc = robot.plan_cloud_truncation(pr, robot.FOLLOW_DEFAULTS["clearance"], robot.FOLLOW_DEFAULTS["epsilon"], DEFAULT_VOXEL)
        field = CloudField.build(cloud, None, truncation=trunc)
        out = {"posed": int(posed.sum()), "field_nodes": int(field.values[0].numel()), "truncation": trunc}
        out["field_build"] = timed(lambda: CloudField.build(cloud, None, truncation=trunc, out=field.values))
        both = alternating({"gripper_roadmap_cloud": lambda: robot.gripper_roadmap_cloud(sp, gp, cloud, field=field, point_radius=pr, W=W),
                            "gripper_roadmap": lambda: robot.gripper_roadmap(sp, gp, cub, cyl, W=W)})
        poses, gst, _, hops, _, _, rounds = robot.gripper_roadmap_cloud(sp, gp, cloud, field=field, point_radius=pr, W=W,
                                                                        return_graph=True)
        out["gripper_roadmap_cloud"] = dict(both["gripper_roadmap_cloud"], **graph_figures(gst, hops, rounds, posed))
        _, pst, _, phops, _, _, prounds = robot.gripper_roadmap(sp, gp, cub, cyl, W=W, return_graph=True)
        out["gripper_roadmap"] = dict(both["gripper_roadmap"], **graph_figures(pst, phops, prounds, posed))
        out["status_cloud_rows_by_primitive_columns"] = [[int((posed & (gst == i) & (pst == j)).sum()) for j in range(3)] for i in range(3)]
        plan, st = robot.franka_plan_global_cloud(qs, qg, cloud, field=field, point_radius=pr)[:2]
        planned = st == 0
        out["planned"] = int(planned.sum())
        at = [int(round(i * 49 / W)) for i in range(1, W + 1)]
        guide = robot.frames_to_matrix(robot.franka_fk(plan[:, at].reshape(-1, 7))[:, gripper]).reshape(B, W, 4, 4)
        valid = {}
        for name, g in (("global", guide), ("gripper_cloud", poses)):
            _, fst, bits, steps = robot.franka_follow_cloud(qs, g, cloud, field=field, point_radius=pr)
            valid[name] = planned & (fst == 0)
            out[f"follow_{name}_guide"] = dict(status_0_1_2=hist(fst, 3), bits=hist(bits, 16), hybrid_valid=int(valid[name].sum()),
                                               hybrid_valid_share_of_planned=float(valid[name].sum() / planned.sum()),
                                               followed_and_valid_without_a_plan=int((~planned & posed & (fst == 0)).sum()),
                                               steps_mean=float(steps[fst != 2].float().mean()))
        a, b = valid["global"], valid["gripper_cloud"]
        out["hybrid_valid_both_only_global_only_gripper_cloud"] = [int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum())]
        out["planned_rows_without_a_gripper_path"] = int((planned & (gst != 0)).sum())
        res["cases"][str(B)] = out
        del prob, field
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
