"""Time the gripper's SE(3) roadmap (csrc/gripper_roadmap.hip, ``robot.gripper_roadmap``) on the GPU, and record what it does
to the hybrid expert, on the inputs of tools/follow_timing.py.

For B in --envs (default 8192) mixed tabletop / cubby / dresser problems (M1 = 40, M2 = 16, start and goal posed by
``make_problem_batch(collision_free=True)``):

  * ``robot.gripper_roadmap`` (W = 8, defaults) from the right_gripper pose of ``q`` to that of ``q_goal``: milliseconds per
    call, the status, hops and rounds histograms;
  * ``robot.franka_roadmap`` (T = 50, defaults) on the same rows, for context;
  * ``robot.franka_plan_global`` and ``robot.franka_follow`` along the GLOBAL guide (eight waypoints of the plan, as
    ``make_problem_batch(hybrid=True)`` builds it) and along the GRIPPER guide (the roadmap's poses): the follower's status
    split and the ``hybrid_valid`` share (planned and followed and valid) under both, on the same batch.

The planner is a stand-in for the reference's OMPL end-effector planner, not a port: the numbers say what this roadmap costs
and finds, nothing about AIT*.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as tools/roadmap_timing.py.
The timed calls are the Python entry points as a user makes them (wrapper host work and output allocations included).
The kernel's register and LDS figures are read from the built library's code object (tests/test_code_objects.py's reader).

    python tools/gripper_roadmap_timing.py [--envs 8192]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from ik_timing import timed  # noqa: E402

MIXED = ("tabletop", "cubby", "dresser")


def kernel_figures():
    from test_code_objects import LIB, kernel_metadata

    (f,) = [f for n, f in kernel_metadata(LIB).items() if "gripper_roadmap_kernel" in n]
    return {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                               ".private_segment_fixed_size", ".group_segment_fixed_size")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192])
    args = ap.parse_args()
    from mpinets_amd import franka_tables as ft, robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    torch.cuda.set_device(0)
    W = scenes.HYBRID_GUIDE_POSES
    res = {"options": dict(robot.GRIPPER_ROADMAP_DEFAULTS, connect_radius="inf"), "W": W, "kernel": kernel_figures(), "cases": {}}
    gripper = ft.LINK_ID["right_gripper"]

    def hist(x, n=0):
        return torch.bincount(x.long(), minlength=n).tolist()

    for B in args.envs:
        prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True,
                                         collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        qs, qg, posed = prob["q"], prob["q_goal"], prob["valid"]  # (unposed rows have a NaN goal: status 2 in every entry)
        ends = robot.frames_to_matrix(robot.franka_fk(torch.cat([qs, qg]))[:, gripper])
        sp, gp = ends[:B].contiguous(), ends[B:].contiguous()
        out = {"posed": int(posed.sum())}
        out["gripper_roadmap"] = timed(lambda: robot.gripper_roadmap(sp, gp, cub, cyl, W=W))
        poses, gst, _, hops, _, _, rounds = robot.gripper_roadmap(sp, gp, cub, cyl, W=W, return_graph=True)
        found = posed & (gst == 0)
        out["gripper_roadmap"].update(status_0_1_2=hist(gst[posed], 3), hops=hist(hops[found]), rounds=hist(rounds[posed]),
                                      rounds_mean=float(rounds[posed].float().mean()), rounds_max=int(rounds[posed].max()),
                                      out_of_rounds=int((posed & (gst == 1) & (rounds == robot.GRIPPER_ROADMAP_DEFAULTS["max_rounds"])).sum()),
                                      share_found=float(found.sum() / posed.sum()))
        out["franka_roadmap"] = timed(lambda: robot.franka_roadmap(qs, qg, cub, cyl))
        rst = robot.franka_roadmap(qs, qg, cub, cyl)[1]
        out["franka_roadmap"].update(status_0_1_2=hist(rst[posed], 3), share_found=float((posed & (rst == 0)).sum() / posed.sum()))
        plan, st = robot.franka_plan_global(qs, qg, cub, cyl)[:2]
        planned = st == 0
        out["planned"] = int(planned.sum())
        at = [int(round(i * 49 / W)) for i in range(1, W + 1)]
        guide = robot.frames_to_matrix(robot.franka_fk(plan[:, at].reshape(-1, 7))[:, gripper]).reshape(B, W, 4, 4)
        for name, g in (("global", guide), ("gripper", poses)):
            _, fst, bits, steps = robot.franka_follow(qs, g, cub, cyl)
            valid = planned & (fst == 0)
            out[f"follow_{name}_guide"] = dict(status_0_1_2=hist(fst, 3), bits=hist(bits, 16), hybrid_valid=int(valid.sum()),
                                               hybrid_valid_share_of_planned=float(valid.sum() / planned.sum()),
                                               steps_mean=float(steps[fst != 2].float().mean()))
            out[f"follow_{name}_guide"]["valid_rows"] = valid
        a, b = out["follow_global_guide"].pop("valid_rows"), out["follow_gripper_guide"].pop("valid_rows")
        out["hybrid_valid_both_only_global_only_gripper"] = [int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum())]
        out["planned_rows_without_a_gripper_path"] = int((planned & (gst != 0)).sum())
        res["cases"][str(B)] = out
        del prob
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
