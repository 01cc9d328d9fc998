"""Time the path follower (csrc/follow.hip, ``robot.franka_follow``) on the GPU next to the planner that steers it.

For B in --envs (default 8192) mixed tabletop / cubby / dresser problems (M1 = 40, M2 = 16, start and goal posed by
``make_problem_batch(collision_free=True)``):

  * ``robot.franka_plan_global`` (T = 50, defaults) on the batch: the global plan, timed for context;
  * the guide: the right_gripper poses of waypoints round(i * 49 / 8), i = 1..8, of that plan (W = 8), as
    ``make_problem_batch(hybrid=True)`` builds it; rows without a plan hand NaN poses and come back with status 2;
  * ``robot.franka_follow`` (T = 50, defaults: at most 1024 steps) on those guides: milliseconds per call, mean steps per
    row over the rows that ran, steps per second, the status and bits histograms, the valid share over the planned rows.

The follower is a stand-in for the reference's Geometric Fabrics expert, not Lula: the numbers say what this controller
costs, nothing about the fabric.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as tools/plan_timing.py.
The timed calls are the Python entry points as a user makes them (wrapper host work and output allocations included).
The kernel's register and LDS figures are read from the built library's code object (tests/test_code_objects.py's reader).

    python tools/follow_timing.py [--envs 8192]
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

    (f,) = [f for n, f in kernel_metadata(LIB).items() if "franka_follow_kernel" in n]
    return {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                               ".private_segment_fixed_size", ".group_segment_fixed_size")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192])
    args = ap.parse_args()
    from mpinets_amd import franka_tables as ft, robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    torch.cuda.set_device(0)
    res = {"options": robot.FOLLOW_DEFAULTS, "T": 50, "W": scenes.HYBRID_GUIDE_POSES, "kernel": kernel_figures(), "cases": {}}
    gripper = ft.LINK_ID["right_gripper"]
    for B in args.envs:
        prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True,
                                         collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        qs, qg = prob["q"], prob["q_goal"]  # (unposed rows have a NaN goal: status 2 in both entries)
        out = {"posed": int(prob["valid"].sum())}
        out["plan_global"] = timed(lambda: robot.franka_plan_global(qs, qg, cub, cyl))
        plan, st = robot.franka_plan_global(qs, qg, cub, cyl)[:2]
        planned = st == 0
        out["planned"] = int(planned.sum())
        at = [int(round(i * 49 / scenes.HYBRID_GUIDE_POSES)) for i in range(1, scenes.HYBRID_GUIDE_POSES + 1)]
        guide = robot.frames_to_matrix(robot.franka_fk(plan[:, at].reshape(-1, 7))[:, gripper]).reshape(B, len(at), 4, 4)
        out["follow"] = timed(lambda: robot.franka_follow(qs, guide, cub, cyl))
        _, status, bits, steps = robot.franka_follow(qs, guide, cub, cyl)
        ran = status != 2
        total = int(steps.sum())
        out["steps_mean_over_rows_that_ran"] = total / max(int(ran.sum()), 1)
        out["steps_max"] = int(steps.max()) if B else 0
        out["rows_at_max_steps"] = int((steps == robot.FOLLOW_DEFAULTS["max_steps"]).sum())
        out["steps_per_second"] = total / (out["follow"]["median_ms"] * 1e-3)
        out["microseconds_per_step_of_the_longest_row"] = out["follow"]["median_ms"] * 1e3 / max(out["steps_max"], 1)
        out["status_histogram_0_1_2"] = torch.bincount(status, minlength=3).tolist()
        out["bits_histogram"] = torch.bincount(bits, minlength=16).tolist()
        out["valid_share_of_planned"] = float((status[planned] == 0).float().mean()) if int(planned.sum()) else None
        out["ratio_follow_over_plan_global"] = out["follow"]["median_ms"] / out["plan_global"]["median_ms"]
        res["cases"][str(B)] = out
        del prob
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
