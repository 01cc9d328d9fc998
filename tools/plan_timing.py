"""Time mpx_franka_plan (csrc/plan.hip) on the GPU: 8192 problems, 8 candidates x the default iterations, in free space,
against tabletop scenes (16 + 16 slots) and against the mixed tabletop / cubby / dresser scenes at M1 = 40, plus one
iteration only.  HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), and
the solved share of each case (over the problems whose start and goal ``make_problem_batch(collision_free=True)`` posed).
The timed call is ``robot.franka_plan`` as a user makes it: besides the kernel it holds the wrapper's host work (the
inward rounding of the limits and their copy to the device, the option struct, four output allocations); the kernel alone
is the ``franka_plan_kernel`` line of ``rocprofv3 --kernel-trace --stats``.

    python tools/plan_timing.py [--envs 8192] [--iterations N] [--candidates K]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ik_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--candidates", type=int, default=None, help="16: the <16> kernel instantiations")
    args = ap.parse_args()
    from mpinets_amd import robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    dev = torch.device("cuda:0")
    B = args.envs
    opts = {k: v for k, v in (("iterations", args.iterations), ("candidates", args.candidates)) if v is not None}
    res = {"envs": B, "options": dict(robot.PLAN_DEFAULTS, **opts)}

    def case(kinds, M1, M2):
        prob = scenes.make_problem_batch(B, seed=0, kinds=kinds, M1=M1, M2=M2, scene_pool=1024, device_clouds=True,
                                         collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        qg = torch.where(prob["valid"][:, None], prob["q_goal"], prob["q"])  # (unposed rows: a trivial problem, same work)
        return prob, cub, cyl, qg

    def run(name, fn, posed):
        res[name] = timed(fn)
        status = fn()[1]
        res[name]["share_solved"] = float((status[posed] == 0).float().mean())
        res[name]["posed"] = int(posed.sum())

    prob, cub, cyl, qg = case(("tabletop",), 16, 16)
    everyone = torch.ones(B, dtype=torch.bool, device=dev)
    run("free_space", lambda: robot.franka_plan(prob["q"], qg, **opts), everyone)
    run("tabletop_scenes", lambda: robot.franka_plan(prob["q"], qg, cub, cyl, **opts), prob["valid"])
    run("one_iteration_tabletop", lambda: robot.franka_plan(prob["q"], qg, cub, cyl, iterations=1), prob["valid"])
    probm, cubm, cylm, qgm = case(("tabletop", "cubby", "dresser"), 40, 16)
    run("mixed_scenes_M1_40", lambda: robot.franka_plan(probm["q"], qgm, cubm, cylm, **opts), probm["valid"])
    st0 = robot.franka_plan(probm["q"], qgm, cubm, cylm, iterations=0)[1]
    res["mixed_scenes_M1_40"]["share_solved_without_iterations"] = float((st0[probm["valid"]] == 0).float().mean())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
