"""Time the task-oriented candidate draw (csrc/task_candidates.hip, ``robot.task_candidates``) on the GPU beside the IK launches
it feeds and the stage it replaces, and record what the task problems do to the yield of the pipeline.

For B in --envs (default 8192) mixed tabletop / cubby / dresser problems (M1 = 40, M2 = 16, S = 8, 256 distinct scenes):

  * ``robot.task_candidates`` (N = 100 draws, C = 8, role 0): milliseconds per call, the histogram of ``count`` and the share
    of free draws' supports per kind;
  * ``robot.franka_ik`` on candidate 0 of every problem: one of the up to 2 x 8 IK launches a task batch makes;
  * ``scenes._task_problems`` (both roles: two candidate calls and the IK launches until every row is settled) and
    ``scenes._collision_free_problems`` (the uniform stage it stands beside: up to five attempts of two IK launches) on the
    same batch.

Then, on one batch of --yield-envs (default 1024) problems per scene kind, how many rows come out ``valid`` and
``expert_valid`` under ``problems="task"`` and under ``"uniform"``.

The candidates are a restatement of the reference's distributions judged by this engine's sphere model, not by PyBullet's
meshes: the numbers say what this draw costs and yields, nothing about the reference's generators.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as tools/ik_timing.py.
The timed calls are the Python entry points as a user makes them (wrapper host work and output allocations included).
The kernel's register and LDS figures are read from the built library's code object (tests/test_code_objects.py's reader).

    python tools/task_candidates_timing.py [--envs 8192] [--yield-envs 1024]
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


def kernel_figures():
    from test_code_objects import LIB, kernel_metadata

    (f,) = [f for n, f in kernel_metadata(LIB).items() if "task_candidates_kernel" in n]
    return {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                               ".private_segment_fixed_size", ".group_segment_fixed_size")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192])
    ap.add_argument("--yield-envs", type=int, default=1024)
    args = ap.parse_args()
    from mpinets_amd import robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    res = {"options": robot.TASK_CANDIDATES_DEFAULTS, "C": scenes.TASK_CANDIDATES, "kernel": kernel_figures(), "cases": {}, "yield": {}}
    for B in args.envs:
        pool = min(B, 256)
        scn = scenes.make_task_scenes(pool, 0, MIXED, 40, 16)
        sid = np.arange(B) % pool
        prims = {k: torch.from_numpy(np.ascontiguousarray(v[sid])).to(dev) for k, v in scn.items()}
        cub = TorchCuboids(prims["cuboid_centers"], prims["cuboid_dims"], prims["cuboid_quats"])
        cyl = TorchCylinders(prims["cylinder_centers"], prims["cylinder_radii"], prims["cylinder_heights"], prims["cylinder_quats"])
        boxes, kind = prims["support_boxes"], prims["support_kind"]
        q = torch.from_numpy(scenes.random_configurations(B, 0)).to(dev)
        q_target = torch.from_numpy(scenes.random_configurations(B, 7)).to(dev)
        out = {}
        out["task_candidates"] = timed(lambda: robot.task_candidates(boxes, kind, cub, cyl, C=scenes.TASK_CANDIDATES))
        poses, draw, support, count = robot.task_candidates(boxes, kind, cub, cyl, C=scenes.TASK_CANDIDATES)
        out["task_candidates"].update(count_histogram=torch.bincount(count.long(), minlength=scenes.TASK_CANDIDATES + 1).tolist(),
                                      count_mean_by_kind={k: float(count[i::3].float().mean()) for i, k in enumerate(MIXED)},
                                      first_kept_draw_mean=float(draw[count > 0, 0].float().mean()))
        first = torch.where((count > 0)[:, None, None], poses[:, 0], torch.eye(4, device=dev)).contiguous()
        out["franka_ik_on_candidate_0"] = timed(lambda: robot.franka_ik(first, cub, cyl))
        out["franka_ik_on_candidate_0"]["solved_share"] = float(((robot.franka_ik(first, cub, cyl)[1] == 0) & (count > 0)).float().mean())
        out["task_problems"] = timed(lambda: scenes._task_problems(prims, boxes, kind, q, q_target, 0, 0), warm=1, reps=5)
        out["task_problems"]["valid"] = int(scenes._task_problems(prims, boxes, kind, q, q_target, 0, 0)[2].sum())
        out["collision_free_problems"] = timed(lambda: scenes._collision_free_problems(prims, q, q_target, 0, 0, 4), warm=1, reps=5)
        out["collision_free_problems"]["valid"] = int(scenes._collision_free_problems(prims, q, q_target, 0, 0, 4)[3].sum())
        res["cases"][str(B)] = out
        del prims, cub, cyl
        torch.cuda.empty_cache()
    Y = args.yield_envs
    for kind_name in MIXED:
        row = {}
        for problems in ("task", "uniform"):
            prob = scenes.make_problem_batch(Y, seed=0, kinds=(kind_name,), M1=40, M2=16, scene_pool=min(Y, 256), device_clouds=True,
                                             collision_free=True, expert=True, problems=problems)
            row[problems] = {"valid": int(prob["valid"].sum()), "expert_valid": int(prob["expert_valid"].sum())}
            del prob
            torch.cuda.empty_cache()
        res["yield"][kind_name] = dict(row, envs=Y)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
