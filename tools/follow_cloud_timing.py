"""Time the cloud form of the path follower (csrc/follow_cloud.hip, ``robot.franka_follow_cloud``) on the GPU beside
``robot.franka_follow`` on the same rows.

For B in --envs (default 8192) mixed tabletop / cubby / dresser problems (M1 = 40, M2 = 16, start and goal posed by
``make_problem_batch(collision_free=True)``; the batch of tools/follow_timing.py):

  * the guide: the right_gripper poses of waypoints round(i * 49 / 8), i = 1..8, of ``robot.franka_plan_global``'s plan (W = 8),
    as ``make_problem_batch(hybrid=True)`` builds it; rows without a plan hand NaN poses and come back with status 2.  BOTH
    followers get this one guide, so the two differ in the environment only;
  * ``robot.franka_follow`` against the primitives (T = 50, defaults: at most 1024 steps);
  * ``CloudField.build`` of the rows' own scene clouds (the 4096 scene rows of the slab, read in place) on the default grid
    with the follower's truncation at ``EXPERT_CLOUD_POINT_RADIUS``: 8192 environments x 61 x 61 x 51 nodes are 6.2 GB;
  * ``robot.franka_follow_cloud`` against those clouds with that field handed in: milliseconds per call, mean steps per row
    over the rows that ran, the status and bits histograms, the valid share over the planned rows -- "valid" by
    ``check_cloud``'s test at that radius, which is not the primitive test.

The follower is a stand-in for the reference's Geometric Fabrics expert, not Lula: the numbers say what this controller
costs, nothing about the fabric.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as tools/follow_timing.py.
The timed calls are the Python entry points as a user makes them (wrapper host work and output allocations included).
The kernels' register and LDS figures are read from the built library's code object (tests/test_code_objects.py's reader).

    python tools/follow_cloud_timing.py [--envs 8192] [--out FILE.json]
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
FIGURES = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
           ".group_segment_fixed_size")


def kernel_figures():
    from test_code_objects import LIB, kernel_metadata

    meta = kernel_metadata(LIB)
    out = {}
    for name in ("franka_follow_kernel", "franka_follow_cloud_kernel", "franka_follow_cloud_finish_kernel"):
        (f,) = [f for n, f in meta.items() if name + "PK" in n or name + "i" in n]
        out[name] = {k.lstrip("."): int(f[k]) for k in FIGURES}
    return out


def summary(status, bits, steps, planned, t, max_steps):
    ran = status != 2
    total = int(steps.sum())
    return dict(t, steps_mean_over_rows_that_ran=total / max(int(ran.sum()), 1), steps_max=int(steps.max()),
                rows_at_max_steps=int((steps == max_steps).sum()), steps_per_second=total / (t["median_ms"] * 1e-3),
                status_histogram_0_1_2=torch.bincount(status, minlength=3).tolist(),
                bits_histogram=torch.bincount(bits, minlength=16).tolist(),
                valid_share_of_planned=float((status[planned] == 0).float().mean()) if int(planned.sum()) else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[8192])
    ap.add_argument("--out", help="also write the result to this JSON file")
    args = ap.parse_args()
    from mpinets_amd import franka_tables as ft, robot, scenes
    from mpinets_amd.field import CloudField
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    torch.cuda.set_device(0)
    pr = scenes.EXPERT_CLOUD_POINT_RADIUS
    res = {"options": robot.FOLLOW_DEFAULTS, "T": 50, "W": scenes.HYBRID_GUIDE_POSES, "point_radius": pr,
           "kernels": kernel_figures(), "cases": {}}
    gripper = ft.LINK_ID["right_gripper"]
    max_steps = robot.FOLLOW_DEFAULTS["max_steps"]
    for B in args.envs:
        prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True,
                                         collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        qs, qg = prob["q"], prob["q_goal"]  # (unposed rows have a NaN goal: status 2 in every entry)
        cloud = prob["xyz"][:, 2048:6144, :3]
        out = {"posed": int(prob["valid"].sum()), "cloud_points": int(cloud.size(1))}
        plan, st = robot.franka_plan_global(qs, qg, cub, cyl)[:2]
        planned = st == 0
        out["planned"] = int(planned.sum())
        at = [int(round(i * 49 / scenes.HYBRID_GUIDE_POSES)) for i in range(1, scenes.HYBRID_GUIDE_POSES + 1)]
        guide = robot.frames_to_matrix(robot.franka_fk(plan[:, at].reshape(-1, 7))[:, gripper]).reshape(B, len(at), 4, 4)
        t = timed(lambda: robot.franka_follow(qs, guide, cub, cyl))
        _, status, bits, steps = robot.franka_follow(qs, guide, cub, cyl)
        out["franka_follow"] = summary(status, bits, steps, planned, t, max_steps)
        trunc = robot.plan_cloud_truncation(pr)
        out["field_build"] = timed(lambda: CloudField.build(cloud, truncation=trunc))
        field = CloudField.build(cloud, truncation=trunc)
        out["field_bytes"] = field.values.numel() * 4
        t = timed(lambda: robot.franka_follow_cloud(qs, guide, cloud, field=field, point_radius=pr))
        _, cstatus, cbits, csteps = robot.franka_follow_cloud(qs, guide, cloud, field=field, point_radius=pr)
        out["franka_follow_cloud"] = summary(cstatus, cbits, csteps, planned, t, max_steps)
        out["ratio_cloud_over_primitives"] = out["franka_follow_cloud"]["median_ms"] / out["franka_follow"]["median_ms"]
        both = planned & (status == 0) & (cstatus == 0)
        out["valid_in_both_share_of_planned"] = float(both.float().sum() / max(int(planned.sum()), 1))
        res["cases"][str(B)] = out
        del prob, field
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
