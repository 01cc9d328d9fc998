"""Time mpx_gripper_shortcut and mpx_gripper_shortcut_cloud (csrc/gripper_shortcut.hip, gripper_shortcut_cloud.hip) on the GPU
beside the gripper roadmaps whose paths they shorten, and record what the shortcut guide does to the hybrid expert, on the
batch of profiles/gripper_roadmap_timing.md: B mixed tabletop / cubby / dresser problems of
``make_problem_batch(collision_free=True)`` (M1 = 40, M2 = 16, scene_pool 256), the cloud forms against the rows' own scene
clouds (the 4096 scene rows of the slab, read in place, at ``EXPERT_CLOUD_POINT_RADIUS``) through one field built once.  The
shortcut's input is ``nodes[path]`` of the roadmap of the same rows, as ``gripper_plan`` hands it over.

  * time: HIP events around each call as a user makes it (the wrappers' host work included), 3 untimed calls, then the median
    of 10 with the spread; with the times the chords and interior poses tested per row and the metric lengths before and after;
  * use: ``robot.franka_follow`` along the roadmap's guide, along the shortcut's, and along the shortcut's at ``clearance``
    0.02: the follower's status split, its bits, its mean steps and ``hybrid_valid`` (planned by ``franka_plan_global`` and
    followed and valid) on the same batch.  Recorded, not floors.

    python tools/gripper_shortcut_timing.py [--envs 8192] [--out FILE.json]
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

    out = {}
    for name in ("gripper_shortcut_kernel", "gripper_shortcut_cloud_kernel"):
        (f,) = [f for n, f in kernel_metadata(LIB).items() if name + "PK" in n]
        out[name] = {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                                        ".private_segment_fixed_size", ".group_segment_fixed_size")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--out", help="also write the result to this JSON file")
    args = ap.parse_args()
    from mpinets_amd import franka_tables as ft, robot, scenes, solvers
    from mpinets_amd.field import CloudField
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    torch.cuda.set_device(0)
    B, W = args.envs, scenes.HYBRID_GUIDE_POSES
    prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True,
                                     collision_free=True)
    cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
    cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
    qs, qg, posed = prob["q"], prob["q_goal"], prob["valid"]  # (unposed rows have a NaN goal: status 2 in every entry)
    gripper = ft.LINK_ID["right_gripper"]
    ends = robot.frames_to_matrix(robot.franka_fk(torch.cat([qs, qg]))[:, gripper])
    sp, gp = ends[:B].contiguous(), ends[B:].contiguous()
    cloud, pr = prob["xyz"][:, 2048:6144, :3], scenes.EXPERT_CLOUD_POINT_RADIUS
    field = CloudField.build(cloud, truncation=robot.plan_cloud_truncation(pr))
    ckw = dict(field=field, point_radius=pr)
    res = {"B": B, "posed": int(posed.sum()), "W": W, "options": robot.GRIPPER_SHORTCUT_DEFAULTS, "kernels": kernel_figures(),
           "forms": {}}

    def hist(x, n=0):
        return torch.bincount(x.long(), minlength=n).tolist()

    def mean(x, rows):
        return float(x[rows].float().mean()) if bool(rows.any()) else None

    forms = (("primitives", lambda **k: robot.gripper_roadmap(sp, gp, cub, cyl, W=W, **k),
              lambda p, c, **k: robot.gripper_shortcut(p, c, cub, cyl, W=W, goal_pose=gp, **k)),
             ("cloud", lambda **k: robot.gripper_roadmap_cloud(sp, gp, cloud, W=W, **ckw, **k),
              lambda p, c, **k: robot.gripper_shortcut_cloud(p, c, cloud, W=W, goal_pose=gp, **ckw, **k)))
    guides = {}
    for name, roadmap, shortcut in forms:
        row = {"roadmap": timed(lambda: roadmap())}
        graph = roadmap(return_graph=True)
        pts, cnt = solvers._path_vertices(graph[4], graph[2], graph[3])
        found = posed & (cnt >= 2)
        many = found & (cnt > 2)
        row["roadmap"].update(found=int(found.sum()), more_than_one_edge=int(many.sum()), hops=hist(graph[3][found]))
        row["shortcut"] = timed(lambda: shortcut(pts, cnt))
        poses, st, po, co, ln, ch, cf = shortcut(pts, cnt, return_trace=True)
        row["shortcut"].update(ratio_to_roadmap=row["shortcut"]["median_ms"] / row["roadmap"]["median_ms"],
                               chords_mean=mean(ch, many), chords_max=int(ch.max()), poses_mean=mean(cf, many),
                               poses_max=int(cf.max()), length_before=mean(ln[:, 0], many), length_after=mean(ln[:, 1], many),
                               shorter_by_1_percent=int((many & (ln[:, 1] < 0.99 * ln[:, 0])).sum()),
                               one_edge_after=int((many & (co == 2)).sum()), vertices_after=mean(co, many))
        if name == "primitives":
            guides = {"roadmap": graph[0], "shortcut": poses,
                      "shortcut_clearance_0.02": shortcut(pts, cnt, clearance=0.02)[0]}
            many_prim = many
        res["forms"][name] = row
        print(json.dumps({name: row}), flush=True)

    # ---- use: the follower along the three guides, on the same batch ---------------------------------------------------------------
    plan, pst = robot.franka_plan_global(qs, qg, cub, cyl)[:2]
    planned = pst == 0
    use = {"planned": int(planned.sum()), "planned_with_more_than_one_edge": int((planned & many_prim).sum())}
    valid_rows = {}
    for tag, guide in guides.items():
        _, fst, bits, steps = robot.franka_follow(qs, guide, cub, cyl)
        valid = planned & (fst == 0)
        valid_rows[tag] = valid
        use[tag] = dict(status_0_1_2=hist(fst, 3), bits=hist(bits, 16), hybrid_valid=int(valid.sum()),
                        hybrid_valid_share_of_planned=float(valid.sum() / planned.sum()),
                        hybrid_valid_on_paths_of_more_than_one_edge=int((valid & many_prim).sum()),
                        steps_mean=float(steps[fst != 2].float().mean()),
                        steps_mean_on_paths_of_more_than_one_edge=mean(steps, many_prim & (fst != 2)))
    a, b = valid_rows["roadmap"], valid_rows["shortcut"]
    use["valid_both_only_roadmap_only_shortcut"] = [int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum())]
    res["use"] = use
    print(json.dumps({"use": use}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
