"""Time mpx_franka_roadmap_cloud (csrc/roadmap_cloud.hip) and robot.franka_plan_global_cloud (the roadmap, then
mpx_franka_plan_cloud_seeded) on the GPU beside robot.franka_plan_cloud, and beside robot.franka_roadmap against the
primitives of the same rows: B mixed tabletop / cubby / dresser problems of ``make_problem_batch(collision_free=True)``
(M1 = 40, M2 = 16) against their own scene clouds (the 4096 scene rows of the slab, read in place, at
``EXPERT_CLOUD_POINT_RADIUS``), and the forced detour of tests/float64_cloud_plan.py drawn as a cloud.  One field per case,
built once on the default grid and handed to every call (its build is timed on its own); 8192 environments x 61 x 61 x 51
nodes are 6.2 GB.  HIP events around each call as a user makes it (the wrappers' host work included), 3 untimed calls, then
the median of 10 with the spread; with each case the status counts, the hops and rounds histograms and the solved shares at
``field_slack`` 0 and 0.866 x voxel.

    python tools/roadmap_cloud_timing.py [--envs 8192] [--detour 256] [--out FILE.json] [--md FILE.md]

``--md`` writes the tables of profiles/roadmap_cloud_timing.md, section 1.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from ik_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="8192")
    ap.add_argument("--detour", type=int, default=256)
    ap.add_argument("--out", help="also write every case to this JSON file")
    ap.add_argument("--md", help="also write the tables as markdown to this file")
    args = ap.parse_args()
    import float64_cloud_plan as fcp
    from mpinets_amd import robot, scenes
    from mpinets_amd.field import DEFAULT_VOXEL, CloudField
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    dev = torch.device("cuda:0")
    slack = 0.866 * DEFAULT_VOXEL
    res = {"plan_options": robot.PLAN_DEFAULTS, "roadmap_options": dict(robot.ROADMAP_DEFAULTS, connect_radius="inf"),
           "voxel": DEFAULT_VOXEL, "conservative_slack": slack, "cases": []}

    def hist(x):
        return torch.bincount(x.long()).tolist()

    def mixed(B):
        prob = scenes.make_problem_batch(B, seed=0, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16,
                                         scene_pool=min(B, 1024), device_clouds=True, collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        qg = torch.where(prob["valid"][:, None], prob["q_goal"], prob["q"])  # (unposed rows: a trivial problem)
        return prob["q"], qg, prob["xyz"][:, 2048:6144, :3], scenes.EXPERT_CLOUD_POINT_RADIUS, (cub, cyl), prob["valid"], dict(seed=0)

    def detour(B):
        qs, qg, lim, cloud, _ = fcp.detour_problems(B)
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        return up(qs), up(qg), up(cloud), fcp.WALL_POINT_RADIUS, None, torch.ones(B, dtype=torch.bool, device=dev), \
            dict(seed=9, limits=lim)

    cases = [("mixed", mixed, int(x)) for x in args.envs.split(",") if int(x) > 0]
    if args.detour > 0:
        cases.append(("detour", detour, args.detour))
    for name, make, B in cases:
        qs, qg, cloud, pr, prims, posed, kw = make(B)
        trunc = robot.plan_cloud_truncation(pr)
        row = {"inputs": name, "B": B, "posed": int(posed.sum()), "cloud_points": int(cloud.size(1)), "point_radius": pr}
        row["field_build"] = timed(lambda: CloudField.build(cloud, truncation=trunc))
        field = CloudField.build(cloud, truncation=trunc)
        row["field_bytes"] = field.values.numel() * 4
        ckw = dict(kw, field=field, point_radius=pr)
        if prims is not None:  # the parent's roadmap against the primitives the clouds were drawn from: context
            r = timed(lambda: robot.franka_roadmap(qs, qg, *prims, **kw))
            st = robot.franka_roadmap(qs, qg, *prims, **kw)[1]
            row["franka_roadmap"] = dict(r, status=hist(st[posed]), share_found=float((st[posed] == 0).float().mean()))
        p = timed(lambda: robot.franka_plan_cloud(qs, qg, cloud, **ckw))
        st = robot.franka_plan_cloud(qs, qg, cloud, **ckw)[1]
        row["franka_plan_cloud"] = dict(p, status=hist(st[posed]), share_solved=float((st[posed] == 0).float().mean()))
        for tag, fs in (("slack0", 0.0), ("slack0.866h", slack)):
            r = timed(lambda: robot.franka_roadmap_cloud(qs, qg, cloud, field_slack=fs, **ckw))
            out = robot.franka_roadmap_cloud(qs, qg, cloud, field_slack=fs, return_graph=True, **ckw)
            found = posed & (out[1] == 0)
            r.update(status=hist(out[1][posed]), hops=hist(out[3][found]), rounds=hist(out[6][posed]),
                     share_found=float(found.float().sum() / posed.sum()))
            g = timed(lambda: robot.franka_plan_global_cloud(qs, qg, cloud, field_slack=fs, **ckw))
            gout = robot.franka_plan_global_cloud(qs, qg, cloud, field_slack=fs, return_all=True, **ckw)
            ok = posed & (gout[1] == 0)
            seed_bits = gout[4][posed & (gout[5] == 0), -1]
            g.update(status=hist(gout[1][posed]), share_solved=float(ok.float().sum() / posed.sum()), choice=hist(gout[2][ok]),
                     seed_valid_share=float((seed_bits == 0).float().mean()) if seed_bits.numel() else None)
            row[tag] = {"franka_roadmap_cloud": r, "franka_plan_global_cloud": g}
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
        del field
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        ms = lambda t: f"{t['median_ms']:.3f} ({t['min_ms']:.3f} - {t['max_ms']:.3f})"  # noqa: E731
        with open(args.md, "w") as f:
            f.write("| inputs | B | posed | field build | `franka_roadmap` (primitives) | found | `franka_plan_cloud` | solved |\n|---|---|---|---|---|---|---|---|\n")
            for r in res["cases"]:
                rm = r.get("franka_roadmap")
                prim = f"{ms(rm)} | {rm['share_found']:.4f}" if rm else "- | -"
                f.write(f"| {r['inputs']} | {r['B']} | {r['posed']} | {ms(r['field_build'])} | {prim} | "
                        f"{ms(r['franka_plan_cloud'])} | {r['franka_plan_cloud']['share_solved']:.4f} |\n")
            f.write("\n| inputs | `field_slack` | `franka_roadmap_cloud` | status 0 / 1 / 2 | hops | `franka_plan_global_cloud` | solved | seed valid |\n|---|---|---|---|---|---|---|---|\n")
            for r in res["cases"]:
                for tag in ("slack0", "slack0.866h"):
                    a, g = r[tag]["franka_roadmap_cloud"], r[tag]["franka_plan_global_cloud"]
                    sv = g["seed_valid_share"]
                    f.write(f"| {r['inputs']} | {tag[5:]} | {ms(a)} | {' / '.join(map(str, (a['status'] + [0, 0, 0])[:3]))} | "
                            f"{a['hops']} | {ms(g)} | {g['share_solved']:.4f} | {'-' if sv is None else f'{sv:.4f}'} |\n")


if __name__ == "__main__":
    main()
