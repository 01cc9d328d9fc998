"""Time mpx_franka_shortcut and mpx_franka_shortcut_cloud (csrc/shortcut_kernel.inc) on the GPU beside the roadmaps whose
paths they shorten, and robot.franka_plan_global / franka_plan_global_cloud with and without ``shortcut=True``: B mixed
tabletop / cubby / dresser problems of ``make_problem_batch(collision_free=True)`` (M1 = 40, M2 = 16), the cloud forms
against the rows' own scene clouds (the 4096 scene rows of the slab, read in place, at ``EXPERT_CLOUD_POINT_RADIUS``) through
one field built once.  The shortcut's input is ``nodes[path]`` of the roadmap of the same rows, as the global planners hand
it over.  HIP events around each call as a user makes it (the wrappers' host work included), 3 untimed calls, then the
median of 10 with the spread; with the times the chords and interior configurations tested per row, the polyline lengths
before and after and the solved shares.

    python tools/shortcut_timing.py [--envs 8192] [--out FILE.json] [--md FILE.md]

``--md`` writes the tables of profiles/shortcut_timing.md.
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
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--out", help="also write the result to this JSON file")
    ap.add_argument("--md", help="also write the tables as markdown to this file")
    args = ap.parse_args()
    from mpinets_amd import robot, scenes, solvers
    from mpinets_amd.field import CloudField
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    B = args.envs
    prob = scenes.make_problem_batch(B, seed=0, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16,
                                     scene_pool=min(B, 1024), device_clouds=True, collision_free=True)
    cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
    cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
    posed = prob["valid"]
    qs, qg = prob["q"], torch.where(posed[:, None], prob["q_goal"], prob["q"])  # (unposed rows: a trivial problem)
    cloud, pr = prob["xyz"][:, 2048:6144, :3], scenes.EXPERT_CLOUD_POINT_RADIUS
    field = CloudField.build(cloud, truncation=robot.plan_cloud_truncation(pr))
    ckw = dict(field=field, point_radius=pr)
    res = {"B": B, "posed": int(posed.sum()), "shortcut_options": robot.SHORTCUT_DEFAULTS, "forms": {}}

    def share(st):
        return float(((st == 0) & posed).float().sum() / posed.sum())

    def mean(x, rows):
        return float(x[rows].float().mean()) if bool(rows.any()) else None

    forms = (("primitives", lambda **k: robot.franka_roadmap(qs, qg, cub, cyl, seed=0, **k),
              lambda p, c, **k: robot.franka_shortcut(p, c, cub, cyl, **k),
              lambda **k: robot.franka_plan_global(qs, qg, cub, cyl, seed=0, **k)),
             ("cloud", lambda **k: robot.franka_roadmap_cloud(qs, qg, cloud, seed=0, **ckw, **k),
              lambda p, c, **k: robot.franka_shortcut_cloud(p, c, cloud, **ckw, **k),
              lambda **k: robot.franka_plan_global_cloud(qs, qg, cloud, seed=0, **ckw, **k)))
    for name, roadmap, shortcut, plan in forms:
        row = {"roadmap": timed(lambda: roadmap())}
        graph = roadmap(return_graph=True)
        pts, cnt = solvers._path_vertices(graph[4], graph[2], graph[3])
        found = posed & (cnt >= 2)
        many = found & (cnt > 2)
        row["roadmap"].update(share_found=share(graph[1]), more_than_one_edge=int(many.sum()))
        row["shortcut"] = timed(lambda: shortcut(pts, cnt))
        traj, st, po, co, ln, ch, cf = shortcut(pts, cnt, return_trace=True)
        row["shortcut"].update(chords_mean=mean(ch, many), chords_max=int(ch.max()), configs_mean=mean(cf, many),
                               configs_max=int(cf.max()), length_before=mean(ln[:, 0], many), length_after=mean(ln[:, 1], many),
                               one_edge_after=int((many & (co == 2)).sum()), vertices_after=mean(co, many))
        for tag, kw in (("plan_global", {}), ("plan_global_shortcut", dict(shortcut=True))):
            t = timed(lambda: plan(**kw))
            out = plan(return_all=True, **kw)
            ok = posed & (out[1] == 0)
            t.update(share_solved=share(out[1]), choice=torch.bincount(out[2][ok].long()).tolist(),
                     length=float((out[0][ok][:, 1:] - out[0][ok][:, :-1]).norm(dim=-1).sum(-1).mean()))
            row[tag] = t
        res["forms"][name] = row
        print(json.dumps({name: row}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    if args.md:
        ms = lambda t: f"{t['median_ms']:.3f} ({t['min_ms']:.3f} - {t['max_ms']:.3f})"  # noqa: E731
        with open(args.md, "w") as f:
            f.write(f"B = {B}, posed {res['posed']}\n\n| form | roadmap | found | paths of > 1 edge | shortcut | chords / row | "
                    "configurations / row | length before -> after [rad] | one edge after |\n|---|---|---|---|---|---|---|---|---|\n")
            for name, r in res["forms"].items():
                s = r["shortcut"]
                f.write(f"| {name} | {ms(r['roadmap'])} | {r['roadmap']['share_found']:.4f} | {r['roadmap']['more_than_one_edge']} | "
                        f"{ms(s)} | {s['chords_mean']:.1f} (max {s['chords_max']}) | {s['configs_mean']:.0f} (max {s['configs_max']}) | "
                        f"{s['length_before']:.3f} -> {s['length_after']:.3f} | {s['one_edge_after']} |\n")
            f.write("\n| form | global planner | solved | mean length [rad] | with `shortcut=True` | solved | mean length [rad] | choice |\n"
                    "|---|---|---|---|---|---|---|---|\n")
            for name, r in res["forms"].items():
                a, b = r["plan_global"], r["plan_global_shortcut"]
                f.write(f"| {name} | {ms(a)} | {a['share_solved']:.4f} | {a['length']:.3f} | {ms(b)} | {b['share_solved']:.4f} | "
                        f"{b['length']:.3f} | {b['choice']} |\n")


if __name__ == "__main__":
    main()
