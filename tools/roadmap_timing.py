"""Time mpx_franka_roadmap (csrc/roadmap.hip) and robot.franka_plan_global (the roadmap, then mpx_franka_plan_seeded) on the
GPU beside robot.franka_plan on the same inputs: B = 1, 256, 1024, 8192 problems, V = 64, 128, 256 nodes, on the mixed
tabletop / cubby / dresser scenes of ``make_problem_batch(collision_free=True)`` (M1 = 40, M2 = 16) and on the forced-detour
problems of tests/test_roadmap_host.py (one 10 cm cube on the straight line).  HIP events around each call as a user makes
it (the wrappers' host work included), 3 untimed calls, then the median of 10 with the spread; with each case the status
counts, the rounds and hops histograms and the solved shares.

    python tools/roadmap_timing.py [--envs 1,256,1024,8192] [--nodes 64,128,256] [--plan-only] [--out FILE.json]

``--plan-only`` times franka_plan alone: with MPX_LIB_PATH pointing at another build of the library (the parent commit's),
that build's planner on the same inputs.
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
    ap.add_argument("--envs", default="1,256,1024,8192")
    ap.add_argument("--nodes", default="64,128,256")
    ap.add_argument("--plan-only", action="store_true")
    ap.add_argument("--out", help="also write every case to this JSON file")
    args = ap.parse_args()
    from mpinets_amd import robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders
    from test_roadmap_host import DETOUR_PLAN_SEED, detour_problems

    dev = torch.device("cuda:0")
    res = {"plan_options": robot.PLAN_DEFAULTS, "cases": []}
    if not args.plan_only:
        res["roadmap_options"] = dict(robot.ROADMAP_DEFAULTS, connect_radius="inf")

    def hist(x):
        return torch.bincount(x.long()).tolist()

    def mixed(B):
        prob = scenes.make_problem_batch(B, seed=0, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16,
                                         scene_pool=min(B, 1024), device_clouds=True, collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        qg = torch.where(prob["valid"][:, None], prob["q_goal"], prob["q"])  # (unposed rows: a trivial problem)
        return prob["q"], qg, cub, cyl, prob["valid"], dict(seed=0)

    def detour(B):
        qs, qg, lim, scn = detour_problems(B)
        t = {k: torch.from_numpy(v).to(dev) for k, v in scn.items()}
        cub = TorchCuboids(t["cuboid_centers"], t["cuboid_dims"], t["cuboid_quats"])
        cyl = TorchCylinders(t["cylinder_centers"], t["cylinder_radii"], t["cylinder_heights"], t["cylinder_quats"])
        return torch.from_numpy(qs).to(dev), torch.from_numpy(qg).to(dev), cub, cyl, torch.ones(B, dtype=torch.bool, device=dev), \
            dict(seed=DETOUR_PLAN_SEED, limits=lim)

    for name, make in (("mixed", mixed), ("detour", detour)):
        for B in (int(x) for x in args.envs.split(",")):
            qs, qg, cub, cyl, posed, kw = make(B)
            row = {"inputs": name, "B": B, "posed": int(posed.sum())}
            row["franka_plan"] = timed(lambda: robot.franka_plan(qs, qg, cub, cyl, **kw))
            st = robot.franka_plan(qs, qg, cub, cyl, **kw)[1]
            row["franka_plan"].update(status=hist(st[posed]), share_solved=float((st[posed] == 0).float().mean()))
            for V in ([] if args.plan_only else [int(x) for x in args.nodes.split(",")]):
                r = timed(lambda: robot.franka_roadmap(qs, qg, cub, cyl, nodes=V, **kw))
                out = robot.franka_roadmap(qs, qg, cub, cyl, nodes=V, return_graph=True, **kw)
                found = posed & (out[1] == 0)
                r.update(status=hist(out[1][posed]), hops=hist(out[3][found]), rounds=hist(out[6][posed]),
                         share_found=float(found.float().sum() / posed.sum()))
                g = timed(lambda: robot.franka_plan_global(qs, qg, cub, cyl, roadmap=dict(nodes=V), **kw))
                gout = robot.franka_plan_global(qs, qg, cub, cyl, roadmap=dict(nodes=V), return_all=True, **kw)
                ok = posed & (gout[1] == 0)
                g.update(status=hist(gout[1][posed]), share_solved=float(ok.float().sum() / posed.sum()), choice=hist(gout[2][ok]))
                row[f"V{V}"] = {"franka_roadmap": r, "franka_plan_global": g}
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
