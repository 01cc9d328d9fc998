"""Time the cloud planner (csrc/cloud_field.hip) on the GPU next to the primitive planner it stands beside.

For B in --envs (default 1 64 1024) mixed tabletop / cubby / dresser problems (M1 = 40, M2 = 16, start and goal posed by
``make_problem_batch(collision_free=True)``) and their 4096-point scene clouds:

  * ``CloudField.build`` at the default grid (61 x 61 x 51 nodes, 3 cm) with the planner's default truncation;
  * ``robot.franka_plan_cloud`` (T = 50, K = 8, defaults) on a prebuilt field, and its split.  The entry enqueues a
    memset, the optimise kernel, K + 1 flag calls and the select kernel; the split is taken by leaving stages out through
    the public arguments: "no_flag_calls" passes the cloud with N = 0 (the field still steers, nothing is judged),
    "drawn_only" also sets iterations = 0.  validity = full - no_flag_calls, optimise = no_flag_calls - drawn_only, and
    drawn_only is what is left: the candidate draw, the jerk and self tests, writing the refined configurations, select;
  * ``robot.franka_plan`` on the primitives those clouds were drawn from: the only comparator there is;
  * the solved share of both planners over the posed problems, and the share of cloud-solved trajectories that the
    primitive test ``FrankaCollisionSampler.check`` rejects, for point_radius 0 and half the clouds' mean
    nearest-neighbour spacing.

Once: ``CloudField.sample`` of 2^20 points (one environment), with and without the gradient.

HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max), as tools/plan_timing.py.
The timed calls are the Python entry points as a user makes them (wrapper host work included).

    python tools/cloud_plan_timing.py [--envs 1 64 1024] [--candidates K]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--candidates", type=int, default=None, help="16: the <16> kernel instantiations")
    args = ap.parse_args()
    from mpinets_amd import robot, scenes
    from mpinets_amd.field import CloudField
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders
    from mpinets_amd.robot import FrankaCollisionSampler

    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    kw = {} if args.candidates is None else {"candidates": args.candidates}
    res = {"options": dict(robot.PLAN_DEFAULTS, **kw), "T": 50, "cases": {}}
    sampler = FrankaCollisionSampler(dev)
    for B in args.envs:
        prob = scenes.make_problem_batch(B, seed=0, kinds=MIXED, M1=40, M2=16, scene_pool=min(B, 256), device_clouds=True,
                                         collision_free=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        posed = prob["valid"]
        qs = prob["q"]
        qg = torch.where(posed[:, None], prob["q_goal"], prob["q"])  # (unposed rows: a trivial problem, same work)
        cloud = prob["xyz"][:, 2048:6144, :3]
        few = cloud[:min(B, 8)].contiguous()
        d = torch.cdist(few, few)
        d.diagonal(dim1=1, dim2=2).fill_(float("inf"))
        spacing = float(d.amin(-1).mean())
        out = {"posed": int(posed.sum()), "mean_nearest_neighbour_spacing_m": spacing}
        trunc = robot.plan_cloud_truncation(0.5 * spacing)
        out["field_build"] = timed(lambda: CloudField.build(cloud, truncation=trunc))
        field = CloudField.build(cloud, truncation=trunc)
        out["field_nodes"], out["field_truncation_m"] = list(field.shape), trunc
        pr = 0.5 * spacing
        out["plan_cloud"] = timed(lambda: robot.franka_plan_cloud(qs, qg, cloud, field=field, point_radius=pr, **kw))
        out["plan_cloud_with_field_build"] = timed(lambda: robot.franka_plan_cloud(qs, qg, cloud, point_radius=pr, **kw))
        none = cloud[:, :0]
        out["plan_cloud_no_flag_calls"] = timed(lambda: robot.franka_plan_cloud(qs, qg, none, field=field, point_radius=pr, **kw))
        out["plan_cloud_drawn_only"] = timed(lambda: robot.franka_plan_cloud(qs, qg, none, field=field, point_radius=pr, iterations=0, **kw))
        full, noflag, drawn = (out[k]["median_ms"] for k in ("plan_cloud", "plan_cloud_no_flag_calls", "plan_cloud_drawn_only"))
        out["split_ms"] = {"optimise": noflag - drawn, "validity": full - noflag, "draw_tests_refine_select": drawn}
        out["plan_primitives"] = timed(lambda: robot.franka_plan(qs, qg, cub, cyl, **kw))
        out["ratio_cloud_over_primitives"] = full / out["plan_primitives"]["median_ms"]
        st_p = robot.franka_plan(qs, qg, cub, cyl, **kw)[1]
        out["share_solved_primitives"] = float((st_p[posed] == 0).float().mean()) if int(posed.sum()) else None
        for name, radius in (("point_radius_0", 0.0), ("point_radius_half_spacing", pr)):
            f = field if radius == pr else CloudField.build(cloud, truncation=robot.plan_cloud_truncation(radius))
            traj, st = robot.franka_plan_cloud(qs, qg, cloud, field=f, point_radius=radius, **kw)
            ok = (st == 0) & posed
            rows = torch.nonzero(ok)[:, 0]
            rej = None
            if rows.numel():
                fine = torch.from_numpy(np.ascontiguousarray(
                    _refine(traj[rows].double().cpu().numpy(), 4))).float().to(dev)
                c = TorchCuboids(cub.centers[rows], cub.dims[rows], cub.quats[rows])
                y = TorchCylinders(cyl.centers[rows], cyl.radii[rows], cyl.heights[rows], cyl.quats[rows])
                rej = float(sampler.check(fine, c, y).float().mean())
            out[name] = {"point_radius_m": radius, "share_solved_cloud": float(ok[posed].float().mean()) if int(posed.sum()) else None,
                         "share_of_cloud_solved_rejected_by_primitive_check": rej}
        res["cases"][str(B)] = out
        del field, prob
        torch.cuda.empty_cache()
    # the sampler alone: 2^20 points in one environment's default grid
    g = torch.Generator(device="cpu").manual_seed(0)
    cloud = (torch.rand((1, 4096, 3), generator=g) * torch.tensor([1.8, 1.8, 1.5]) + torch.tensor([-0.9, -0.9, -0.3])).to(dev)
    field = CloudField.build(cloud, truncation=0.2)
    pts = (torch.rand((1, 1 << 20, 3), generator=g) * torch.tensor([1.8, 1.8, 1.5]) + torch.tensor([-0.9, -0.9, -0.3])).to(dev)
    res["sample_2^20_points"] = {"dist": timed(lambda: field.sample(pts)), "dist_and_grad": timed(lambda: field.sample(pts, True))}
    print(json.dumps(res))


def _refine(traj, substeps):
    """[N,T,7] float64 -> [N,(T-1) substeps + 1,7]: plain linear interpolation (the judge's own arithmetic)."""
    f = (np.arange(substeps) / substeps)[:, None]
    a, b = traj[:, :-1, None, :], traj[:, 1:, None, :]
    body = (a + f * (b - a)).reshape(traj.shape[0], -1, 7)
    return np.concatenate([body, traj[:, -1:]], 1)


if __name__ == "__main__":
    main()
