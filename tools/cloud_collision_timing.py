"""Time mpx_franka_cloud_collision (csrc/cloud_collision.hip) on the GPU: 8192 trajectories x 50 waypoints x 56 spheres
against the 4096 scene rows of the policy slab, read in place (``xyz[:, 2048:6144, :3]``), for tabletop and for mixed
tabletop / cubby / dresser slabs, plus one 1024-environment case.  Per case: the full form (min_dist + nearest), the
flags-only form with the box cull and early stop (the default) and without them (MPX_VARIANT_CLOUD_CULL = 0), and the
primitive check (``FrankaCollisionSampler.check``) on the same trajectories as context.  Two kinds of trajectories:
straight joint-space lines between uniform configurations (most of them cross the scene: the early stop decides) and short
lines around the neutral pose (most of them free: every surviving point is visited, the box cull decides).
HIP events around each call, 3 untimed calls, then the median of 10 with the spread (min .. max).  The timed call is
``check_cloud`` as a user makes it (the flag / output allocations included).

    python tools/cloud_collision_timing.py [--envs 8192]
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

VARIANT_CLOUD_CULL = 3  # MPX_VARIANT_CLOUD_CULL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--waypoints", type=int, default=50)
    args = ap.parse_args()
    from mpinets_amd import _lib, franka_tables as ft, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders
    from mpinets_amd.robot import FrankaCollisionSampler

    dev = torch.device("cuda:0")
    T = args.waypoints
    s = FrankaCollisionSampler(dev)
    lib = _lib.load()
    res = {"waypoints": T, "spheres": s.num_spheres, "points": 4096}

    def trajectories(B, kind):
        if kind == "crossing":
            return torch.from_numpy(scenes.linear_trajectories(B, T, 0)).to(dev)
        rng = np.random.default_rng(1)
        a, b = (np.asarray(ft.DEFAULT_Q, np.float32)[None] + rng.uniform(-0.2, 0.2, (B, 7)).astype(np.float32) for _ in range(2))
        w = np.linspace(0.0, 1.0, T, dtype=np.float32)[None, :, None]
        return torch.from_numpy((a[:, None] * (1 - w) + b[:, None] * w).astype(np.float32)).to(dev)

    def case(name, B, kinds, M1, M2):
        prob = scenes.make_problem_batch(B, seed=0, kinds=kinds, M1=M1, M2=M2, scene_pool=1024, device_clouds=True)
        cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
        cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
        rows = prob["xyz"][:, 2048:6144, :3]  # the slab's scene rows, in place
        for kind in ("crossing", "near_neutral"):
            q = trajectories(B, kind)
            out = {"envs": B}
            out["full"] = timed(lambda: s.check_cloud(q, rows, return_distance=True, return_nearest=True))
            out["flags_only_cull"] = timed(lambda: s.check_cloud(q, rows))
            assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 0) == 0
            try:
                out["flags_only_no_cull"] = timed(lambda: s.check_cloud(q, rows))
                plain = s.check_cloud(q, rows)
            finally:
                assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 1) == 0
            out["primitive_check"] = timed(lambda: s.check(q, cub, cyl))
            flags = s.check_cloud(q, rows)
            full = s.check_cloud(q, rows, return_distance=True)[0]
            assert torch.equal(flags, plain) and torch.equal(flags, full)
            out["share_hit_cloud"] = float(flags.float().mean())
            out["share_hit_primitives"] = float(s.check(q, cub, cyl).float().mean())
            res[f"{name}_{kind}"] = out

    case("tabletop", args.envs, ("tabletop",), 16, 16)
    case("mixed", args.envs, ("tabletop", "cubby", "dresser"), 40, 16)
    case("mixed_1024", 1024, ("tabletop", "cubby", "dresser"), 40, 16)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
