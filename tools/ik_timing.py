"""Time mpx_franka_ik (csrc/ik.hip) on the GPU: 8192 problems, 64 starts x 64 iterations, in free space and against
the benchmark's tabletop scenes.  HIP events around each call, 3 untimed calls, then the median of 10 with the
spread (min .. max).  ``--host N`` also times the float64 restatement (tests/float64_ik.py) on N problems on the CPU,
for orientation only.

    python tools/ik_timing.py [--envs 8192] [--iterations 64] [--host 0]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--host", type=int, default=0, help="problems for the float64 restatement on the CPU (0: skip)")
    args = ap.parse_args()
    from mpinets_amd import franka_tables as ft, robot, scenes
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    dev = torch.device("cuda:0")
    B = args.envs
    q = torch.from_numpy(scenes.random_configurations(B, 0)).to(dev)
    poses = robot.frames_to_matrix(robot.franka_fk(q)[:, ft.LINK_ID["right_gripper"]])
    scn = {k: torch.from_numpy(v).to(dev) for k, v in scenes.make_scenes(B, 0).items()}
    cub = TorchCuboids(scn["cuboid_centers"], scn["cuboid_dims"], scn["cuboid_quats"])
    cyl = TorchCylinders(scn["cylinder_centers"], scn["cylinder_radii"], scn["cylinder_heights"], scn["cylinder_quats"])
    res = {"envs": B, "seeds": robot.IK_SEEDS, "iterations": args.iterations}
    cases = {"free_space": lambda **kw: robot.franka_ik(poses, iterations=args.iterations, **kw),
             "tabletop_scenes": lambda **kw: robot.franka_ik(poses, cub, cyl, iterations=args.iterations, **kw)}
    for name, fn in cases.items():
        res[name] = timed(fn)
        res[name]["share_solved"] = float((fn()[1] == 0).float().mean())
    res["tabletop_scenes_all_seeds_tested"] = timed(lambda: cases["tabletop_scenes"](return_all=True))
    res["one_iteration_free_space"] = timed(lambda: robot.franka_ik(poses, iterations=1))
    if args.host:
        import float64_ik as f64

        t0 = time.time()
        f64.solve(poses[:args.host].cpu().numpy(), iterations=args.iterations)
        res["float64_restatement_host"] = {"envs": args.host, "seconds": time.time() - t0, "threads": torch.get_num_threads()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
