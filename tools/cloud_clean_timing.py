"""Time mpx_cloud_clean (csrc/cloud_clean.hip) on the GPU: 1 and 16 synthetic 640 x 480 captures (307 200 rows each: a
jittered table plane reaching past the workspace, object blobs, points around the robot's spheres, speckle, NaN rows --
tests/float64_cloud_clean.py's generator) cleaned down to 4096 rows, in two forms:

  crop + draw     what the reference's clean_point_cloud does (planning_node.py:187-228)
  all four        + robot removal (57 spheres, margin 2 cm) + outlier removal (4 neighbours within the radius the
                  generator derives from the table's density; the share of alive1 it removes is printed)

and, for the split, the filter-only calls (no draw) of both.  HIP events around ``clean_point_clouds`` as a user calls it
(allocations and the read-back of the counts included), 3 untimed calls, then the median of 10 with the spread.  In the
same run the reference's own NumPy crop + ``np.random.choice`` is timed on the host for the crop + draw form (wall clock,
one capture at a time, as the reference runs it).  Also printed: the bytes every pass moves, from the shapes and the
measured row counts.

    python tools/cloud_clean_timing.py            # the table
    python tools/cloud_clean_timing.py --once 16  # five calls of the all-four form and nothing else (for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ik_timing import timed  # noqa: E402

W, H, N_OUT = 640, 480, 4096


def reference_clean(xyz, n_out):
    """planning_node.py:201-228 restated for timing: two box masks, their union, np.random.choice without replacement."""
    from mpinets_amd.capture import REFERENCE_WORKSPACE as ws

    mask = np.zeros(len(xyz), bool)
    for b in ws:
        mask |= np.logical_and.reduce((xyz[:, 0] > b[0], xyz[:, 0] < b[3], xyz[:, 1] > b[1], xyz[:, 1] < b[4],
                                       xyz[:, 2] > b[2], xyz[:, 2] < b[5]))
    kept = xyz[mask]
    return kept[np.random.choice(len(kept), size=n_out, replace=False)]


def captures(B):
    import float64_cloud_clean as f64

    rng = np.random.default_rng(0)
    q = f64.capture_configurations(B, 0)
    centres, radii = f64.oracle_centres(q).astype(np.float64), f64.sphere_radii().astype(np.float64)
    cloud = np.zeros((B, W * H, 3), np.float32)
    for b in range(B):
        cloud[b], r = f64.synthetic_capture(W * H, centres[b], radii, rng)
    return cloud, q, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--once", type=int, default=0, metavar="B", help="five calls of the all-four form on B captures, no timing")
    args = ap.parse_args()
    import float64_cloud_clean as f64
    from mpinets_amd import _lib
    from mpinets_amd.capture import clean_point_clouds
    from mpinets_amd.robot import FrankaCollisionSampler

    dev = torch.device("cuda:0")
    s = FrankaCollisionSampler(dev, with_base_link=True)
    lib = _lib.load()
    res = {"rows": W * H, "n_out": N_OUT, "spheres": s.num_spheres, "min_neighbors": f64.MIN_NEIGHBORS,
           "robot_margin": f64.ROBOT_MARGIN}
    for B in ([args.once] if args.once else [1, 16]):
        cloud_np, q_np, r = captures(B)
        cloud, q = torch.from_numpy(cloud_np).to(dev), torch.from_numpy(q_np).to(dev)
        full = dict(q=q, collision_sampler=s, robot_margin=f64.ROBOT_MARGIN, outlier_radius=r, min_neighbors=f64.MIN_NEIGHBORS)
        if args.once:
            for seed in range(5):
                clean_point_clouds(cloud, N_OUT, seed=seed, **full)
            torch.cuda.synchronize()
            continue
        out = {"envs": B, "outlier_radius": r, "scratch_bytes": int(lib.mpx_cloud_clean_scratch(B, W * H))}
        out["crop_draw"] = timed(lambda: clean_point_clouds(cloud, N_OUT))
        out["crop_only"] = timed(lambda: clean_point_clouds(cloud, 0))
        out["all_four_draw"] = timed(lambda: clean_point_clouds(cloud, N_OUT, **full))
        out["all_four_only"] = timed(lambda: clean_point_clouds(cloud, 0, **full))
        reason, count = clean_point_clouds(cloud, 0, **full)
        n = np.stack([np.bincount(row, minlength=5) for row in reason.cpu().numpy()]).sum(axis=0)
        n1 = int(n[0] + n[4])
        out["rows_by_reason"] = n.tolist()
        out["share_of_alive1_removed_as_outliers"] = float(n[4]) / max(n1, 1)
        assert int(count.sum()) == int(n[0])
        rows = B * W * H
        out["bytes"] = {  # what each pass reads + writes, from the shapes and the measured row counts
            "classify": rows * 12 + rows,
            "grid (zeroing the counters, at most)": B * 262144 * 4,
            "bin count": rows + n1 * 12 + n1 * 4,
            "scan (at most)": 2 * B * 262144 * 4,
            "bin scatter": rows + n1 * 12 + n1 * 4 + n1 * 16,
            "neighbours (own row + reason; the runs it walks come on top)": n1 * 16 + int(n[4]),
            "draw": 4 * rows + B * N_OUT * (12 + 12 + 4),
        }
        host = []
        for rep in range(13):
            t0 = time.perf_counter()
            for b in range(B):
                reference_clean(cloud_np[b], N_OUT)
            host.append((time.perf_counter() - t0) * 1e3)
        host = host[3:]
        out["numpy_crop_draw_host"] = {"median_ms": float(np.median(host)), "min_ms": min(host), "max_ms": max(host), "reps": 10}
        res[f"B{B}"] = out
    if not args.once:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
