"""SA1 / SA2 ball queries alone on bench-scene clouds at B environments, event-timed.
usage: ball_query_timing.py ENTRY [B]   (ENTRY: mpx_ball_query_hits | mpx_ball_query_set | mpx_ball_query)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd")]
import torch

from mpinets_amd import _lib
from mpinets_amd.pointnet2 import furthest_point_sample
from mpinets_amd.scenes import make_problem_batch

entry = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
dev = torch.device("cuda:0")
prob = make_problem_batch(B, seed=1000, device=dev, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16,
                          scene_pool=1024, device_clouds=True)
xyz = prob["xyz"][:B].contiguous()
N = xyz.size(1)
_, xyz1 = furthest_point_sample(xyz, 512, return_xyz=True)
xyz1 = xyz1.contiguous()
_, xyz2 = furthest_point_sample(xyz1, 128, return_xyz=True)
xyz2 = xyz2.contiguous()
torch.cuda.synchronize()


def timed(name, ctr, npoint, pts, stride, n, radius):
    idx = torch.zeros((B, npoint, 128), dtype=torch.int32, device=dev)
    cnt = torch.zeros((B, npoint), dtype=torch.int32, device=dev)
    call = lambda: _lib.call(entry, _lib.ptr(ctr), 3, _lib.ptr(pts), stride, B, n, npoint, radius, 128, _lib.ptr(idx), _lib.ptr(cnt))
    call()
    torch.cuda.synchronize()
    reps = 10
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for r in range(reps):
        call()
        ev[r + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[r].elapsed_time(ev[r + 1]) for r in range(reps))
    print(f"lib {os.path.basename(_lib.LIB_PATH)} {entry} {name} B={B}: median {ts[reps // 2]:.3f} ms  min {ts[0]:.3f}  max {ts[-1]:.3f}  "
          f"mean cnt {cnt.float().mean().item():.2f}", flush=True)


timed("SA1 (6272 pts, 512 queries, r 0.05)", xyz1, 512, xyz, 4, N, 0.05)
timed("SA2 (512 pts, 128 queries, r 0.3)", xyz2, 128, xyz1, 3, 512, 0.3)
