"""Time the reference's scenes (csrc/scene_gen_reference.hip, ``mpx_scene_generate_reference``) beside the stand-ins
(``mpx_scene_generate``, whose kernel this tree did not touch) and the host generators, on one machine.

8192 scenes at M1 = 40, M2 = 16, S = 8, per kind and mixed:

  * device: the launch alone into buffers that exist, by HIP events: 3 untimed calls, then the median of 10 with the spread
    (min .. max), as tools/ik_timing.py;
  * host: wall clock of ``make_task_scenes`` (one run);
  * the mean live cuboids and cylinders per kind, old and new: density is what the step time follows;
  * the new kernel's register, spill and LDS figures from the built library's code object (tests/test_code_objects.py's
    reader, as a library).

Recorded, not asserted.

    python tools/scene_reference_timing.py [--envs 8192]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from ik_timing import timed  # noqa: E402
from mpinets_amd import scenes  # noqa: E402

OLD = ("tabletop", "cubby", "dresser")
NEW = scenes.REFERENCE_KINDS
M1, M2, S = 40, 16, 8
KEYS = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights",
        "cylinder_quats", "support_boxes", "support_kind")


def kernel_figures(name):
    from test_code_objects import LIB, kernel_metadata

    (f,) = [f for n, f in kernel_metadata(LIB).items() if name in n]
    return {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                               ".private_segment_fixed_size", ".group_segment_fixed_size")}


def case(kinds, B, dev):
    from mpinets_amd import _lib

    out = scenes.make_scenes_device(B, 0, kinds, M1, M2, S=S, device=dev)
    kind = torch.tensor([scenes.SCENE_KIND_CODES[k] for k in kinds], dtype=torch.int32)[torch.arange(B) % len(kinds)].to(dev)
    tail = (B, M1, M2, S, 0, 0, *(_lib.ptr(out[k]) for k in KEYS))
    res = {}
    if any(k in OLD for k in kinds):
        res["mpx_scene_generate"] = timed(lambda: _lib.call("mpx_scene_generate", _lib.ptr(kind), None, *tail))
    if any(k in NEW for k in kinds):
        res["mpx_scene_generate_reference"] = timed(lambda: _lib.call("mpx_scene_generate_reference", _lib.ptr(kind), None, None, *tail))
    res["make_scenes_device"] = timed(lambda: scenes.make_scenes_device(B, 0, kinds, M1, M2, S=S, device=dev))
    t0 = time.perf_counter()
    host = scenes.make_task_scenes(B, 0, kinds, M1, M2, S)
    res["host_make_task_scenes_s"] = time.perf_counter() - t0
    for name, scn in (("device", {k: v.cpu().numpy() for k, v in out.items()}), ("host", host)):
        res[f"mean_live_cuboids_{name}"] = float((scn["cuboid_dims"] != 0).any(-1).sum(1).mean())
        res[f"mean_live_cylinders_{name}"] = float((scn["cylinder_radii"][..., 0] != 0).sum(1).mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    res = {"shape": {"B": args.envs, "M1": M1, "M2": M2, "S": S},
           "kernels": {"scene_reference_kernel": kernel_figures("scene_reference_kernel"),
                       "scene_generate_kernel": kernel_figures("scene_generate_kernel")}, "cases": {}}
    for kinds in [(k,) for k in OLD + NEW] + [OLD, NEW, OLD + NEW]:
        res["cases"]["+".join(kinds)] = case(kinds, args.envs, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
