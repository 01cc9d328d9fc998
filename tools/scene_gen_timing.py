"""Time the two scene sources on one machine: the host generators (``scenes.make_task_scenes``, one numpy rng, one Python call
per scene, plus the upload of the arrays) and the device generator (csrc/scene_gen.hip, ``scenes.make_scenes_device``).

For B in --envs (default 256 8192 65536) mixed tabletop / cubby / dresser scenes at M1 = 40, M2 = 16, S = 8:

  * host: wall clock of ``make_task_scenes(B)`` and of moving its nine arrays to the GPU (one run: it takes seconds);
  * device: ``make_scenes_device(B, S=8)`` as a user calls it (the kind codes, nine ``torch.empty`` and the launch), and the
    launch alone into buffers that exist (``mpx_scene_generate``), by HIP events: 3 untimed calls, then the median of 10 with
    the spread (min .. max), as tools/ik_timing.py.

Then the case the device source exists for, the last eighth of a 65536-row batch (``env_offset`` = 57344, B = 8192): the host
has to walk its rng through all 65536 scenes and keeps 8192, the device generates the 8192.

The two sources draw different scenes of the same distributions; the numbers say what each costs, not that they agree.
The kernel's register and LDS figures are read from the built library's code object (tests/test_code_objects.py's reader).

    python tools/scene_gen_timing.py [--envs 256 8192 65536]
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
from mpinets_amd import scenes  # noqa: E402

MIXED = ("tabletop", "cubby", "dresser")
M1, M2, S = 40, 16, 8


def kernel_figures():
    from test_code_objects import LIB, kernel_metadata

    (f,) = [f for n, f in kernel_metadata(LIB).items() if "scene_generate_kernel" in n]
    return {k.lstrip("."): int(f[k]) for k in (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
                                               ".private_segment_fixed_size", ".group_segment_fixed_size")}


def host_source(total, rows, dev):
    """The host's way to the scenes ``rows`` of a batch of ``total``: generate all of them, keep the rows, upload."""
    t0 = time.perf_counter()
    scn = scenes.make_task_scenes(total, 0, MIXED, M1, M2, S)
    t1 = time.perf_counter()
    out = {k: torch.from_numpy(np.ascontiguousarray(v[rows])).to(dev) for k, v in scn.items()}
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"generate_s": t1 - t0, "upload_s": t2 - t1, "total_s": t2 - t0, "scenes_generated": total, "scenes_kept": len(out["support_kind"])}


def device_source(B, env_offset, dev):
    from mpinets_amd import _lib

    res = {"make_scenes_device": timed(lambda: scenes.make_scenes_device(B, 0, MIXED, M1, M2, S=S, device=dev, env_offset=env_offset))}
    out = scenes.make_scenes_device(B, 0, MIXED, M1, M2, S=S, device=dev, env_offset=env_offset)
    kind = torch.tensor([0, 1, 2], dtype=torch.int32)[(env_offset + torch.arange(B)) % 3].to(dev)
    keys = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights",
            "cylinder_quats", "support_boxes", "support_kind")
    res["mpx_scene_generate"] = timed(lambda: _lib.call("mpx_scene_generate", _lib.ptr(kind), None, B, M1, M2, S, 0, env_offset,
                                                        *(_lib.ptr(out[k]) for k in keys)))
    res["bytes_written"] = int(sum(out[k].numel() * out[k].element_size() for k in keys))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 8192, 65536])
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    res = {"shape": {"kinds": MIXED, "M1": M1, "M2": M2, "S": S}, "kernel": kernel_figures(), "cases": {}}
    for B in args.envs:
        res["cases"][str(B)] = {"host": host_source(B, np.arange(B), dev), "device": device_source(B, 0, dev)}
    total, B, off = 65536, 8192, 57344
    res["last_eighth_of_65536"] = {"host": host_source(total, off + np.arange(B), dev), "device": device_source(B, off, dev)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
