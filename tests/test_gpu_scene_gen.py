"""``mpx_scene_generate`` (csrc/scene_gen.hip, ``scenes.make_scenes_device``) on the GPU against its float64 restatement
(tests/float64_scene_gen.py), and ``make_problem_batch(scene_source="device")``: sharding and the pipeline end to end.

Launches: B in {1, 5, 9} (a lone scene, a part-filled last workgroup of four, the three kinds cycling) at ``scene_offset`` = 3
times (M1, M2, S) in {(16, 16, 8), (64, 64, 64), (3, 0, 1), (5, 2, 4), (40, 16, 8)}; one at ``scene_offset`` = 2^32 - 9; one
with explicit ``scene_ids`` (unordered, with a repeat); one with a kind code 7; one with NULL supports and S = 0.  Every
output buffer is pre-filled with NaN (``support_kind`` with -1).  Discrete results are compared exactly, every other float
within ``FLOAT_TOL`` (derived in tests/test_scene_gen_host.py, not measured).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_scene_gen as fsg  # noqa: E402
from test_gpu_plan import dev, prims_of  # noqa: E402
from test_scene_gen_host import FLOAT_TOL, SHAPES, check_structure  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20
KINDS3 = ("tabletop", "cubby", "dresser")
FLOAT_KEYS = fsg.PRIMITIVE_KEYS + ("support_boxes",)


def launch(kind, B, m1, m2, s, scene_offset=0, scene_ids=None, seed=SEED):
    """The C entry itself on NaN-filled buffers -> numpy arrays under ``make_task_scenes``' keys (``s`` = 0: NULL supports)."""
    from mpinets_amd import _lib

    def nan(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())

    out = {"cuboid_centers": nan(B, m1, 3), "cuboid_dims": nan(B, m1, 3), "cuboid_quats": nan(B, m1, 4),
           "cylinder_centers": nan(B, m2, 3), "cylinder_radii": nan(B, m2, 1), "cylinder_heights": nan(B, m2, 1),
           "cylinder_quats": nan(B, m2, 4)}
    if s:
        out.update(support_boxes=nan(B, s, 12), support_kind=torch.full((B, s), -1, dtype=torch.int32, device=dev()))
    k = torch.as_tensor(np.asarray(kind), dtype=torch.int32, device=dev())
    ids = None if scene_ids is None else torch.as_tensor(np.asarray(scene_ids), dtype=torch.int64, device=dev())
    _lib.call("mpx_scene_generate", _lib.ptr(k), _lib.ptr(ids), B, m1, m2, s, seed, int(scene_offset),
              *(_lib.ptr(out[key]) for key in fsg.PRIMITIVE_KEYS), _lib.ptr(out.get("support_boxes")), _lib.ptr(out.get("support_kind")))
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in out.items()}


def compare(got, kind, ids, m1, m2, s, seed=SEED):
    """The kernel's arrays against the restatement -> the largest deviation of a float."""
    kind, ids = np.asarray(kind), np.asarray(ids, np.int64)
    ref = fsg.generate(kind, ids, m1, m2, s, seed)
    assert set(got) == set(ref)
    for key in got:
        assert got[key].shape == ref[key].shape and not np.isnan(got[key].astype(np.float64)).any(), key  # (every element written)
    # exact: the live rows of every array, the support kinds, the padding and the structure the contract promises
    for a, b in zip(fsg.live_rows(got), fsg.live_rows(ref)):
        assert (a is None and b is None) or np.array_equal(a, b)
    check_structure(got, kind, m1, m2, s)
    cub, cyl, sup = fsg.live_rows(ref)
    if s:
        assert np.array_equal(got["support_kind"], ref["support_kind"])
    # exact: what the contract copies or sets
    g = {key: got[key].astype(np.float64) for key in FLOAT_KEYS if key in got}
    mount = np.full(len(kind), -1)
    for b in np.flatnonzero(kind == fsg.TABLETOP):  # the mount table stands behind the front table and the side table
        mount[b] = 2 if ref["cuboid_dims"][b, 1, 0] == fsg.f(0.9) else 1
        rows = slice(0, mount[b] + 1)
        assert np.array_equal(g["cuboid_quats"][b, rows], ref["cuboid_quats"][b, rows])  # (identity)
        assert (g["cuboid_dims"][b, rows, 2] == fsg.f(0.05)).all()  # thick
        assert g["cuboid_centers"][b, 0, 1] == 0
        for key in ("cuboid_centers", "cuboid_dims"):
            assert np.array_equal(g[key][b, mount[b]], ref[key][b, mount[b]]), (key, b)  # the mount table's constants
        if mount[b] == 2:
            assert g["cuboid_centers"][b, 1, 0] == 0 and g["cuboid_dims"][b, 1, 0] == fsg.f(0.9)
        if s:  # a surface copies its cuboid, the weight is the float32 product of its first two dims
            for r in range(min(s, mount[b])):
                assert np.array_equal(got["support_boxes"][b, r, :6], np.concatenate([got["cuboid_centers"][b, r], got["cuboid_dims"][b, r]]))
                assert got["support_boxes"][b, r, 11] == np.float32(got["cuboid_dims"][b, r, 0] * got["cuboid_dims"][b, r, 1])
                assert np.array_equal(got["support_boxes"][b, r, 6:11], [1, 0, 0, 0, 0])
    if s:
        volumes = ref["support_kind"] == fsg.VOLUME
        assert (got["support_boxes"][volumes][:, 11] == 1).all()
        assert (got["support_boxes"][(kind == fsg.CUBBY)[:, None] & volumes][:, 10] == 0).all()
    # within the bar: every float
    worst = 0.0
    for key in g:
        d = np.abs(g[key] - ref[key]).max() if g[key].size else 0.0
        worst = max(worst, d)
        assert d <= FLOAT_TOL, (key, d)
    return worst


def test_kernel_matches_float64_on_every_launch_shape():
    worst = 0.0
    for m1, m2, s in SHAPES:
        for B in (1, 5, 9):
            ids = 3 + np.arange(B)
            kind = ids % 3
            worst = max(worst, compare(launch(kind, B, m1, m2, s, scene_offset=3), kind, ids, m1, m2, s))
    print(f"scene generation vs float64: largest deviation of a float {worst:.3e} (bar {FLOAT_TOL:.1e})")


def test_last_ids_of_the_counter_range():
    ids = (1 << 32) - 9 + np.arange(9)
    kind = ids % 3
    d = compare(launch(kind, 9, 16, 16, 8, scene_offset=(1 << 32) - 9), kind, ids, 16, 16, 8)
    print(f"scene ids up to 2^32 - 1: largest deviation {d:.3e}")


def test_explicit_scene_ids_and_a_repeat():
    ids = np.array([40, 7, 123456789, 7, 0, 8, 41], np.int64)
    kind = ids % 3
    got = launch(kind, len(ids), 16, 16, 8, scene_offset=1000, scene_ids=ids)  # (the offset is not used with ids)
    compare(got, kind, ids, 16, 16, 8)
    for key, v in got.items():
        assert np.array_equal(v[1], v[3]), key  # the repeated scene, bit for bit
    again = launch(kind[[1]], 1, 16, 16, 8, scene_offset=7)
    for key, v in got.items():
        assert np.array_equal(v[1], again[key][0]), key  # ... and the scene of ``scene_offset`` = 7


def test_unknown_kind_is_an_empty_scene():
    kind = np.array([0, 7, 1, -1, 2])
    ids = 3 + np.arange(5)
    got = launch(kind, 5, 16, 16, 8, scene_offset=3)
    compare(got, kind, ids, 16, 16, 8)
    for b in (1, 3):
        assert (got["cuboid_dims"][b] == 0).all() and (got["cylinder_radii"][b] == 0).all() and (got["support_kind"][b] == 0).all()
        assert (got["support_boxes"][b] == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]).all()
        assert (got["cuboid_quats"][b] == [1, 0, 0, 0]).all() and (got["cuboid_centers"][b] == 0).all()


def test_without_supports():
    ids = 3 + np.arange(9)
    kind = ids % 3
    got = launch(kind, 9, 40, 16, 0, scene_offset=3)
    assert set(got) == set(fsg.PRIMITIVE_KEYS)
    compare(got, kind, ids, 40, 16, 0)
    with_supports = launch(kind, 9, 40, 16, 8, scene_offset=3)
    for key in got:
        assert np.array_equal(got[key], with_supports[key]), key


def test_wrapper_keys_kinds_and_offsets():
    """``make_scenes_device``: ``make_scenes``' / ``make_task_scenes``' keys, shapes and dtypes; the kind of id g is
    ``kinds[g % len(kinds)]``; ``env_offset`` and ``scene_ids`` name the same scenes."""
    from mpinets_amd import scenes

    host = scenes.make_task_scenes(6, 0, KINDS3, 40, 16, 8)
    a = scenes.make_scenes_device(6, SEED, KINDS3, 40, 16, S=8, env_offset=4)
    assert set(a) == set(host)
    for key, v in host.items():
        assert tuple(a[key].shape) == v.shape and a[key].dtype == torch.from_numpy(v).dtype and a[key].device == dev(), key
    plain = scenes.make_scenes_device(6, SEED, KINDS3, 40, 16, env_offset=4)
    assert set(plain) == set(scenes.make_scenes(1, 0, KINDS3, 40, 16))
    ids = 4 + np.arange(6)
    compare({k: v.cpu().numpy() for k, v in a.items()}, ids % 3, ids, 40, 16, 8)
    b = scenes.make_scenes_device(6, SEED, KINDS3, 40, 16, S=8, scene_ids=torch.from_numpy(ids))
    assert all(torch.equal(a[k], b[k]) for k in a) and all(torch.equal(a[k], plain[k]) for k in plain)


def test_shards_and_scene_pool():
    """Rows 5 .. 8 of a 16-row batch, generated alone, are those rows bit for bit (primitives, supports, scene cloud); with
    ``scene_pool`` = 3 rows g and g + 3 hold the same primitives."""
    from mpinets_amd import scenes

    kw = dict(seed=3, kinds=KINDS3, M1=16, M2=16, scene_source="device", device_clouds=True, problems="task", collision_free=True)
    whole = scenes.make_problem_batch(16, **kw)
    part = scenes.make_problem_batch(4, env_offset=5, total_envs=16, **kw)
    for key in fsg.PRIMITIVE_KEYS + ("support_boxes", "support_kind"):
        assert torch.equal(part[key], whole[key][5:9]), key
    lo, hi = scenes.NUM_ROBOT_POINTS, scenes.NUM_ROBOT_POINTS + scenes.NUM_OBSTACLE_POINTS
    assert torch.equal(part["xyz"][:, lo:hi], whole["xyz"][5:9, lo:hi])
    plain = scenes.make_problem_batch(4, env_offset=5, total_envs=16, seed=3, kinds=KINDS3, scene_source="device", device_clouds=True)
    for key in fsg.PRIMITIVE_KEYS:
        assert torch.equal(plain[key], whole[key][5:9]), key
    assert "support_boxes" not in plain
    pool = scenes.make_problem_batch(8, seed=3, kinds=KINDS3, scene_pool=3, scene_source="device", device_clouds=True)
    for key in fsg.PRIMITIVE_KEYS:
        assert torch.equal(pool[key][:5], pool[key][3:8]) and torch.equal(pool[key][:3], whole[key][:3]), key
    assert not torch.equal(pool["xyz"][0, lo:hi], pool["xyz"][3, lo:hi])  # (every environment still gets its own cloud draw)


def test_pipeline_end_to_end_on_device_scenes():
    """48 task problems over the three kinds from both sources: the device source's share of valid rows is at least half the
    host source's (the reference here; the two draw different scenes from one distribution, and 48 rows of a share near 0.9
    scatter by about 0.1), and ``task_candidates`` finds a free candidate on a device scene of every kind."""
    from mpinets_amd import scenes, solvers

    kw = dict(kinds=KINDS3, M1=40, M2=16, collision_free=True, problems="task", device_clouds=True)
    host = scenes.make_problem_batch(48, **kw)
    device = scenes.make_problem_batch(48, scene_source="device", **kw)
    share_host, share_device = float(host["valid"].float().mean()), float(device["valid"].float().mean())
    print(f"valid share of 48 task problems: host scenes {share_host:.3f}, device scenes {share_device:.3f}")
    assert set(device) == set(host)
    assert share_device >= 0.5 * share_host
    cub, cyl = prims_of({k: device[k] for k in fsg.PRIMITIVE_KEYS})
    count = solvers.task_candidates(device["support_boxes"], device["support_kind"], cub, cyl)[3].cpu().numpy()
    for i, name in enumerate(KINDS3):
        assert (count[i::3] > 0).any(), name
