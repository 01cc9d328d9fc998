"""``mpx_scene_generate_reference`` (csrc/scene_gen_reference.hip, ``scenes.make_scenes_device``) on the GPU against its
float64 restatement (tests/float64_scene_reference.py), and the new kinds through ``make_problem_batch``: mixed batches,
shards, the per-row merge and the pipeline end to end.

Launches: B in {1, 5, 9} with the kinds cycling 3, 4, 5 at ``scene_offset`` = 3 times (M1, M2, S) in {(7, 0, 1), (8, 2, 4),
(16, 16, 8), (64, 64, 64)} (the first two force every overflow path); one at ``scene_offset`` = 2^32 - 9; one with explicit
``scene_ids`` (unordered, with a repeat); ``merge_pockets`` as NULL, as all twelve ordered pairs and as (-1, -1).  Every
output buffer is pre-filled with NaN (``support_kind`` with -1).  Discrete results are compared exactly, every other float
within ``FLOAT_TOL_REF``; tabletop scenes within ``FRAGILE_MARGIN`` of a float decision are left out of the comparison, at
most 1 in 20 (both derived in tests/test_scene_reference_host.py, which also counts them for this seed on the CPU).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_scene_gen as fsg  # noqa: E402
import float64_scene_reference as fsr  # noqa: E402
from test_gpu_plan import dev, prims_of  # noqa: E402
from test_gpu_scene_gen import launch as launch_old  # noqa: E402
from test_scene_reference_host import (FLOAT_TOL_REF, FRAGILE_CAP, GPU_SEED, KINDS, SHAPES, check_structure, fragile,  # noqa: E402
                                       gpu_cases)

pytestmark = pytest.mark.gpu

SEED = GPU_SEED
FLOAT_KEYS = fsg.PRIMITIVE_KEYS + ("support_boxes",)
COUNT = {"compared": 0, "left out": 0}  # tabletop scenes over the whole module


def nan_buffers(B, m1, m2, s):
    def nan(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())

    out = {"cuboid_centers": nan(B, m1, 3), "cuboid_dims": nan(B, m1, 3), "cuboid_quats": nan(B, m1, 4),
           "cylinder_centers": nan(B, m2, 3), "cylinder_radii": nan(B, m2, 1), "cylinder_heights": nan(B, m2, 1),
           "cylinder_quats": nan(B, m2, 4)}
    if s:
        out.update(support_boxes=nan(B, s, 12), support_kind=torch.full((B, s), -1, dtype=torch.int32, device=dev()))
    return out


def launch(kind, B, m1, m2, s, scene_offset=0, scene_ids=None, merge_pockets=None, seed=SEED, out=None):
    """The C entry itself on NaN-filled buffers (or on ``out``) -> numpy arrays under ``make_task_scenes``' keys."""
    from mpinets_amd import _lib

    out = nan_buffers(B, m1, m2, s) if out is None else out
    k = torch.as_tensor(np.asarray(kind), dtype=torch.int32, device=dev())
    ids = None if scene_ids is None else torch.as_tensor(np.asarray(scene_ids), dtype=torch.int64, device=dev())
    mp = None if merge_pockets is None else torch.as_tensor(np.asarray(merge_pockets), dtype=torch.int32, device=dev()).contiguous()
    _lib.call("mpx_scene_generate_reference", _lib.ptr(k), _lib.ptr(ids), _lib.ptr(mp), B, m1, m2, s, seed, int(scene_offset),
              *(_lib.ptr(out[key]) for key in fsg.PRIMITIVE_KEYS), _lib.ptr(out.get("support_boxes")), _lib.ptr(out.get("support_kind")))
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in out.items()}


def compare(got, kind, ids, m1, m2, s, merge_pockets=None, seed=SEED):
    """The kernel's arrays against the restatement -> the largest deviation of a float.  Rows of other kinds must still hold
    the NaN / -1 they were filled with (the restatement returns exactly that for them)."""
    kind, ids = np.asarray(kind), np.asarray(ids, np.int64)
    ref, aux = fsr.generate(kind, ids, m1, m2, s, seed, merge_pockets=merge_pockets, aux=True)
    assert set(got) == set(ref)
    own = np.isin(kind, (3, 4, 5))
    for key in got:
        assert got[key].shape == ref[key].shape, key
        assert not np.isnan(got[key][own].astype(np.float64)).any(), key  # (every element of an own row written)
        if got[key].dtype == np.int32:
            assert (got[key][~own] == -1).all(), key  # (every other row untouched)
        else:
            assert np.isnan(got[key][~own]).all(), key
    keep = own.copy()
    if 3 in aux:
        frag = fragile(aux[3])
        keep[aux[3]["rows"][frag]] = False
        COUNT["compared"] += len(frag)
        COUNT["left out"] += int(frag.sum())
    check_structure(got, kind, m1, m2, s)  # (holds for fragile scenes too)
    g = {key: got[key][keep] for key in got}
    r = {key: ref[key][keep] for key in ref}
    for a, b in zip(fsg.live_rows(g), fsg.live_rows(r)):
        assert (a is None and b is None) or np.array_equal(a, b)  # exact: the live rows of every array
    if s:
        assert np.array_equal(g["support_kind"], r["support_kind"])
        volumes = r["support_kind"] == fsr.VOLUME
        assert (g["support_boxes"][volumes][:, 11] == 1).all() and (g["support_boxes"][volumes][:, 10] == 0).all()
    worst = 0.0
    for key in FLOAT_KEYS:
        if key in g and g[key].size:
            d = np.abs(g[key].astype(np.float64) - r[key]).max()
            worst = max(worst, d)
            assert d <= FLOAT_TOL_REF, (key, d)
    return worst


def test_kernel_matches_float64_on_every_launch_shape():
    worst = 0.0
    for m1, m2, s in SHAPES:
        for B in (1, 5, 9):
            ids = 3 + np.arange(B)
            kind = 3 + ids % 3
            worst = max(worst, compare(launch(kind, B, m1, m2, s, scene_offset=3), kind, ids, m1, m2, s))
    print(f"reference scenes vs float64: largest deviation of a float {worst:.3e} (bar {FLOAT_TOL_REF:.1e})")


def test_last_ids_of_the_counter_range():
    ids = (1 << 32) - 9 + np.arange(9)
    kind = 3 + ids % 3
    d = compare(launch(kind, 9, 16, 16, 8, scene_offset=(1 << 32) - 9), kind, ids, 16, 16, 8)
    print(f"scene ids up to 2^32 - 1: largest deviation {d:.3e}")


def test_explicit_scene_ids_and_a_repeat():
    ids = gpu_cases()[-1][0]
    kind = 3 + ids % 3
    got = launch(kind, len(ids), 16, 16, 8, scene_offset=1000, scene_ids=ids)  # (the offset is not used with ids)
    compare(got, kind, ids, 16, 16, 8)
    for key, v in got.items():
        assert np.array_equal(v[1], v[3]), key  # the repeated scene, bit for bit
    again = launch(kind[[1]], 1, 16, 16, 8, scene_offset=7)
    for key, v in got.items():
        assert np.array_equal(v[1], again[key][0]), key  # ... and the scene of ``scene_offset`` = 7


def test_merge_pockets_every_ordered_pair_unmerged_and_drawn():
    pairs = [(a, b) for a in range(4) for b in range(4) if a != b] + [(-1, -1), (0, 4), (2, 2)]  # (the last two: unmerged too)
    B = len(pairs)
    ids = 50 + np.arange(B)
    kind = np.full(B, 5)
    got = launch(kind, B, 8, 2, 4, scene_offset=50, merge_pockets=pairs)
    compare(got, kind, ids, 8, 2, 4, merge_pockets=pairs)
    plates = (got["cuboid_dims"] != 0).any(-1).sum(1)
    assert [int(n) for n in plates] == [7 - ((a >> 1) != (b >> 1)) - ((a & 1) != (b & 1)) for a, b in pairs[:12]] + [7, 7, 7]
    drawn = launch(kind, B, 8, 2, 4, scene_offset=50)  # NULL: every scene draws its pair
    compare(drawn, kind, ids, 8, 2, 4)
    assert ((drawn["cuboid_dims"] != 0).any(-1).sum(1) < 7).all()
    # kind 4 does not read the operand
    plain = launch(np.full(B, 4), B, 8, 2, 4, scene_offset=50, merge_pockets=pairs)
    compare(plain, np.full(B, 4), ids, 8, 2, 4, merge_pockets=pairs)


def test_same_cubby_for_kinds_4_and_5():
    ids = np.r_[np.arange(12), np.arange(12)]
    kind = np.r_[np.full(12, 4), np.full(12, 5)]
    got = launch(kind, 24, 16, 16, 8, scene_ids=ids)
    for key in ("cuboid_centers", "cuboid_dims", "cuboid_quats"):
        assert np.array_equal(got[key][:12, :5], got[key][12:, :5]), key  # the five plates no merge removes, bit for bit
    live = (got["cuboid_dims"][12:] != 0).any(-1)
    for b in range(12):  # a kept wall or shelf is the unmerged cubby's, in its moved-up row
        rows = [tuple(np.r_[got["cuboid_centers"][b, r], got["cuboid_dims"][b, r]]) for r in (5, 6)]
        for r in range(5, int(live[b].sum())):
            assert tuple(np.r_[got["cuboid_centers"][12 + b, r], got["cuboid_dims"][12 + b, r]]) in rows


def test_mixed_batch_old_entry_then_new():
    B, m1, m2, s = 18, 16, 16, 8
    ids = 3 + np.arange(B)
    kind = ids % 6
    old_alone = launch_old(kind, B, m1, m2, s, scene_offset=3, seed=SEED)
    out = nan_buffers(B, m1, m2, s)
    from mpinets_amd import _lib

    k = torch.as_tensor(kind, dtype=torch.int32, device=dev())
    _lib.call("mpx_scene_generate", _lib.ptr(k), None, B, m1, m2, s, SEED, 3, *(_lib.ptr(out[key]) for key in fsg.PRIMITIVE_KEYS),
              _lib.ptr(out["support_boxes"]), _lib.ptr(out["support_kind"]))
    both = launch(kind, B, m1, m2, s, scene_offset=3, out=out)
    old = kind < 3
    for key, v in both.items():
        assert np.array_equal(v[old], old_alone[key][old]), key  # every old row bit-identical to the old entry alone
        assert not np.isnan(v.astype(np.float64)).any(), key
    new_alone = launch(kind, B, m1, m2, s, scene_offset=3)
    for key, v in both.items():
        assert np.array_equal(v[~old], new_alone[key][~old]), key
    # the wrapper dispatches the same way
    from mpinets_amd import scenes

    six = ("tabletop", "cubby", "dresser") + KINDS
    w = scenes.make_scenes_device(B, SEED, six, m1, m2, S=s, env_offset=3)
    for key, v in both.items():
        assert np.array_equal(w[key].cpu().numpy(), v), key
    only_old = scenes.make_scenes_device(B, SEED, six[:3], m1, m2, S=s, env_offset=3)
    assert np.array_equal(only_old["cuboid_dims"].cpu().numpy(), launch_old(ids % 3, B, m1, m2, s, scene_offset=3, seed=SEED)["cuboid_dims"])


def test_fragile_scenes_stay_under_the_cap():
    """Runs after the comparisons above (file order): the tabletop scenes they left out, against the cap."""
    if COUNT["compared"] == 0:  # (run alone: make the comparisons of the first test)
        test_kernel_matches_float64_on_every_launch_shape()
    print(f"tabletop scenes compared exactly: {COUNT['compared'] - COUNT['left out']} of {COUNT['compared']}")
    assert COUNT["left out"] <= FRAGILE_CAP * COUNT["compared"]


def test_old_kinds_through_make_problem_batch_equal_the_golden():
    from mpinets_amd import scenes

    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "problem_batch_default.npz"))
    prob = scenes.make_problem_batch(8, seed=0, device=dev())
    for key in golden.files:
        assert np.array_equal(np.asarray(prob[key].cpu() if torch.is_tensor(prob[key]) else prob[key]), golden[key]), key


KW = dict(seed=3, kinds=KINDS, M1=16, M2=16, scene_source="device", device_clouds=True, problems="task", collision_free=True)


@pytest.fixture(scope="module")
def whole():
    from mpinets_amd import scenes

    return scenes.make_problem_batch(16, **KW)


def test_shards(whole):
    """Rows 5 .. 8 of a 16-row task batch over the three kinds, generated alone, are those rows bit for bit."""
    from mpinets_amd import scenes

    part = scenes.make_problem_batch(4, env_offset=5, total_envs=16, **KW)
    for key in fsg.PRIMITIVE_KEYS + ("support_boxes", "support_kind", "target_support", "valid"):
        assert torch.equal(part[key], whole[key][5:9]), key
    lo, hi = scenes.NUM_ROBOT_POINTS, scenes.NUM_ROBOT_POINTS + scenes.NUM_OBSTACLE_POINTS
    assert torch.equal(part["xyz"][:, lo:hi], whole["xyz"][5:9, lo:hi])


def inside(box, point, slack=1e-5):
    yaw = 2 * np.arctan2(box[9], box[6])
    c, s = np.cos(yaw), np.sin(yaw)
    d = point - box[:3]
    local = np.array([c * d[0] + s * d[1], c * d[1] - s * d[0], d[2]])
    return bool((np.abs(local) <= box[3:6] / 2 + slack).all())


def box_local(points, centre, quat):
    yaw = 2 * np.arctan2(quat[3], quat[0])
    c, s = np.cos(yaw), np.sin(yaw)
    d = points - centre
    return np.stack([c * d[:, 0] + s * d[:, 1], c * d[:, 1] - s * d[:, 0], d[:, 2]], -1)


def test_pipeline_end_to_end_on_reference_scenes():
    """48 task problems over the three new kinds, and over the old three on the same call as the reference figure."""
    from mpinets_amd import scenes, solvers

    kw = dict(M1=40, M2=16, collision_free=True, problems="task", device_clouds=True, scene_source="device")
    old = scenes.make_problem_batch(48, kinds=("tabletop", "cubby", "dresser"), **kw)
    new = scenes.make_problem_batch(48, kinds=KINDS, **kw)
    share_old, share_new = float(old["valid"].float().mean()), float(new["valid"].float().mean())
    per_kind = [float(new["valid"][i::3].float().mean()) for i in range(3)]
    print(f"valid share of 48 task problems: old kinds {share_old:.3f}, reference kinds {share_new:.3f} "
          f"(tabletop_reference {per_kind[0]:.3f}, cubby_reference {per_kind[1]:.3f}, merged_cubby {per_kind[2]:.3f})")
    assert set(new) == set(old)
    assert share_new >= 0.5 * share_old
    cub, cyl = prims_of({k: new[k] for k in fsg.PRIMITIVE_KEYS})
    count = solvers.task_candidates(new["support_boxes"], new["support_kind"], cub, cyl)[3].cpu().numpy()
    for i, name in enumerate(KINDS):
        assert (count[i::3] > 0).any(), name
    # the merged rows: one volume holds start and goal, the plates between them are gone from primitives and cloud
    unmerged = scenes.make_scenes_device(48, 0, KINDS, 40, 16, S=8, merge_pockets=torch.full((48, 2), -1, dtype=torch.int32, device=dev()))
    n = {k: v.cpu().numpy() for k, v in new.items() if torch.is_tensor(v)}
    u = {k: v.cpu().numpy() for k, v in unmerged.items()}
    lo, hi = scenes.NUM_ROBOT_POINTS, scenes.NUM_ROBOT_POINTS + scenes.NUM_OBSTACLE_POINTS
    merged_rows = [b for b in range(2, 48, 3) if n["valid"][b]]
    assert merged_rows, "no valid merged-cubby row among 16"
    for b in merged_rows:
        vol = np.r_[n["target_volume"][b], 0, 0]
        assert inside(vol, n["start_pose"][b, :3, 3]) and inside(vol, n["target_pose"][b, :3, 3]), b
        assert np.array_equal(n["target_volume"][b], n["support_boxes"][b, n["target_support"][b], :10])
        live, live_u = (n["cuboid_dims"][b] != 0).any(-1), (u["cuboid_dims"][b] != 0).any(-1)
        assert live_u.sum() == 7 and live.sum() in (5, 6)
        kept = {tuple(np.r_[n["cuboid_centers"][b, r], n["cuboid_dims"][b, r]]) for r in np.flatnonzero(live)}
        gone = [r for r in range(7) if tuple(np.r_[u["cuboid_centers"][b, r], u["cuboid_dims"][b, r]]) not in kept]
        assert len(gone) == 7 - live.sum() and set(gone) <= {5, 6}
        cloud = n["xyz"][b, lo:hi, :3]
        for r in gone:  # no cloud point lies in the removed plate's slab, away from the plates that are still there
            on = np.abs(box_local(cloud, u["cuboid_centers"][b, r], u["cuboid_quats"][b, r])) <= u["cuboid_dims"][b, r] / 2 + [-0.05, -0.05, -0.05] + 0.0501 * (np.arange(3) == (1 if r == 5 else 2))
            near = np.zeros(len(cloud), bool)
            for k in np.flatnonzero(live):
                q = np.abs(box_local(cloud, n["cuboid_centers"][b, k], n["cuboid_quats"][b, k])) - n["cuboid_dims"][b, k] / 2
                near |= (q <= 0.05).all(-1)
            assert not (on.all(-1) & ~near).any(), (b, r)
    for b in range(2, 48, 3):
        if not n["valid"][b]:  # invalid rows stay unmerged
            assert np.array_equal(n["cuboid_dims"][b], u["cuboid_dims"][b])
