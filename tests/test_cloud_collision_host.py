"""CPU: the float64 restatement of the point-cloud collision check against a plain brute force, the new entry point in
the library / header / bindings, its argument checks, the kernels' code objects, and the restatement's own undecided
share on the seeds the GPU tests use (tests/test_gpu_cloud_collision.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import float64_cloud_collision as f64
from mpinets_amd import franka_tables as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mpx_franka_cloud_collision"


def test_restatement_equals_a_plain_brute_force():
    case = (3, 4, False, 300, 0.01, 0.005)
    q, cloud = f64.make_case(case, seed=5)
    centres = f64.oracle_centres(q, False)
    radii = ft.collision_sphere_table(False)[1]
    res = f64.restate(centres, cloud, radii, 0.01, 0.005)
    R = radii.astype(np.float64) + 0.01 + 0.005
    for b in range(3):
        d = np.linalg.norm(centres[b].astype(np.float64)[:, :, None, :] - cloud[b].astype(np.float64)[None, None, :, :], axis=-1)
        # (the restatement subtracts in float32 like the kernel: half an ulp of a coordinate <= 2 m per component)
        np.testing.assert_allclose(np.sqrt(res["d2_min"][b]), d.min(axis=2), rtol=0, atol=3e-7)
        assert (res["nearest"][b] == d.argmin(axis=2)).mean() > 0.999  # (a float32-subtraction near-tie may differ)
        clear = np.abs(d - R[None, :, None]).min(axis=2) > 1e-6  # pairs a micrometre from the threshold decide nothing
        brute = (d <= R[None, :, None]).any(axis=2)
        assert (res["hit"][b][clear] == brute[clear]).all()
        assert res["env_hit"][b] == brute.any() or not clear.all()
        assert res["in_band"](b, res["nearest"][b]).all()
    assert 0 < res["hit"].sum() < res["hit"].size  # both outcomes occur among the (waypoint, sphere) pairs


def test_restatement_ignores_non_finite_points_and_respects_counts():
    q, cloud = f64.make_case((2, 2, False, 40, 0.0, 0.0), seed=6)
    centres = f64.oracle_centres(q, False)
    radii = ft.collision_sphere_table(False)[1]
    bad = cloud.copy()
    bad[:, 3, 0], bad[:, 17, 2], bad[:, 30, 1] = np.nan, np.inf, -np.inf
    keep = np.ones(40, bool)
    keep[[3, 17, 30]] = False
    a, b = f64.restate(centres, bad, radii), f64.restate(centres, cloud[:, keep], radii)
    assert (a["d2_min"] == b["d2_min"]).all()
    assert ((np.cumsum(keep) - 1)[a["nearest"]] == b["nearest"]).all()
    c, d = f64.restate(centres, cloud, radii, counts=[0, 7]), f64.restate(centres, cloud[:, :7], radii)
    assert np.isinf(c["d2_min"][0]).all() and (c["nearest"][0] == -1).all() and not c["env_hit"][0]
    assert (c["d2_min"][1] == d["d2_min"][1]).all() and (c["nearest"][1] == d["nearest"][1]).all()
    allnan = f64.restate(centres, np.full_like(cloud, np.nan), radii)
    assert np.isinf(allnan["d2_min"]).all() and (allnan["nearest"] == -1).all() and not allnan["env_hit"].any()


def test_symbol_is_exported_bound_and_declared():
    from test_abi_and_host import header_symbols

    from mpinets_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME)
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME]) == 19
    assert NAME in header_symbols()
    assert _lib.load().mpx_version() == 341
    # the constants the tests restate are the header's
    assert f64.WAYPOINT_CHUNK == f64._header_constant("MPX_CLOUD_TC")
    assert f64.TILE == f64._header_constant("MPX_CLOUD_TILE")
    assert _lib.load().mpx_get_variant(f64._header_constant("MPX_VARIANT_CLOUD_CULL")) == 1


def _call(lib, B=2, T=3, S=56, N=8, stride=3, point_radius=0.0, clearance=0.0, one=ctypes.c_void_p(256)):
    # any non-NULL "device pointer": validation fails before it is touched
    return lib.mpx_franka_cloud_collision(one, B, T, 0.025, one, one, one, S, one, N * stride, stride, N, None, point_radius,
                                          clearance, one, None, None, None)


def test_argument_errors_are_reported_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert _call(lib, S=65) != 0 and b"64" in lib.mpx_last_error()
    for kw in (dict(B=-1), dict(T=-1), dict(S=-1), dict(N=-1)):
        assert _call(lib, **kw) != 0 and b"negative size" in lib.mpx_last_error(), kw
    assert _call(lib, point_radius=-1e-3) != 0 and b"point_radius" in lib.mpx_last_error()
    assert _call(lib, point_radius=float("nan")) != 0 and b"point_radius" in lib.mpx_last_error()
    assert _call(lib, stride=2) != 0 and b"cloud_point_stride" in lib.mpx_last_error()
    assert _call(lib, one=None) != 0 and b"NULL" in lib.mpx_last_error()
    # nothing to do: no launch, no error, nothing touched
    assert _call(lib, B=0) == 0 and _call(lib, T=0) == 0 and _call(lib, S=0) == 0 and _call(lib, N=0) == 0


def test_python_entry_points_refuse_cpu_tensors():
    import inspect

    from mpinets_amd import _lib, metrics, robot, rollout

    sig = inspect.signature(robot.FrankaCollisionSampler.check_cloud).parameters
    assert [sig[k].default for k in ("counts", "point_radius", "clearance", "return_distance", "return_nearest")] == \
        [None, 0.0, 0.0, False, False]
    sig = inspect.signature(metrics.BatchedEvaluator.evaluate_trajectories).parameters
    assert [sig[k].default for k in ("scene_cloud", "scene_cloud_counts", "cloud_point_radius")] == [None, None, 0.0]
    assert inspect.signature(rollout.RolloutEngine.cloud_collision).parameters["point_radius"].default == 0.0
    # (the class needs a GPU device to build; the method itself refuses CPU operands before anything else)
    s = robot.FrankaCollisionSampler.__new__(robot.FrankaCollisionSampler)
    with pytest.raises(_lib.MpxError):
        s.check_cloud(torch.zeros(2, 3, 7), torch.zeros(2, 5, 3))


def test_cloud_kernels_use_no_scratch():
    """Every instantiation (3 forms x 9 pairs-per-thread shapes): private segment 0, no VGPR spills -- the pairs' centres
    and minima are registers, not memory."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "franka_cloud_collision_kernel" in n}
    assert len(hits) == 27, sorted(hits)
    for n, f in sorted(hits.items()):
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, n
    # the benchmark shape (50 x 56 pairs = 12 per thread) keeps 4 waves per SIMD in both forms
    for n, f in hits.items():
        if "ILi256ELi12E" in n:
            print(n[:52], {k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
            assert int(f[".vgpr_count"]) <= 128, (n, f[".vgpr_count"])


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_undecided_cap_holds_for_the_restatement_alone(case):
    """With centres from the oracle's FK on the CPU: the share of undecided environments of every GPU case is within the
    cap (expected 0), so the GPU test's condition is satisfiable before anything runs on a GPU."""
    B, T, base, N, pr, cl = case
    q, cloud = f64.make_case(case)
    res = f64.restate(f64.oracle_centres(q, base), cloud, ft.collision_sphere_table(base)[1], pr, cl)
    share = res["env_undecided"].mean()
    print(f"{f64.case_id(case)}: hit {int(res['env_hit'].sum())}/{B}, undecided {int(res['env_undecided'].sum())}")
    assert share <= f64.UNDECIDED_CAP


def test_cases_reach_both_outcomes():
    hit = total = 0
    for case in f64.CASES:
        B, T, base, N, pr, cl = case
        if B * T * N > 200000:
            continue
        q, cloud = f64.make_case(case)
        res = f64.restate(f64.oracle_centres(q, base), cloud, ft.collision_sphere_table(base)[1], pr, cl)
        hit, total = hit + int(res["env_hit"].sum()), total + B
    assert 0 < hit < total
