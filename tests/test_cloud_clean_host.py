"""CPU: the restatement of the captured-cloud cleaning (tests/float64_cloud_clean.py) on its own -- its Philox, its
undecided share and what every stage removes on the cases the GPU tests use -- and the new entry points in the library /
header / bindings with their argument checks, which need no GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import float64_cloud_clean as f64

NAME = "mpx_cloud_clean"


def test_numpy_philox_equals_the_oracle(oracle):
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((1, 2, 15, 0), (7, 0)), ((76799 >> 2, 3, 15, 0), (0xDEADBEEF, 0x12345678)),
                     ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)),
                     ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))):
        got = np.array([int(w) for w in f64.philox4x32_np(*[np.uint32(c) for c in ctr], *key)], np.uint32)
        np.testing.assert_array_equal(got, oracle.philox4x32(ctr, key))
    # the draw's keys are those words, row i taking word i & 3 of block i >> 2
    keys = f64.draw_keys(11, (5 << 32) | 9, 4)
    for i in (0, 3, 4, 10):
        assert keys[i] == oracle.philox4x32((i >> 2, 4, f64.STREAM_CAPTURE, 0), (9, 5))[i & 3]


def test_draw_restatement_is_a_sorted_subset():
    valid = np.random.default_rng(0).random(1000) < 0.4
    got = f64.draw(valid, 100, 3, 0)
    assert len(set(got.tolist())) == 100 and valid[got].all()
    keys = f64.draw_keys(1000, 3, 0)
    assert (np.diff(keys[got].astype(np.int64)) >= 0).all() and keys[got].max() <= np.sort(keys[valid])[99]
    assert f64.draw(valid, int(valid.sum()) + 1, 3, 0) is None
    assert not np.array_equal(got, f64.draw(valid, 100, 4, 0)) and not np.array_equal(got, f64.draw(valid, 100, 3, 1))


def test_restatement_equals_a_plain_brute_force():
    case = (1, 700, True, True, True, False, 0)
    data, kw = f64.make_case(case), f64.case_arguments(case)
    centres, radii = f64.oracle_centres(data["q"]), f64.sphere_radii()
    res = f64.restate_case(case, centres)[0]
    p = data["cloud"][0].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p).all(axis=1)
        inside = np.zeros(len(p), bool)
        for b in f64.WORKSPACE.astype(np.float64):
            inside |= ((p > b[:3]) & (p < b[3:])).all(axis=1)
        R = radii.astype(np.float64) + kw["robot_margin"]
        dr = np.linalg.norm(p[:, None, :] - centres[0].astype(np.float64)[None], axis=-1) - R[None]
        robot = (dr <= 0).any(axis=1)
        alive1 = ok & inside & ~robot
        d = np.linalg.norm(p[:, None, :] - p[None], axis=-1)
        d[~np.isfinite(d)] = np.inf
        near = (d <= kw["outlier_radius"]) & alive1[None, :]
        np.fill_diagonal(near, False)
        kept = alive1 & (near.sum(axis=1) >= kw["min_neighbors"])
    brute = np.where(~ok, 1, np.where(~inside, 2, np.where(robot, 3, np.where(kept, 0, 4))))
    clear = ~res["undecided"]
    assert clear.mean() > 0.99 and (res["allowed"][clear] == 1 << brute[clear]).mean() > 0.995  # (micrometre ties aside)
    assert set(np.unique(brute).tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_restatement_alone_is_within_the_cap_and_every_stage_bites_and_spares(case):
    """With centres from the oracle's FK: at most 1 % of an environment's rows are undecided (expected 0), the boxes, the
    robot and the outlier stage each remove >= 3 % of the rows reaching them and keep >= 50 % (clouds of <= 5 rows
    exempt), and a case that draws has enough rows left in every environment."""
    B, N, crop, robot, outlier, ragged, n_out = case
    res = f64.restate_case(case)
    reached, removed = {2: 0, 3: 0, 4: 0}, {2: 0, 3: 0, 4: 0}
    for b, r in enumerate(res):
        assert r["undecided"].sum() <= f64.UNDECIDED_CAP * N, (b, int(r["undecided"].sum()))
        assert (r["allowed"] != 0).all()
        for stage, (n_in, n_out_stage) in r["stats"].items():
            reached[stage] += n_in
            removed[stage] += n_out_stage
        if n_out:
            assert (r["allowed"] == 1).sum() >= n_out, (b, int((r["allowed"] == 1).sum()))
    print(f64.case_id(case), {s: (reached[s], removed[s]) for s in reached},
          "undecided", sum(int(r["undecided"].sum()) for r in res))
    assert set(s for s in reached if reached[s]) <= {s for s, on in ((2, crop), (3, robot), (4, outlier)) if on}
    if N > 5:
        for stage, on in ((2, crop), (3, robot), (4, outlier)):
            if on:
                assert 0.03 * reached[stage] <= removed[stage] <= 0.5 * reached[stage], (stage, reached[stage], removed[stage])


def test_symbols_are_exported_bound_and_declared():
    from test_abi_and_host import header_symbols

    from mpinets_amd import _lib, capture

    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ((NAME, 26), (NAME + "_scratch", 2)):
        assert hasattr(lib, name) and name in header_symbols()
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name]) == nargs
    assert _lib.load().mpx_version() == 341
    assert _lib.RESTYPES[NAME + "_scratch"] is ctypes.c_int64
    np.testing.assert_array_equal(capture.REFERENCE_WORKSPACE, f64.WORKSPACE)
    assert capture.REFERENCE_WORKSPACE.dtype == np.float32 and capture.REFERENCE_WORKSPACE.shape == (2, 6)


def test_scratch_size_grows_with_the_batch_and_the_rows():
    from mpinets_amd import _lib

    lib = _lib.load()
    a, b, c = lib.mpx_cloud_clean_scratch(1, 4096), lib.mpx_cloud_clean_scratch(2, 4096), lib.mpx_cloud_clean_scratch(1, 307200)
    assert 0 < a < b and a < c
    assert c >= 307200 * 17  # a packed 16-byte row and a reason per row
    assert lib.mpx_cloud_clean_scratch(16, 307200) < 1 << 28  # the 16 x 640 x 480 batch stays below 256 MB
    assert lib.mpx_cloud_clean_scratch(-1, 4) < 0 and lib.mpx_cloud_clean_scratch(1, -4) < 0


def _call(lib, B=2, N=100, stride=3, n_boxes=2, S=57, margin=0.0, radius=0.01, min_neighbors=4, n_out=16, env_offset=0,
          scratch_bytes=None, one=ctypes.c_void_p(256)):
    # any non-NULL "device pointer": validation fails before it is touched
    if scratch_bytes is None:
        scratch_bytes = lib.mpx_cloud_clean_scratch(max(B, 0), max(N, 0))
    return lib.mpx_cloud_clean(one, N * stride, stride, N, None, B, one, n_boxes, one, one, S, margin, radius, min_neighbors,
                               n_out, 0, env_offset, one, n_out * 3, 3, one, one, one, one, scratch_bytes, None)


def test_argument_errors_are_reported_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert _call(lib, n_out=4097) != 0 and b"n_out" in lib.mpx_last_error() and b"4096" in lib.mpx_last_error()
    assert _call(lib, S=65) != 0 and b"spheres" in lib.mpx_last_error() and b"64" in lib.mpx_last_error()
    assert _call(lib, n_boxes=9) != 0 and b"n_boxes" in lib.mpx_last_error() and b"8" in lib.mpx_last_error()
    assert _call(lib, margin=-1e-3) != 0 and b"robot_margin" in lib.mpx_last_error()
    assert _call(lib, margin=float("nan")) != 0 and b"robot_margin" in lib.mpx_last_error()
    for radius in (0.0, -0.01, float("nan")):
        assert _call(lib, radius=radius) != 0 and b"outlier_radius" in lib.mpx_last_error(), radius
    need = lib.mpx_cloud_clean_scratch(2, 100)
    assert _call(lib, scratch_bytes=need - 1) != 0 and b"scratch" in lib.mpx_last_error()
    for kw in (dict(B=-1), dict(N=-1), dict(S=-1), dict(n_boxes=-1), dict(min_neighbors=-1), dict(n_out=-1)):
        assert _call(lib, **kw) != 0 and b"negative size" in lib.mpx_last_error(), kw
    assert _call(lib, stride=2) != 0 and b"cloud_point_stride" in lib.mpx_last_error()
    assert _call(lib, env_offset=-1) != 0 and b"env_offset" in lib.mpx_last_error()
    assert _call(lib, one=None) != 0 and b"NULL" in lib.mpx_last_error()
    # nothing to do: no launch, no error, nothing touched; a radius is not needed while the outlier stage is off
    assert _call(lib, B=0) == 0 and _call(lib, B=0, radius=0.0, min_neighbors=0) == 0


def test_python_entry_points_refuse_cpu_tensors_and_keep_their_defaults():
    from mpinets_amd import _lib, capture

    sig = inspect.signature(capture.clean_point_clouds).parameters
    assert sig["num_points"].default == 4096 and sig["boxes"].default is capture.REFERENCE_WORKSPACE
    assert [sig[k].default for k in ("counts", "q", "collision_sampler", "robot_margin", "outlier_radius", "min_neighbors",
                                     "seed", "env_offset", "out", "return_index", "return_reason")] == \
        [None, None, None, 0.0, 0.0, 0, 0, 0, None, False, False]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in sig if k not in ("cloud", "num_points"))
    with pytest.raises(_lib.MpxError):
        capture.clean_point_clouds(torch.zeros(2, 50, 3), 8)
    assert list(inspect.signature(capture.clean_point_cloud).parameters)[:2] == ["xyz", "rgba"]
