"""Every instantiation ``mpx_fps`` can launch (csrc/pointnet.hip), at the lowest and the highest N of its range, on a
uniform cloud and on a cloud of exact ties, bit for bit against the scalar oracle -- and the row strides no other test
uses, for each kernel family of ``mpx_fps`` and of ``mpx_ball_query``.

``launch_routes.fps_route`` asks the library which instantiation a shape takes (the launcher obeys the same function);
``test_fps_cases_reach_every_instantiation`` (CPU) walks it over every N the entry point accepts and shows that the cases
reach each instantiation at both ends of its range.  The highest N of a range fills the last per-lane slot on every lane,
the lowest leaves it empty on most; the tie order (k mod bs, k) meets a different layout of points over lanes in every
instantiation, so each one gets a tied cloud of its own."""
import numpy as np
import pytest
import torch

from launch_routes import FPS_MAX_N, MPX_VARIANT_BALL_QUERY, MPX_VARIANT_FPS, fps_route

MPX_FPS4_MIN_B = 768   # the smallest batch at which the 4-wave form exists (asserted of the library below)
NPOINT, NPOINT_4WAVE = 48, 16

INSTANTIATIONS = ([("wave", p) for p in (1, 2, 4, 8)] + [("cull8", p) for p in (2, 4, 6, 8, 10, 13, 16)]
                  + [("cull4", p) for p in (20, 25, 32)] + [("plain", p) for p in (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16)])

# (family, B, variant, npoint, {P: (the lowest, the highest N of the instantiation's range)}): the cases, written out --
# test_fps_cases_reach_every_instantiation holds every tag and every range end against the library
TAGGED = [
    ("wave", 2, 1, NPOINT, {1: (1, 64), 2: (65, 128), 4: (129, 256), 8: (257, 512)}),
    ("cull8", 2, 1, NPOINT, {2: (513, 1024), 4: (1025, 2048), 6: (2049, 3072), 8: (3073, 4096), 10: (4097, 5120),
                             13: (5121, 6656), 16: (6657, 8192)}),
    ("plain", 2, 0, NPOINT, {1: (1, 512), 2: (513, 1024), 3: (1025, 1536), 4: (1537, 2048), 5: (2049, 2560), 6: (2561, 3072),
                             7: (3073, 3584), 8: (3585, 4096), 10: (4097, 5120), 13: (5121, 6656), 16: (6657, 8192)}),
    # 768 is the smallest batch at which the 4-wave form exists
    ("cull4", MPX_FPS4_MIN_B, 1, NPOINT_4WAVE, {20: (4097, 5120), 25: (5121, 6400), 32: (6401, 8192)}),
]
CASES = [(B, N, variant, npoint) for _, B, variant, npoint, ends in TAGGED for lo_hi in ends.values() for N in lo_hi]
TAGS = {(B, N, variant): (fam, P) for fam, B, variant, _, ends in TAGGED for P, lo_hi in ends.items() for N in lo_hi}


def case_id(case):
    B, N, variant, npoint = case
    fam, P = TAGS[B, N, variant]
    return f"{fam}{P}-B{B}-N{N}"


def _ranges(B, variant):
    spans = {}
    for N in range(1, FPS_MAX_N + 1):
        spans.setdefault(fps_route(B, N, variant), []).append(N)
    return {k: (v[0], v[-1]) for k, v in spans.items()}


def test_fps_cases_reach_every_instantiation():
    """CPU: the launcher takes exactly the instantiations listed, every case's tag is the library's route for it, and CASES
    holds both ends of each instantiation's range."""
    reach = {}
    for B, variant in ((2, 1), (2, 0), (MPX_FPS4_MIN_B, 1), (MPX_FPS4_MIN_B - 1, 1)):
        for key, span in _ranges(B, variant).items():
            reach.setdefault(key, set()).add(span)
    assert set(reach) == set(INSTANTIATIONS)
    assert len(CASES) == 50 and len(TAGS) == len(CASES)
    for B, N, v, _ in CASES:
        assert fps_route(B, N, v) == TAGS[B, N, v], (B, N, v)
    have = {(fps_route(B, N, v), N) for B, N, v, _ in CASES}
    for key, spans in sorted(reach.items()):
        print(key, sorted(spans))
        for lo, hi in spans:
            assert (key, lo) in have and (key, hi) in have, (key, lo, hi)
    # one below the threshold batch keeps the 8-wave form; N <= 4096 keeps it at any batch
    assert fps_route(MPX_FPS4_MIN_B - 1, 8192)[0] == "cull8" and fps_route(MPX_FPS4_MIN_B, 4096) == ("cull8", 8)
    assert fps_route(MPX_FPS4_MIN_B, 4097) == ("cull4", 20) and fps_route(2, 512) == ("wave", 8) and fps_route(2, 513) == ("cull8", 2)
    assert fps_route(2, 512, 0) == ("plain", 1) and fps_route(2, 513, 0) == ("plain", 2) and fps_route(2, 8192, 0) == ("plain", 16)
    # the selectors this file passes to mpx_set_variant are the header's
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mpinets_hip.h")).read()
    assert "#define MPX_VARIANT_FPS %d\n" % MPX_VARIANT_FPS in hdr and "#define MPX_VARIANT_BALL_QUERY %d\n" % MPX_VARIANT_BALL_QUERY in hdr


def uniform_cloud(B, N, seed, stride=3):
    return np.random.default_rng(seed).uniform(-1, 1, (B, N, stride)).astype(np.float32)


def tied_cloud(B, N, seed):
    """A shuffled lattice with spacing 0.125 cut to N, every point there twice where N allows, a sixth of the points
    scaled into the skipped ball |p|^2 <= 1e-3; each environment in an order of its own."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(-8, 9)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.125)
    g = g[rng.permutation(len(g))]
    half = N - N // 2
    assert half <= len(g)
    base = np.concatenate([g[:half], g[:N // 2]], 0)  # (N // 2 of them twice)
    base[::6] *= np.float32(0.01)                      # |p| <= 0.01 * sqrt(3): skipped
    order = rng.permuted(np.tile(np.arange(N), (B, 1)), axis=1)
    return np.ascontiguousarray(base[order])


def _set_variant(what, value):
    from mpinets_amd import _lib

    assert _lib.load().mpx_set_variant(what, value) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fps_instantiation_bit_exact(oracle, case):
    """Indices and new_xyz equal the oracle's on EVERY environment, on the uniform and on the tied cloud."""
    from mpinets_amd.pointnet2 import furthest_point_sample

    B, N, variant, npoint = case
    seed = 31 * N + B + variant
    print(f"FPSFORMS {case_id(case)} route {fps_route(B, N, variant)}")
    try:
        if variant == 0:
            _set_variant(MPX_VARIANT_FPS, 0)
        for name, x in (("uniform", uniform_cloud(B, N, seed)), ("tied", tied_cloud(B, N, seed + 1))):
            idx, nx = furthest_point_sample(torch.from_numpy(x).to("cuda:0"), npoint, return_xyz=True)
            ref = oracle.fps(x, npoint)
            np.testing.assert_array_equal(idx.cpu().numpy(), ref, err_msg=name)
            np.testing.assert_array_equal(nx.cpu().numpy(), oracle.gather_points(x, ref), err_msg=name)
            if name == "tied" and N >= 64:
                assert len(np.unique(x[0], axis=0)) < N  # (the cloud does hold duplicates)
    finally:
        if variant == 0:
            _set_variant(MPX_VARIANT_FPS, 1)


def _poisoned(x3, stride):
    """[B,N,3] -> [B,N,stride] with NaN in the columns no kernel may read."""
    out = np.full(x3.shape[:2] + (stride,), np.nan, np.float32)
    out[..., :3] = x3
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("family,B,N,variant,npoint", [("wave", 3, 300, 1, 48), ("cull8", 3, 3000, 1, 48), ("plain", 3, 3000, 0, 48),
                                                       ("cull4", MPX_FPS4_MIN_B, 4097, 1, NPOINT_4WAVE)])
def test_fps_row_stride_7_and_new_xyz_stride_5(oracle, family, B, N, variant, npoint):
    """Rows of 7 floats (columns 3..6 NaN) in, rows of 5 floats out (columns 3, 4 keep their sentinel)."""
    from mpinets_amd import _lib

    assert fps_route(B, N, variant)[0] == family
    x3 = tied_cloud(B, N, 5 * N) if family != "cull4" else uniform_cloud(B, N, 5 * N)
    x = _poisoned(x3, 7)
    xd = torch.from_numpy(x).to("cuda:0")
    idx = torch.full((B, npoint), -1, dtype=torch.int32, device="cuda:0")
    nx = torch.full((B, npoint, 5), -7.0, dtype=torch.float32, device="cuda:0")
    try:
        if variant == 0:
            _set_variant(MPX_VARIANT_FPS, 0)
        _lib.call("mpx_fps", _lib.ptr(xd), B, N, 7, npoint, _lib.ptr(idx), _lib.ptr(nx), 5)
    finally:
        if variant == 0:
            _set_variant(MPX_VARIANT_FPS, 1)
    ref = oracle.fps(x3, npoint)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref)
    got = nx.cpu().numpy()
    np.testing.assert_array_equal(got[..., :3], oracle.gather_points(x3, ref))
    assert (got[..., 3:] == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("family,N,npoint,radius,nsample,variant,stride,new_stride,offset",
                         [("wave", 300, 70, 0.3, 32, 1, 7, 5, 0),
                          ("bucketed", 3000, 200, 0.08, 64, 1, 7, 5, 0),
                          ("plain <0, false>", 3000, 200, 0.08, 64, 0, 7, 5, 0),
                          ("plain <0, false>", 700, 50, 0.2, 32, 1, 7, 5, 0),       # (512 < N < 2048: the plain kernel by size)
                          ("plain <4, false>", 701, 50, 0.2, 32, 1, 4, 3, 0),       # stride 4, N % 4 != 0
                          ("plain <4, false>", 700, 50, 0.2, 32, 1, 4, 3, 1)])      # stride 4, base one float off 64 bytes
def test_ball_query_row_strides(oracle, family, N, npoint, radius, nsample, variant, stride, new_stride, offset):
    """Strides above 4 (and stride 4 off the aligned path) through each kernel family of ``mpx_ball_query``: indices and
    counts equal the oracle's on the first three columns; every other column is NaN, so a read of the wrong column shows."""
    from mpinets_amd import _lib

    B = 3
    rng = np.random.default_rng(N + stride)
    x3 = rng.uniform(-0.5, 0.5, (B, N, 3)).astype(np.float32)
    x3[:, 20:20 + 2 * nsample] = np.float32([0.1, 0.2, -0.1]) + rng.normal(scale=radius * 0.2, size=(B, 2 * nsample, 3)).astype(np.float32)
    c3 = np.ascontiguousarray(x3[:, rng.permutation(N)[:npoint]]).copy()
    c3[:, 0] = [0.1, 0.2, -0.1]   # more than nsample hits
    c3[:, 1] = 50.0               # none
    x, c = _poisoned(x3, stride), _poisoned(c3, new_stride)
    buf = torch.full((x.size + offset,), float("nan"), dtype=torch.float32, device="cuda:0")
    xd = buf[offset:].view(B, N, stride)
    xd.copy_(torch.from_numpy(x))
    if offset:
        assert xd.data_ptr() % 64 != 0
    cd = torch.from_numpy(c).to("cuda:0")
    idx = torch.full((B, npoint, nsample), -7, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((B, npoint), -7, dtype=torch.int32, device="cuda:0")
    try:
        if variant == 0:
            _set_variant(MPX_VARIANT_BALL_QUERY, 0)
        _lib.call("mpx_ball_query", _lib.ptr(cd), new_stride, _lib.ptr(xd), stride, B, N, npoint, float(radius), nsample,
                  _lib.ptr(idx), _lib.ptr(cnt))
    finally:
        if variant == 0:
            _set_variant(MPX_VARIANT_BALL_QUERY, 1)
    ref, rcnt = oracle.ball_query(c3, x3, radius, nsample, return_counts=True)
    assert rcnt[:, 0].min() == nsample and rcnt[:, 1].max() == 0
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref)
