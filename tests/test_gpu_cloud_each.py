"""GPU: ``mpx_franka_cloud_collision_each`` (csrc/cloud_collision.hip, ``FrankaCollisionSampler.check_cloud_each``): one
verdict per waypoint, held bit for bit to the entry that predates it -- ``check_cloud`` on every waypoint as an environment
of its own -- and, inside the bands of tests/float64_cloud_collision.py, to the float64 restatement; then the ``active``
mask, the cloud's edges and the output's.

The 18 cases are those of tests/test_gpu_cloud_collision.py: T from 1 to chunk + 1, every pairs-per-thread
instantiation, N from 1 to two tiles + 3."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik_cloud as f64  # noqa: E402

from mpinets_amd import _lib, scenes  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd.robot import FrankaCollisionSampler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
VARIANT_CLOUD_CULL = 3  # MPX_VARIANT_CLOUD_CULL


@functools.lru_cache(maxsize=None)
def sampler(with_base_link=False):
    return FrankaCollisionSampler(DEV, with_base_link=with_base_link)


def both_variants(fn):
    """-> (fn() with the cull, fn() without it); the variant is restored."""
    lib = _lib.load()
    culled = fn()
    assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 0) == 0
    try:
        plain = fn()
    finally:
        assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 1) == 0
    return culled, plain


def one_by_one(s, q, cloud, counts=None, **kw):
    """``check_cloud`` on the B*T configurations as separate environments, each cloud repeated T times -> bool [B,T]."""
    B, T, _ = q.shape
    cn = None if counts is None else counts.repeat_interleave(T, 0)
    return s.check_cloud(q.reshape(B * T, 1, 7), cloud.repeat_interleave(T, 0), cn, **kw).reshape(B, T)


@functools.lru_cache(maxsize=None)
def run_case(case):
    """One device run per case, shared by the tests below (inputs and results are not modified)."""
    B, T, base, N, pr, cl = case
    qn, cn = f64.make_case(case)
    s = sampler(base)
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    kw = dict(point_radius=pr, clearance=cl)
    each = both_variants(lambda: s.check_cloud_each(q, cloud, **kw))
    single = both_variants(lambda: one_by_one(s, q, cloud, **kw))
    env = both_variants(lambda: s.check_cloud(q, cloud, **kw))
    centres = s.sphere_centers(q.reshape(B * T, 7)).reshape(B, T, -1, 3).cpu().numpy()
    ref = f64.verdicts(centres, cn, s.radii.cpu().numpy(), pr, cl)
    torch.cuda.synchronize()
    return q, cloud, each, single, env, ref


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_equals_the_existing_entry_waypoint_by_waypoint(case):
    B, T = case[:2]
    _, _, each, single, env, _ = run_case(case)
    for v in (0, 1):  # with the cull, without it
        assert each[v].dtype == torch.bool and each[v].shape == (B, T)
        assert torch.equal(each[v], single[v]), v
        assert torch.equal(each[v].any(1), env[v]), v
    assert torch.equal(each[0], each[1]) and torch.equal(single[0], single[1])


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_device_against_float64(case):
    B, T = case[:2]
    _, _, each, _, _, (hit, und) = run_case(case)
    got = each[0].cpu().numpy()
    print(f"{f64.case_id(case)}: {int(hit.sum())} of {B * T} waypoints hit, {int(und.sum())} undecided waypoints left out")
    assert und.mean() <= f64.UNDECIDED_CAP
    assert (got[~und] == hit[~und]).all()


MASK_CASES = [f64.CASES[i] for i in (5, 7, 10, 11, 16, 17)]  # T = 50, 2, 65, 65, 40, 64


@pytest.mark.parametrize("case", MASK_CASES, ids=f64.case_id)
def test_active_mask(case):
    B, T, base, N, pr, cl = case
    q, cloud, each, _, _, _ = run_case(case)
    s = sampler(base)
    full = each[0]
    assert bool(full.any())
    g = torch.Generator().manual_seed(100 + B * T)
    active = (torch.rand((B, T), generator=g) < 0.5).to(DEV)
    if T > 64:
        active[:, 64:] = False  # the second chunk's only waypoint
        active[:, 63] = True
    active[B - 1] = False  # an environment with nothing active
    kw = dict(point_radius=pr, clearance=cl)
    for form, a in (("bool", active), ("int32", active.int()), ("int64 -5", active.long() * -5)):
        got = both_variants(lambda: s.check_cloud_each(q, cloud, active=a, **kw))
        for v in (0, 1):
            assert torch.equal(got[v], full & active), (form, v)
    assert not bool(got[0][B - 1].any())
    everything = both_variants(lambda: s.check_cloud_each(q, cloud, active=torch.ones_like(active), **kw))
    assert torch.equal(everything[0], full) and torch.equal(everything[1], full)
    nothing = both_variants(lambda: s.check_cloud_each(q, cloud, active=torch.zeros_like(active), **kw))
    assert not bool(nothing[0].any()) and not bool(nothing[1].any())
    # an inactive waypoint's q is not read: garbage there changes nothing
    junk = torch.where(active[:, :, None], q, torch.full_like(q, float("nan")))
    got = both_variants(lambda: s.check_cloud_each(junk, cloud, active=active, **kw))
    assert torch.equal(got[0], full & active) and torch.equal(got[1], full & active)


def test_a_hit_of_an_inactive_waypoint_does_not_leak():
    """Three far-apart configurations, one point on the last sphere's centre of the second (the restatement on the CPU: the
    other two clear it by 0.59 m and 0.45 m), laid out as trajectories in which only one waypoint is the second
    configuration.  Tested, that waypoint alone hits; switched off, nothing does
    -- although padding and replaced pairs repeat a pair of an active waypoint."""
    s = sampler()
    q = torch.from_numpy(scenes.random_configurations(3, 60)).to(DEV)[None].contiguous()  # [1,3,7]
    cloud = s.sphere_centers(q[0])[1, -1].reshape(1, 1, 3).contiguous()
    for T in (3, 65, 130):  # one chunk; the inactive waypoint in a chunk of one; three chunks
        qq = q[:, [0, 2] * ((T - 1) // 2) + [1] + ([0] if T % 2 == 0 else []), :].contiguous()
        assert qq.shape == (1, T, 7)
        want = torch.zeros((1, T), dtype=torch.bool, device=DEV)
        want[0, 2 * ((T - 1) // 2)] = True
        off = ~want
        for got in both_variants(lambda: s.check_cloud_each(qq, cloud)):
            assert torch.equal(got, want), T
        for got in both_variants(lambda: s.check_cloud_each(qq, cloud, active=off)):
            assert not bool(got.any()), T
        for got in both_variants(lambda: s.check_cloud_each(qq, cloud, active=want)):
            assert torch.equal(got, want), T


def test_counts():
    case = (1, 50, False, 300, 0.01, 0.0)
    qn, cn = f64.make_case(case, seed=31)
    s = sampler()
    N = case[3]
    counts = torch.tensor([-3, 0, 1, N, N + 5], dtype=torch.int32, device=DEV)
    B = counts.numel()
    q = torch.from_numpy(qn).to(DEV).expand(B, -1, -1).contiguous()
    cloud = torch.from_numpy(cn).to(DEV).expand(B, -1, -1).contiguous()
    cloud[:, 0] = s.sphere_centers(q[:, 7].contiguous())[:, -1]  # row 0 certainly hits waypoint 7 (and few others)
    kw = dict(point_radius=0.01)
    for got in both_variants(lambda: s.check_cloud_each(q, cloud, counts, **kw)):
        assert not bool(got[:2].any())
        assert torch.equal(got[2:3], s.check_cloud_each(q[2:3], cloud[2:3, :1].contiguous(), **kw)) and bool(got[2, 7])
        full = s.check_cloud_each(q[3:4], cloud[3:4], **kw)
        assert torch.equal(got[3:4], full) and torch.equal(got[4:5], full) and not torch.equal(full, got[2:3])
        assert torch.equal(got, one_by_one(s, q, cloud, counts, **kw))
    for dtype in (torch.int64, torch.int32):
        assert torch.equal(s.check_cloud_each(q, cloud, counts.to(dtype), **kw), got)


def test_non_finite_rows_never_hit():
    s = sampler()
    q = torch.from_numpy(scenes.linear_trajectories(2, 50, 32)).to(DEV)
    c = s.sphere_centers(q[:, 10].contiguous())[:, 20]  # [2,3]: a sphere centre of waypoint 10
    nan, inf = float("nan"), float("inf")
    rows = []
    for axis in range(3):
        for bad in (nan, inf, -inf):
            r = c.clone()
            r[:, axis] = bad
            rows.append(r)
    rows.append(torch.full_like(c, nan))
    cloud = torch.stack(rows, 1).contiguous()  # [2,10,3]
    for got in both_variants(lambda: s.check_cloud_each(q, cloud, point_radius=0.05)):
        assert not bool(got.any())
    control = torch.cat([cloud, c[:, None]], 1).contiguous()
    for got in both_variants(lambda: s.check_cloud_each(q, control, point_radius=0.05)):
        assert bool(got[:, 10].all()) and torch.equal(got, s.check_cloud_each(q, c[:, None].contiguous(), point_radius=0.05))


def test_slab_view_equals_a_contiguous_copy():
    B, T, N = 3, 50, 100
    qn, cn = f64.make_case((B, T, False, N, 0.0, 0.0), seed=33)
    s = sampler()
    q = torch.from_numpy(qn).to(DEV)
    xyz = torch.empty((B, 6272, 4), device=DEV)
    xyz[..., 3] = torch.rand((B, 6272), device=DEV) * 3 - 1  # other data in the label column
    # every row outside the view WOULD hit every waypoint's first sphere... of waypoint t = row % T
    hit_rows = s.sphere_centers(q.reshape(B * T, 7)).reshape(B, T, -1, 3)[:, :, 0]
    xyz[:, :, :3] = hit_rows[:, torch.arange(6272, device=DEV) % T]
    xyz[:, 2048:2048 + N, :3] = torch.from_numpy(cn).to(DEV)
    view = xyz[:, 2048:2048 + N, :3]
    assert not view.is_contiguous() and view.stride() == (6272 * 4, 4, 1)
    a = both_variants(lambda: s.check_cloud_each(q, view))
    b = both_variants(lambda: s.check_cloud_each(q, view.contiguous()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], a[1])
    assert not bool(a[0].all()) and bool(a[0].any())  # (a kernel that strays outside the view finds every waypoint hit)


def test_output_is_written_not_ored_and_guard_rows_stay():
    case = f64.CASES[10]  # B 3, T 65
    B, T, base, N, pr, cl = case
    q, cloud, each, _, _, _ = run_case(case)
    s = sampler(base)
    G = 2
    for variant in (1, 0):
        buf = torch.full((B + 2 * G, T), -77, dtype=torch.int32, device=DEV)
        lib = _lib.load()
        assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, variant) == 0
        try:
            _lib.call("mpx_franka_cloud_collision_each", _lib.ptr(q), B, T, s.finger, _lib.ptr(s.centers), _lib.ptr(s.radii),
                      _lib.ptr(s.links), s.num_spheres, _lib.ptr(cloud), cloud.stride(0), cloud.stride(1), N, None, pr, cl,
                      None, _lib.ptr(buf[G:]))
        finally:
            assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 1) == 0
        torch.cuda.synchronize()
        inner = buf[G:G + B]
        assert bool(((inner == 0) | (inner == 1)).all()) and torch.equal(inner != 0, each[0])
        assert bool((buf[:G] == -77).all()) and bool((buf[G + B:] == -77).all()), "a guard row was written"
    # the zero paths write too: no point, no sphere count to speak of
    buf = torch.full((B + 2 * G, T), -77, dtype=torch.int32, device=DEV)
    _lib.call("mpx_franka_cloud_collision_each", _lib.ptr(q), B, T, s.finger, _lib.ptr(s.centers), _lib.ptr(s.radii),
              _lib.ptr(s.links), s.num_spheres, None, 0, 3, 0, None, pr, cl, None, _lib.ptr(buf[G:]))
    assert bool((buf[G:G + B] == 0).all()) and bool((buf[:G] == -77).all()) and bool((buf[G + B:] == -77).all())
    zeros = torch.zeros(B, dtype=torch.int32, device=DEV)
    buf.fill_(-77)
    _lib.call("mpx_franka_cloud_collision_each", _lib.ptr(q), B, T, s.finger, _lib.ptr(s.centers), _lib.ptr(s.radii),
              _lib.ptr(s.links), s.num_spheres, _lib.ptr(cloud), cloud.stride(0), cloud.stride(1), N, _lib.ptr(zeros), pr, cl,
              None, _lib.ptr(buf[G:]))
    assert bool((buf[G:G + B] == 0).all()) and bool((buf[:G] == -77).all()) and bool((buf[G + B:] == -77).all())


def test_empty_shapes_and_repeatability():
    case = f64.CASES[8]  # B 70, T 50
    B, T, base, N, pr, cl = case
    q, cloud, each, _, _, _ = run_case(case)
    s = sampler(base)
    kw = dict(point_radius=pr, clearance=cl)
    assert s.check_cloud_each(q[:0], cloud[:0], **kw).shape == (0, T)
    assert s.check_cloud_each(q[:, :0], cloud, **kw).shape == (B, 0)
    none = s.check_cloud_each(q, cloud[:, :0], **kw)
    assert none.shape == (B, T) and not bool(none.any())
    single = s.check_cloud_each(q[:, 0].contiguous(), cloud, **kw)  # [B,7] -> [B,1]
    assert single.shape == (B, 1) and torch.equal(single[:, 0], each[0][:, 0])
    again = s.check_cloud_each(q, cloud, **kw)
    assert torch.equal(again, each[0]) and torch.equal(s.check_cloud_each(q, cloud, **kw), again)
    with pytest.raises(_lib.MpxError):
        s.check_cloud_each(q, cloud[:1], **kw)
