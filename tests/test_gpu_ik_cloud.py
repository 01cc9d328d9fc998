"""GPU: collision-free inverse kinematics against a point cloud (``mpx_franka_ik_cloud``, ``robot.franka_ik_cloud``) held to
the entries it is made of -- ``franka_ik`` for every start's q and bits 0 and 2, ``check_cloud`` for bit 1, bit for bit
-- to the float64 restatement of the cloud test inside its bands, and to the first-free-start rule; then the Python layer
on top (``collision_free_ik(cloud=...)``, ``capture.plan_to_poses``).

Inputs (tests/float64_ik_cloud.py; tests/test_ik_cloud_host.py shows on the CPU that they can tell right from wrong): 24
targets, the right_gripper poses of ``scenes.random_configurations(24, 41)``, seed 3, clouds of 65 points at radius 0.02
and of 255 bare points uniform in the reach box."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik_cloud as f64  # noqa: E402
from test_gpu_ik import LIMITS, assert_reaches, target_poses  # noqa: E402

from mpinets_amd import _lib, capture, robot, scenes  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd.robot import FrankaCollisionSampler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
fik = f64.fik


def same(a, b):
    """bit-equal, NaN rows included"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.float(), nan=-9.0),
                                                                     torch.nan_to_num(b.float(), nan=-9.0))


@functools.lru_cache(maxsize=None)
def coll():
    return FrankaCollisionSampler(DEV)


@functools.lru_cache(maxsize=None)
def problem(N, B=f64.IK_B):
    poses, q_gen = target_poses(B, seed=f64.IK_TARGET_SEED)
    return poses, q_gen, torch.from_numpy(f64.ik_cloud(N, B)).to(DEV)


@functools.lru_cache(maxsize=None)
def run_case(N, point_radius):
    """One device run per input case, shared by the tests below (results are not modified)."""
    poses, _, cloud = problem(N)
    out = robot.franka_ik_cloud(poses, cloud, point_radius=point_radius, seed=f64.IK_SEED, return_all=True)
    torch.cuda.synchronize()
    return out


def one_by_one(all_q, cloud, **kw):
    """``check_cloud`` on every start's configuration as an environment of its own -> bool [B,64]."""
    B = all_q.size(0)
    return coll().check_cloud(all_q.reshape(B * 64, 1, 7), cloud.repeat_interleave(64, 0), **kw).reshape(B, 64)


@pytest.mark.parametrize("N,point_radius", f64.IK_CASES)
def test_solver_is_franka_ik(N, point_radius):
    poses, _, _ = problem(N)
    _, _, aq, ast = run_case(N, point_radius)
    _, _, fq, fst = robot.franka_ik(poses, seed=f64.IK_SEED, return_all=True, check_self=True)
    assert torch.equal(aq, fq) and torch.equal(ast & 5, fst) and aq.dtype == torch.float32 and ast.dtype == torch.int32


@pytest.mark.parametrize("B", [0, 1, 65])
def test_solver_is_franka_ik_at_batch_edges(B):
    poses, q_gen, cloud = problem(65, B)
    kw = dict(seed=8, env_offset=1000, q_init=q_gen, return_all=True)
    q, st, aq, ast = robot.franka_ik_cloud(poses, cloud, point_radius=0.02, **kw)
    _, _, fq, fst = robot.franka_ik(poses, check_self=True, **kw)
    assert q.shape == (B, 7) and st.shape == (B,) and aq.shape == (B, 64, 7) and ast.shape == (B, 64)
    assert torch.equal(aq, fq) and torch.equal(ast & 5, fst)
    conv = (ast & 1) != 0
    assert torch.equal((ast & 2) != 0, one_by_one(aq, cloud, point_radius=0.02) & conv)
    want_q, want_st = fik.pick(aq.cpu().numpy(), ast.cpu().numpy())
    assert np.array_equal(st.cpu().numpy(), want_st) and same(q, torch.from_numpy(want_q).to(DEV))


@pytest.mark.parametrize("N,point_radius", f64.IK_CASES)
def test_bit_1_is_check_cloud_on_the_single_configuration(N, point_radius):
    _, _, cloud = problem(N)
    _, _, aq, ast = run_case(N, point_radius)
    conv = (ast & 1) != 0
    bit1 = (ast & 2) != 0
    single = one_by_one(aq, cloud, point_radius=point_radius)
    assert torch.equal(bit1[conv], single[conv])
    assert not bool(bit1[~conv].any())
    assert bool(bit1.any()) and bool((conv & ~bit1).any())
    # and the float64 restatement on the device's own sphere centres
    B = aq.size(0)
    centres = coll().sphere_centers(aq.reshape(B * 64, 7)).reshape(B, 64, -1, 3).cpu().numpy()
    hit, und = f64.verdicts(centres, cloud.cpu().numpy(), coll().radii.cpu().numpy(), point_radius, 0.0)
    c, got = conv.cpu().numpy(), bit1.cpu().numpy()
    print(f"N = {N}: {int(c.sum())} converged starts, {int((hit & c).sum())} hit, {int((und & c).sum())} undecided left out")
    assert (und & c).sum() <= f64.UNDECIDED_CAP * c.sum()
    keep = c & ~und
    assert (got[keep] == hit[keep]).all()


@pytest.mark.parametrize("N,point_radius", f64.IK_CASES)
def test_result_is_the_lowest_free_start(N, point_radius):
    from mpinets_amd.metrics import BatchedEvaluator

    poses, _, cloud = problem(N)
    q, st, aq, ast = run_case(N, point_radius)
    bits, stn = ast.cpu().numpy(), st.cpu().numpy()
    want_q, want_st = fik.pick(aq.cpu().numpy(), bits)
    assert np.array_equal(stn, want_st) and same(q, torch.from_numpy(want_q).to(DEV))
    assert bool(torch.isnan(q[st != 0]).all()) and bool(torch.isfinite(q[st == 0]).all())
    counts, moved = np.bincount(stn, minlength=3).tolist(), f64.moved_winners(bits, stn)
    print(f"N = {N}, point_radius {point_radius}: status 0/1/2 = {counts}, moved winners {moved}, converged "
          f"{float(((bits & 1) != 0).mean()):.3f}, self hits {int(((bits & 4) != 0).sum())}")
    assert counts[0] >= 1 and counts[1] >= 1 and moved >= 1
    ok = st == 0
    assert_reaches(q[ok], poses[ok], f"franka_ik_cloud N = {N}")
    assert not bool(coll().check_cloud(q[ok].contiguous(), cloud[ok].contiguous(), point_radius=point_radius).any())
    res = BatchedEvaluator(DEV).evaluate_trajectories(q[ok][:, None].contiguous(), poses[ok])
    assert not bool(res["self_collision"].any())


@pytest.mark.parametrize("N,point_radius", f64.IK_CASES)
def test_result_does_not_depend_on_return_all(N, point_radius):
    poses, _, cloud = problem(N)
    q, st, _, _ = run_case(N, point_radius)
    q2, st2 = robot.franka_ik_cloud(poses, cloud, point_radius=point_radius, seed=f64.IK_SEED)
    assert same(q, q2) and torch.equal(st, st2)


def test_an_empty_cloud_is_free_space():
    poses, q_gen, cloud = problem(65)
    kw = dict(seed=f64.IK_SEED, return_all=True)
    free = robot.franka_ik(poses, check_self=True, **kw)
    none = robot.franka_ik_cloud(poses, cloud[:, :0], point_radius=0.02, **kw)
    zero = robot.franka_ik_cloud(poses, cloud, torch.zeros(poses.size(0), dtype=torch.int32, device=DEV), point_radius=0.02, **kw)
    for got in (none, zero):
        for a, b in zip(got, free):
            assert same(a, b)
    # clearance and check_self are options, as for franka_ik
    off = robot.franka_ik_cloud(poses, cloud[:, :0], check_self=False, **kw)
    for a, b in zip(off, robot.franka_ik(poses, **kw)):
        assert same(a, b)
    wide = robot.franka_ik_cloud(poses, cloud, point_radius=0.0, clearance=0.02, **kw)
    ball = robot.franka_ik_cloud(poses, cloud, point_radius=0.02, **kw)
    assert torch.equal(wide[2], ball[2])
    assert torch.equal((wide[3] & 2) != 0, one_by_one(wide[2], cloud, clearance=0.02) & ((wide[3] & 1) != 0))


def test_first_start_right_but_blocked():
    """q_init = the configuration that generated the target, a one-point cloud on that configuration's link-4 sphere
    centre: start 0 converges at once and hits.  The row returned differs from q_init -- or the status is 1."""
    B = 64
    poses, q_gen = target_poses(B, seed=5)
    s4 = int(np.nonzero(coll().links.cpu().numpy() == ft.LINK_ID["panda_link4"])[0][0])
    cloud = coll().sphere_centers(q_gen)[:, s4][:, None, :].contiguous()  # [B,1,3]
    q, st, aq, ast = robot.franka_ik_cloud(poses, cloud, q_init=q_gen, return_all=True, check_self=False)
    assert bool(((ast[:, 0] & 3) == 3).all()), "start 0 (the generating configuration) must converge and hit its point"
    assert int((st == 2).sum()) == 0
    ok = st == 0
    print(f"start 0 blocked: status 0 in {int(ok.sum())} of {B}")
    assert bool(ok.any())
    assert bool(((q[ok] - q_gen[ok]).abs().amax(1) > 0).all())
    assert_reaches(q[ok], poses[ok], "blocked start 0")
    assert not bool(coll().check_cloud(q[ok].contiguous(), cloud[ok].contiguous()).any())


def test_determinism_sharding_and_seeds():
    B, cut = 65, 30
    poses, _, cloud = problem(255, B)
    kw = dict(point_radius=0.0, return_all=True)
    a = robot.franka_ik_cloud(poses, cloud, seed=21, **kw)
    b = robot.franka_ik_cloud(poses, cloud, seed=21, **kw)
    for x, y in zip(a, b):
        assert same(x, y)
    for lo, hi in ((0, cut), (cut, B)):
        part = robot.franka_ik_cloud(poses[lo:hi].contiguous(), cloud[lo:hi], seed=21, env_offset=lo, **kw)
        for x, y in zip(a, part):
            assert same(x[lo:hi], y), (lo, hi)
    other = robot.franka_ik_cloud(poses, cloud, seed=22, **kw)
    assert not torch.equal(a[2][:, 1:], other[2][:, 1:])  # another seed: other starts
    assert int((a[1] == 0).sum()) >= 1 and int((a[1] == 1).sum()) >= 1


def _raw(poses, cloud, qbuf, sbuf, abuf, bbuf, scratch, scratch_bytes, point_radius=0.02):
    B, N = poses.size(0), cloud.size(1)
    lim = torch.from_numpy(ft.limits_float32_inward(LIMITS)).to(DEV)
    s = coll()
    opt = _lib.IkOptions(64, 0.05, 0.5, 1e-3, float(np.radians(0.5)), 0.0, 1)
    import ctypes

    _lib.call("mpx_franka_ik_cloud", _lib.ptr(poses), B, ft.FINGER_OPENING, _lib.ptr(lim), None, _lib.ptr(s.centers),
              _lib.ptr(s.radii), _lib.ptr(s.links), s.num_spheres, _lib.ptr(cloud), cloud.stride(0), cloud.stride(1), N, None,
              point_radius, ctypes.byref(opt), 0, 0, _lib.ptr(qbuf), _lib.ptr(sbuf), _lib.ptr(abuf), _lib.ptr(bbuf),
              _lib.ptr(scratch), scratch_bytes)


def test_guard_rows_unreachable_targets_and_scratch():
    B, G = 24, 4
    poses, _, cloud = problem(65)
    nbytes = int(_lib.load().mpx_franka_ik_cloud_scratch(B))
    assert nbytes == B * 2560
    scratch = torch.empty(nbytes + 64, dtype=torch.uint8, device=DEV)
    scratch[nbytes:] = 0x5A
    qbuf = torch.full((B + 2 * G, 7), 7.25, device=DEV)
    sbuf = torch.full((B + 2 * G,), -77, dtype=torch.int32, device=DEV)
    abuf = torch.full((B + 2 * G, 64, 7), 7.25, device=DEV)
    bbuf = torch.full((B + 2 * G, 64), -77, dtype=torch.int32, device=DEV)
    _raw(poses, cloud, qbuf[G:], sbuf[G:], abuf[G:], bbuf[G:], scratch, nbytes)
    torch.cuda.synchronize()
    want = robot.franka_ik_cloud(poses, cloud, point_radius=0.02, return_all=True)
    for got, w in zip((qbuf, sbuf, abuf, bbuf), want):
        assert same(got[G:G + B], w)
    for buf, fill in ((qbuf, 7.25), (sbuf, -77), (abuf, 7.25), (bbuf, -77)):
        assert bool((buf[:G] == fill).all()) and bool((buf[G + B:] == fill).all()), "a guard row was written"
    assert bool((scratch[nbytes:] == 0x5A).all()), "the scratch was overrun"
    # without all_q / all_status the same q and status
    q2 = torch.full((B, 7), 7.25, device=DEV)
    s2 = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    _raw(poses, cloud, q2, s2, None, None, scratch, nbytes)
    assert same(q2, want[0]) and torch.equal(s2, want[1]) and bool((scratch[nbytes:] == 0x5A).all())
    # a scratch one byte short is refused, and nothing is written
    q2.fill_(7.25)
    with pytest.raises(_lib.MpxError, match="scratch"):
        _raw(poses, cloud, q2, s2, None, None, scratch, nbytes - 1)
    torch.cuda.synchronize()
    assert bool((q2 == 7.25).all())
    # unreachable targets: status 2, NaN rows, no bit set
    far = poses.clone()
    far[:, :3, 3] = torch.nn.functional.normalize(far[:, :3, 3], dim=1) * 2.0  # 2 m from the base
    q, st, aq, ast = robot.franka_ik_cloud(far, cloud, point_radius=0.02, return_all=True)
    assert bool((st == 2).all()) and bool(torch.isnan(q).all()) and bool((ast == 0).all()) and bool(torch.isfinite(aq).all())


def test_collision_free_ik_against_a_cloud():
    from mpinets_amd.robot import FrankaRealRobot

    n, N, pr = 16, 255, 0.01
    poses, _, cloud = problem(N)
    solved = 0
    for i in range(n):
        pc = cloud[i].cpu().numpy()
        q = FrankaRealRobot.collision_free_ik(poses[i].cpu().numpy(), cloud=pc, point_radius=pr, seed=f64.IK_SEED, device=DEV)
        forms = [FrankaRealRobot.collision_free_ik(poses[i].cpu().numpy(), cloud=c, point_radius=pr, seed=f64.IK_SEED, device=DEV)
                 for c in (cloud[i], cloud[i:i + 1], torch.nn.functional.pad(cloud[i], (0, 1)).cpu().numpy())]
        for other in forms:  # tensor [N,3], tensor [1,N,3], numpy [N,4]
            assert (other is None) == (q is None) and (q is None or np.array_equal(other, q))
        if q is None:
            continue
        solved += 1
        assert q.shape == (7,) and q.dtype == np.float64 and FrankaRealRobot.within_limits(q)
        qt = torch.from_numpy(q).float().to(DEV)[None]
        assert not bool(coll().check_cloud(qt, cloud[i:i + 1], point_radius=pr)[0])
        assert_reaches(qt, poses[i:i + 1], f"collision_free_ik(cloud) {i}")
    batch_q, batch_st = robot.franka_ik_cloud(poses[:n].contiguous(), cloud[:n], point_radius=pr, seed=f64.IK_SEED)
    print(f"collision_free_ik against a cloud: {solved} of {n} solved")
    assert 1 <= solved == int((batch_st == 0).sum())
    with pytest.raises(ValueError):
        FrankaRealRobot.collision_free_ik(poses[0].cpu().numpy(), cloud=cloud[:2], device=DEV)


def test_plan_to_poses():
    B, pr, T = 8, scenes.EXPERT_CLOUD_POINT_RADIUS, 50
    prob = scenes.make_problem_batch(B, seed=4, device=DEV, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16,
                                     collision_free=True, device_clouds=True)
    cloud = prob["xyz"][:, 2048:6144, :3]  # the slab's scene rows, read in place
    assert not cloud.is_contiguous()
    out = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, T=T, seed=4)
    assert sorted(out) == ["ik_status", "plan_status", "q_goal", "trajectory", "valid"]
    q_goal, ik_st, traj, plan_st, valid = (out[k] for k in ("q_goal", "ik_status", "trajectory", "plan_status", "valid"))
    assert q_goal.shape == (B, 7) and traj.shape == (B, T, 7) and valid.dtype == torch.bool
    print(f"plan_to_poses: ik status {ik_st.tolist()}, plan status {plan_st.tolist()}")
    assert torch.equal(valid, (ik_st == 0) & (plan_st == 0))
    assert bool((plan_st[ik_st != 0] == 2).all()) and bool(torch.isnan(q_goal[ik_st != 0]).all())
    want_q, want_st = robot.franka_ik_cloud(prob["target_pose"], cloud, point_radius=pr, seed=4)
    assert same(q_goal, want_q) and torch.equal(ik_st, want_st)
    assert bool(torch.isnan(traj[~valid & (plan_st != 0)]).all())
    if bool(valid.any()):
        v = traj[valid]
        assert torch.equal(v[:, 0], prob["q"][valid]) and torch.equal(v[:, -1], q_goal[valid])
        assert not bool(coll().check_cloud(v.contiguous(), cloud[valid].contiguous(), point_radius=pr).any())
    ok = ik_st == 0
    assert bool(ok.any())
    assert_reaches(q_goal[ok], prob["target_pose"][ok], "plan_to_poses goals")
    # options reach both calls
    again = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, T=T, seed=4,
                                  ik_options=dict(check_self=True), plan_options=dict(candidates=8))
    assert all(same(out[k].float(), again[k].float()) for k in out)
