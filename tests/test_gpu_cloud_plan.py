"""GPU: ``mpx_franka_plan_cloud`` (csrc/cloud_field.hip) against ``mpx_franka_plan`` where the two must agree bit for
bit (no usable point), against the float64 restatement (tests/float64_cloud_plan.py) for one iteration, against
``FrankaCollisionSampler.check_cloud`` for validity, and at its edges.  One module-scoped fixture per scenario: a launch
runs once."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_plan as fcp  # noqa: E402
import float64_plan as fp  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_cloud_plan_host import CLOUD_ONE_STEP_REFERENCE, DETOUR_PLANNED, DETOUR_SOLVED, LEFT_OUT_CAP, ONE_STEP_POINT_RADIUS, \
    RECORDED_DISAGREEMENTS, SHARE_PLANNED, SHARE_POINT_RADIUS, SHARE_SCENES, SHARE_SEED, SHARE_SOLVED, mixed_problems, \
    one_step_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SUBSTEPS, MARGIN = 4, 1e-4


def dev():
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same(a, b):
    """Bit-equal, NaN included."""
    if a.dtype.is_floating_point:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def grid_dict(g):
    return {"lo": np.array([g.lo[0], g.lo[1], g.lo[2]], np.float32), "h": np.float32(g.h), "nx": g.nx, "ny": g.ny, "nz": g.nz,
            "trunc": np.float32(g.trunc)}


def build_field(cloud, point_radius, counts=None, **kw):
    from mpinets_amd import robot
    from mpinets_amd.field import CloudField

    return CloudField.build(cloud, counts, truncation=robot.plan_cloud_truncation(point_radius, **kw))


@pytest.mark.parametrize("T", [8, 50])
@pytest.mark.parametrize("how", ["counts0", "N0"])
def test_empty_cloud_is_the_planner_without_primitives(T, how):
    """No usable point: every output equals ``robot.franka_plan(cuboids=None, cylinders=None)`` on the same inputs bit for
    bit (the field is trunc everywhere: every sphere is saturated, g is zero, the flag calls find nothing)."""
    from mpinets_amd import robot, scenes

    torch.cuda.set_device(0)
    B, K = 65, 8
    qs, qg = up(scenes.random_configurations(B, 61)), up(scenes.random_configurations(B, 62))
    if how == "counts0":
        cloud = up(np.random.default_rng(1).uniform(-0.5, 0.5, size=(B, 64, 3)).astype(np.float32))
        counts = torch.zeros(B, dtype=torch.int32, device=dev())
    else:
        cloud, counts = torch.zeros((B, 0, 3), dtype=torch.float32, device=dev()), None
    got = robot.franka_plan_cloud(qs, qg, cloud, counts, T=T, seed=7, env_offset=3, return_all=True, candidates=K)
    want = robot.franka_plan(qs, qg, None, None, T=T, seed=7, env_offset=3, return_all=True, candidates=K)
    for name, g, w in zip(("traj", "status", "choice", "all_traj", "all_status"), got, want):
        assert same(g, w), name
    assert int((want[1] == 0).sum()) > 0 and int((want[1] == 2).sum()) > 0  # (solved rows and refused rows both occur)


@pytest.fixture(scope="module")
def one_step(oracle):
    from mpinets_amd import robot

    torch.cuda.set_device(0)
    scn, qs, qg, cloud, start_host = one_step_inputs(oracle)
    c = up(cloud)
    field = build_field(c, ONE_STEP_POINT_RADIUS)
    kw = dict(field=field, point_radius=ONE_STEP_POINT_RADIUS, seed=5, env_offset=1000, return_all=True)
    drawn = robot.franka_plan_cloud(up(qs), up(qg), c, iterations=0, **kw)
    stepped = robot.franka_plan_cloud(up(qs), up(qg), c, iterations=1, **kw)
    return qs, qg, start_host, field, drawn, stepped


def test_one_iteration_against_float64(one_step):
    """All 8 candidates of 16 mixed-scene problems against their 4096-point clouds, on the device's own field and own
    candidates: one iteration is within 4 x CLOUD_ONE_STEP_REFERENCE (tests/test_cloud_plan_host.py: the float32 against
    the float64 run of the restatement) of the float64 restatement, waypoints with a sphere on a discontinuity left out
    (d within 1e-5 m of 0 or epsilon, D within 1e-5 of trunc, a centre within 1e-5 cells of a face; at most 1 %)."""
    qs, qg, start_host, field, drawn, stepped = one_step
    planned = (drawn[1] != 2).cpu().numpy()
    assert planned.mean() >= 0.75  # (an endpoint the CPU solved against the primitives can touch the cloud's 1 cm balls)
    c0 = drawn[3].cpu().numpy()
    assert np.abs(c0[planned] - start_host[planned]).max() <= 2e-6
    assert np.array_equal(c0[planned][:, 0], fp.line(qs, qg, 50)[planned])
    lim = torch.from_numpy(fp.limits32(ft.JOINT_LIMITS_REAL)).double()
    f = field.values.cpu().numpy()[planned]
    ref, fragile = fcp.step(torch.from_numpy(c0[planned]).double(), torch.from_numpy(fp.line(qs, qg, 50)[planned]).double(), f,
                            grid_dict(field.grid), lim[:, 0], lim[:, 1], ONE_STEP_POINT_RADIUS, want_fragile=True)
    got = stepped[3].cpu().double()[torch.from_numpy(planned)]
    d = (got - ref).abs().amax(-1)[:, :, 1:-1]
    print(f"one iteration against a cloud: max {float(d[~fragile].max()):.3e} (bar {4 * CLOUD_ONE_STEP_REFERENCE:.2e}), median "
          f"{float(d.median()):.3e}, left out {float(fragile.float().mean()):.4f}")
    assert float(fragile.float().mean()) <= LEFT_OUT_CAP
    assert float(d[~fragile].max()) <= 4 * CLOUD_ONE_STEP_REFERENCE
    assert float((ref - torch.from_numpy(c0[planned]).double()).abs().max()) > 1e-3  # (the step moved something)
    assert torch.equal(got[:, :, 0], torch.from_numpy(c0[planned][:, :, 0]).double())  # endpoints untouched
    assert torch.equal(got[:, :, -1], torch.from_numpy(c0[planned][:, :, -1]).double())


@pytest.fixture(scope="module")
def share(oracle):
    from mpinets_amd import robot

    torch.cuda.set_device(0)
    scn, qs, qg, cloud = mixed_problems(oracle, SHARE_SCENES, SHARE_SEED)
    c = up(cloud)
    out = robot.franka_plan_cloud(up(qs), up(qg), c, point_radius=SHARE_POINT_RADIUS, return_all=True)
    return scn, qs, qg, c, out


def test_validity_is_the_cloud_collision_check(share):
    """Every candidate of every planned problem: refined on the host with the fma emulation and judged by ``check_cloud``
    at (point_radius, float32(clearance + check_margin)) -- bit 0 of all_status is that flag, candidates whose smallest
    distance comes within 1e-6 m of the threshold left out (at most 2 %).  Solved rows are also free by ``check_cloud`` with
    the plain clearance on a refinement in other arithmetic (float64, cast to float32)."""
    from mpinets_amd.robot import FrankaCollisionSampler

    scn, qs, qg, c, (traj, status, choice, all_traj, all_status) = share
    planned = status != 2
    assert int(planned.sum()) > 0
    at = all_traj[planned]
    n, K = at.shape[:2]
    fine = up(fcp.refine32(at.cpu().numpy(), SUBSTEPS)).reshape(n * K, -1, 7)
    clouds = c[planned].repeat_interleave(K, 0)
    sampler = FrankaCollisionSampler(dev())
    reach = float(np.float32(0.0) + np.float32(MARGIN))
    hit, dist = sampler.check_cloud(fine, clouds, point_radius=SHARE_POINT_RADIUS, clearance=reach, return_distance=True)
    gap = (dist - (sampler.radii + reach)).reshape(n * K, -1).amin(1)
    undecided = gap.abs() <= fcp.DECIDE
    bit = (all_status[planned].reshape(-1) & 1) != 0
    print(f"validity: {n} x {K} candidates, {int(bit.sum())} flagged, {int(undecided.sum())} within 1e-6 m of the threshold")
    assert float(undecided.float().mean()) <= fcp.UNDECIDED_CAP
    assert torch.equal(bit[~undecided], hit[~undecided])
    assert int(bit.sum()) > 0 and int((~bit).sum()) > 0
    ok = status == 0
    rows = torch.nonzero(ok)[:, 0]
    other = fp.refine(traj[rows].double().cpu(), SUBSTEPS).float().to(dev()).contiguous()
    assert not bool(sampler.check_cloud(other, c[rows], point_radius=SHARE_POINT_RADIUS).any())
    assert same(traj[rows], all_traj[rows, choice[rows].long()])
    assert bool((all_status[rows, choice[rows].long()] == 0).all())
    free = all_status == 0
    first = torch.where(free.any(1) & planned, free.int().argmax(1), torch.full_like(choice, -1)).int()
    assert torch.equal(first, choice)
    assert bool(torch.isnan(traj[~ok]).all()) and not bool(torch.isnan(traj[ok]).any())
    assert torch.equal(traj[rows, 0], up(qs)[rows]) and torch.equal(traj[rows, -1], up(qg)[rows])


def test_solved_share_in_scenes_against_the_restatement(share):
    """The device solves at least the float64 restatement's count on the same problems (recorded by
    tests/test_cloud_plan_host.py) minus max(2, 2 x the recorded float32 / float64 disagreements)."""
    scn, qs, qg, c, (traj, status, choice, all_traj, all_status) = share
    n_dev = int((status == 0).sum())
    print(f"{len(qs)} mixed-scene clouds: device solved {n_dev}, planned {int((status != 2).sum())}; float64 restatement "
          f"{SHARE_SOLVED} of {SHARE_PLANNED} planned")
    assert n_dev >= SHARE_SOLVED - max(2, 2 * RECORDED_DISAGREEMENTS)


def test_forced_detour():
    """The wall of test_gpu_plan.py's forced detour drawn as a cloud (a 2 cm lattice with 2 cm balls).  With
    iterations = 0 candidate 0, the straight line, is flagged; with the defaults the solved rows' choice is a valid
    candidate that is not the line, and the device solves at least the restatement's count minus the margin."""
    from mpinets_amd import robot
    from mpinets_amd.robot import FrankaCollisionSampler

    torch.cuda.set_device(0)
    qs, qg, lim, cloud, _ = fcp.detour_problems()
    c = up(cloud)
    kw = dict(point_radius=fcp.WALL_POINT_RADIUS, seed=9, limits=lim, return_all=True)
    drawn = robot.franka_plan_cloud(up(qs), up(qg), c, iterations=0, **kw)
    planned = drawn[1] != 2
    assert int(planned.sum()) > 0 and bool(((drawn[4][planned, 0] & 1) != 0).all())
    traj, status, choice, all_traj, all_status = robot.franka_plan_cloud(up(qs), up(qg), c, **kw)
    ok = status == 0
    rows = torch.nonzero(ok)[:, 0]
    n_dev = int(ok.sum())
    print(f"forced detour as a cloud, {len(qs)} problems: device solved {n_dev} of {int(planned.sum())} planned, choice "
          f"histogram {torch.bincount(choice[ok], minlength=8).tolist()}; float64 restatement {DETOUR_SOLVED} of {DETOUR_PLANNED}")
    assert n_dev > 0 and bool((choice[rows] >= 0).all()) and bool((all_status[rows, choice[rows].long()] == 0).all())
    L = up(fp.line(qs, qg, 50))
    assert bool(((traj[rows] - L[rows]).abs().amax(dim=(1, 2)) > 1e-3).all())
    fine = fp.refine(traj[rows].double().cpu(), SUBSTEPS).float().to(dev()).contiguous()
    assert not bool(FrankaCollisionSampler(dev()).check_cloud(fine, c[rows], point_radius=fcp.WALL_POINT_RADIUS).any())
    assert n_dev >= DETOUR_SOLVED - max(2, 2 * RECORDED_DISAGREEMENTS)


def test_status_2_for_an_endpoint_inside_a_cluster():
    """A cluster of points on the sphere centres of the start (problem 0) or the goal (problem 1): status 2, NaN rows,
    all_status 7; problem 2's cloud is far away and it is planned."""
    from mpinets_amd import robot
    from mpinets_amd.robot import FrankaCollisionSampler

    torch.cuda.set_device(0)
    q0 = np.array([0.0, -0.5, 0.0, -2.0, 0.0, 1.6, 0.8], np.float32)
    q1 = np.array([0.6, -0.2, 0.3, -1.7, 0.2, 1.9, 0.1], np.float32)
    qs, qg = up(np.stack([q0, q0, q0])), up(np.stack([q1, q1, q1]))
    sampler = FrankaCollisionSampler(dev())
    cs, cg = sampler.sphere_centers(qs[:1])[0], sampler.sphere_centers(qg[:1])[0]
    cloud = torch.stack([cs, cg, cs + 5.0])
    traj, status, choice, all_traj, all_status = robot.franka_plan_cloud(qs, qg, cloud, return_all=True)
    assert status.tolist()[:2] == [2, 2] and int(status[2]) != 2
    assert bool(torch.isnan(traj[:2]).all()) and bool(torch.isnan(all_traj[:2]).all())
    assert bool((all_status[:2] == 7).all()) and choice.tolist()[:2] == [-1, -1]
    assert not bool(torch.isnan(all_traj[2]).any())


def _guarded(shape, dtype, fill):
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev())
    return whole, whole[1:-1]


@pytest.mark.parametrize("B", [0, 1, 65])
@pytest.mark.parametrize("T", [2, 8, 64])
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("substeps", [1, 4])
def test_edges_sizes_and_guard_rows(B, T, K, substeps):
    """Every output buffer is written exactly: guard rows around traj / status / choice / all_traj / all_status and guard
    bytes behind the scratch keep their fill; an endpoint in the cloud, outside the limits or NaN gives status 2."""
    from mpinets_amd import _lib, robot, scenes
    from mpinets_amd.field import CloudField
    from mpinets_amd.robot import FrankaCollisionSampler

    torch.cuda.set_device(0)
    N, pr = 300, 0.01
    rng = np.random.default_rng(100 + B + T)
    cloud = up((fcp.fcf.REACH_LO + rng.random((B, N, 3), dtype=np.float32) * (fcp.fcf.REACH_HI - fcp.fcf.REACH_LO)).astype(np.float32))
    qs, qg = up(scenes.random_configurations(B, 41)), up(scenes.random_configurations(B, 42))
    if B == 65:
        qs[3, 2] = float("nan")
        qg[4, 0] = 3.0  # outside the limits
        cloud[5, :56] = FrankaCollisionSampler(dev()).sphere_centers(qs[5:6])[0]  # the start sits in a cluster
    field = CloudField.build(cloud, voxel=0.06, truncation=robot.plan_cloud_truncation(pr, voxel=0.06))
    lim = up(ft.limits_float32_inward(ft.JOINT_LIMITS_REAL))
    sc, sr, sl = robot._ik_sphere_table(dev(), False)
    (wt, traj), (ws, status), (wc, choice) = _guarded((B, T, 7), torch.float32, 7.0), _guarded((B,), torch.int32, -9), \
        _guarded((B,), torch.int32, -9)
    (wa, all_traj), (wb, all_status) = _guarded((B, K, T, 7), torch.float32, 7.0), _guarded((B, K), torch.int32, -9)
    nbytes = int(_lib.load().mpx_franka_plan_cloud_scratch(B, T, K, substeps))
    scratch = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device=dev())
    opt = _lib.PlanOptions(K, 3, 2e-4, 20.0, 0.05, 0.5, substeps, 1e-4, 0.0, 0.15, 1)
    _lib.call("mpx_franka_plan_cloud", _lib.ptr(qs), _lib.ptr(qg), B, T, ft.FINGER_OPENING, _lib.ptr(lim), _lib.ptr(sc),
              _lib.ptr(sr), _lib.ptr(sl), int(sc.size(0)), _lib.ptr(field.values), ctypes.byref(field.grid), _lib.ptr(cloud),
              N * 3, 3, N, None, pr, ctypes.byref(opt), 1, 0, _lib.ptr(traj), _lib.ptr(status), _lib.ptr(choice),
              _lib.ptr(all_traj), _lib.ptr(all_status), _lib.ptr(scratch), nbytes)
    torch.cuda.synchronize()
    for whole, fill in ((wt, 7.0), (wa, 7.0), (ws, -9), (wc, -9), (wb, -9)):
        assert bool((whole[0] == fill).all()) and bool((whole[-1] == fill).all())
    assert bool((scratch[nbytes:] == 0x5A).all())
    if B == 0:
        return
    assert bool(((status >= 0) & (status <= 2)).all())
    ok = status == 0
    assert not bool(torch.isnan(traj[ok]).any()) and bool(torch.isnan(traj[~ok]).all())
    assert bool((choice[ok] >= 0).all()) and bool((choice[~ok] == -1).all())
    assert torch.equal(traj[ok][:, 0], qs[ok]) and torch.equal(traj[ok][:, -1], qg[ok])
    planned = status != 2
    assert not bool(torch.isnan(all_traj[planned]).any()) and bool(((all_status[planned] >= 0) & (all_status[planned] < 8)).all())
    assert same(traj[ok], all_traj[ok, choice[ok].long()])
    if B == 65:
        assert status[3:6].tolist() == [2, 2, 2]
        assert bool(torch.isnan(all_traj[3:6]).all()) and bool((all_status[3:6] == 7).all())
    # without the optional outputs: the same traj and status
    t2, s2 = torch.empty_like(traj), torch.empty_like(status)
    _lib.call("mpx_franka_plan_cloud", _lib.ptr(qs), _lib.ptr(qg), B, T, ft.FINGER_OPENING, _lib.ptr(lim), _lib.ptr(sc),
              _lib.ptr(sr), _lib.ptr(sl), int(sc.size(0)), _lib.ptr(field.values), ctypes.byref(field.grid), _lib.ptr(cloud),
              N * 3, 3, N, None, pr, ctypes.byref(opt), 1, 0, _lib.ptr(t2), _lib.ptr(s2), None, None, None, _lib.ptr(scratch),
              nbytes)
    assert same(t2, traj) and torch.equal(s2, status)


def test_determinism_sharding_seeds_and_slabs(share, monkeypatch):
    from mpinets_amd import robot, solvers

    scn, qs, qg, c, want = share
    a, b = up(qs), up(qg)
    kw = dict(point_radius=SHARE_POINT_RADIUS, return_all=True)
    again = robot.franka_plan_cloud(a, b, c, **kw)
    for g, w in zip(again, want):
        assert same(g, w)
    n = len(qs) // 2
    lo = robot.franka_plan_cloud(a[:n], b[:n], c[:n], **kw)
    hi = robot.franka_plan_cloud(a[n:], b[n:], c[n:], env_offset=n, **kw)
    for x, z, w in zip(lo, hi, want):
        assert same(torch.cat([x, z]), w)
    # slabs of problems (scratch held below a small bound): the same rows
    per = int(robot._lib.load().mpx_franka_plan_cloud_scratch(1, 50, 8, 4))
    monkeypatch.setattr(solvers, "PLAN_CLOUD_SCRATCH_BYTES", 5 * per)  # (the module that owns it: ``robot`` re-exports a copy)
    slabbed = robot.franka_plan_cloud(a, b, c, **kw)
    for g, w in zip(slabbed, want):
        assert same(g, w)
    # the scene rows of the xyz slab, read in place, with counts = N: the same rows
    slab = torch.zeros((len(qs), 6272, 4), dtype=torch.float32, device=dev())
    slab[:, 2048:6144, :3] = c
    counts = torch.full((len(qs),), 4096, dtype=torch.int32, device=dev())
    inplace = robot.franka_plan_cloud(a, b, slab[:, 2048:6144, :3], counts, **kw)
    for g, w in zip(inplace, want):
        assert same(g, w)
    other = robot.franka_plan_cloud(a, b, c, seed=3, iterations=0, **kw)
    drawn = robot.franka_plan_cloud(a, b, c, seed=0, iterations=0, **kw)
    planned = drawn[1] != 2
    assert torch.equal(other[3][planned][:, 0], drawn[3][planned][:, 0])
    assert not torch.equal(other[3][planned][:, 1:], drawn[3][planned][:, 1:])


def test_dataset_from_clouds():
    """``make_problem_batch(expert=True, expert_from="cloud")`` runs and ``problems_to_dataset`` accepts the result;
    ``expert_from="primitives"`` equals a call without the argument bit for bit."""
    from mpinets_amd import scenes
    from mpinets_amd.robot import FrankaCollisionSampler

    torch.cuda.set_device(0)
    kw = dict(seed=4, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16, collision_free=True, expert=True)
    prob = scenes.make_problem_batch(8, expert_from="cloud", **kw)
    ev, sol = prob["expert_valid"], prob["global_solutions"]
    assert sol.shape == (8, 50, 7) and ev.dtype == torch.bool and bool((~ev | prob["valid"]).all())
    assert bool(torch.isnan(sol[~ev]).all()) and not bool(torch.isnan(sol[ev]).any())
    print(f"expert_from='cloud': {int(prob['valid'].sum())} of 8 posed, {int(ev.sum())} planned")
    if int(ev.sum()):
        assert torch.equal(sol[ev][:, 0], prob["q"][ev]) and torch.equal(sol[ev][:, -1], prob["q_goal"][ev])
        fine = fp.refine(sol[ev].double().cpu(), SUBSTEPS).float().to(dev()).contiguous()
        hit = FrankaCollisionSampler(dev()).check_cloud(fine, prob["xyz"][ev][:, 2048:6144, :3].contiguous(),
                                                        point_radius=scenes.EXPERT_CLOUD_POINT_RADIUS)
        assert not bool(hit.any())
    arrays = scenes.problems_to_dataset(prob)
    assert arrays["global_solutions"].shape == (int(ev.sum()), 50, 7)
    a = scenes.make_problem_batch(8, expert_from="primitives", **kw)
    b = scenes.make_problem_batch(8, **kw)
    assert set(a) == set(b) == set(prob)
    assert all(same(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
