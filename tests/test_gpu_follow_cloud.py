"""GPU: ``mpx_franka_follow_cloud`` (csrc/follow_cloud.hip) -- the reactive follower (a stand-in for the reference's Geometric
Fabrics expert, NOT Lula) against a point cloud: the cloud's distance field steers, ``check_cloud``'s kernel judges --
against the float64 restatement (tests/float64_follow_cloud.py), against ``franka_follow`` where there is no environment,
chunked, in slabs, on strided clouds, at its edges, and through ``make_problem_batch(hybrid_against="cloud")`` and
``capture.plan_to_poses(follow=True)``.

Inputs: ``float64_follow_cloud.problems(32, PROBLEM_SEED)`` -- the 32 starts, goals and 8-pose guides of
``float64_follow.problems`` with the 0.1 m cube drawn as a cloud (its 152-point surface lattice, 2 cm apart, ``point_radius``
0.02) on the default grid.  The float64 runs of the restatement and the bars come from tests/test_follow_cloud_host.py
(computed once per session, never written).  Both sides of a comparison read the same nodes: the one-step test hands the
restatement the field the DEVICE built, the whole-rollout test hands the device the field the HOST built."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_plan as fcp  # noqa: E402
import float64_follow as ff  # noqa: E402
import float64_follow_cloud as ffc  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_follow_cloud_host import LEFT_OUT_CAP, ONE_STEP_LEFT_OUT_CAP, ONE_STEP_REFERENCE, ROLLOUT_REFERENCE, T, \
    VERDICT_LEFT_OUT_CAP, one_step, one_step_states, shared_problems  # noqa: E402

pytestmark = pytest.mark.gpu

OUTPUTS = ("traj", "status", "bits", "steps", "traj_any", "path", "arc", "q_end", "v_end", "progress_end")
PR = ffc.POINT_RADIUS
REACH = float(np.float32(0.0) + np.float32(1e-4))  # clearance + check_margin of the defaults, summed in float32
MARGIN_ROUNDING = dict(check_margin=2e-6, max_jerk=1e-5, miss_tol=1e-5)  # test 3's leave-out rule: metres, relative, relative


def dev():
    return torch.device("cuda:0")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def follow(q, poses, cloud, counts=None, field=None, **kw):
    """``robot.franka_follow_cloud`` with every output -> dict by name."""
    from mpinets_amd import robot

    return dict(zip(OUTPUTS, robot.franka_follow_cloud(q, poses, cloud, counts, field, kw.pop("point_radius", PR), T=kw.pop("T", T),
                                                       return_path=True, return_state=True, **kw)))


def same(a, e):
    a, e = a.float(), e.float()
    return torch.equal(torch.nan_to_num(a), torch.nan_to_num(e)) and torch.equal(torch.isnan(a), torch.isnan(e))


def written(out, name):
    """path / arc over the rows that are written, everything else whole."""
    t = out[name]
    if name in ("path", "arc"):
        keep = torch.arange(t.size(1), device=t.device)[None, :] <= out["steps"][:, None]
        return t[keep]
    return t


def env_hit(traj, cloud, counts=None, reach=REACH):
    """``check_cloud`` on the refined configurations of traj [N,T,7] (float32, the device's fma) -> bool [N]."""
    from mpinets_amd.robot import FrankaCollisionSampler

    fine = gpu(fcp.refine32(traj.cpu().numpy(), 4))
    return FrankaCollisionSampler(dev()).check_cloud(fine, cloud, counts, point_radius=PR, clearance=reach)


@pytest.fixture(scope="module")
def runs():
    """One launch per scenario on the 32 problems: the cube's cloud with its field (the defaults, and ``repel = 0``), no
    environment, the field alone, the cloud alone."""
    from mpinets_amd import robot
    from mpinets_amd.field import CloudField

    torch.cuda.set_device(0)
    qs, _, guide, cloud, _ = shared_problems()
    q, g, c = gpu(qs), gpu(guide), gpu(cloud)
    B = q.size(0)
    field = CloudField.build(c, truncation=robot.plan_cloud_truncation(PR))
    zero = torch.zeros(B, dtype=torch.int32, device=dev())
    empty = CloudField.build(c, zero, truncation=robot.plan_cloud_truncation(PR))
    host = (field.values.cpu().numpy(), dict(lo=np.asarray(list(field.grid.lo), np.float32), h=field.grid.h, nx=field.grid.nx,
                                             ny=field.grid.ny, nz=field.grid.nz, trunc=field.grid.trunc))
    return {"q": q, "guide": g, "cloud": c, "field": field, "empty": empty, "zero": zero, "host_field": host,
            "cube": follow(q, g, c, field=field), "repel0": follow(q, g, c, field=field, repel=0.0),
            "free": follow(q, g, c, zero), "steered": follow(q, g, c, zero, field=field),
            "judged": follow(q, g, c, field=empty)}


def test_the_device_field_is_the_hosts(runs):
    """The grid ``franka_follow_cloud`` builds by default is the one the host restates, and its nodes are the host's to
    float32 rounding of a distance (the build's contract is tested in test_gpu_cloud_field.py)."""
    from test_follow_cloud_host import host_field

    field, grid = host_field()
    dfield, dgrid = runs["host_field"]
    assert (dgrid["nx"], dgrid["ny"], dgrid["nz"]) == (grid["nx"], grid["ny"], grid["nz"])
    assert np.float32(dgrid["trunc"]) == np.float32(grid["trunc"]) and np.float32(dgrid["h"]) == np.float32(grid["h"])
    assert np.abs(dfield - field).max() <= 1e-6


def test_one_step_teacher_forced(runs):
    """Every 16th state of the float64 rollout (tests/test_follow_cloud_host.py's, computed once), rounded to float32, with
    max_steps = 1, v_init and progress against the DEVICE-built field: q' and v' within 4 x ONE_STEP_REFERENCE (1.2e-7 rad,
    7.8e-6 rad/s) of the float64 step from the same float32 state on that same field, progress and steps equal, fragile
    states left out (at most 2 %), and the obstacle term moves something."""
    states = one_step_states()
    rows, q, v, pg = states
    field, grid = runs["host_field"]
    q64, v64, p64, fragile, repel = one_step(torch.float64, field, grid, states)
    assert fragile.mean() <= ONE_STEP_LEFT_OUT_CAP and repel.max() > 1e-3
    r = gpu(rows)
    # (one environment per state: the field rows are gathered, 760 kB each -- in chunks, so that no more than 256 are held)
    got = {k: [] for k in ("q_end", "v_end", "progress_end", "steps", "status")}
    from mpinets_amd.field import CloudField

    for at in range(0, len(rows), 256):
        sl = slice(at, at + 256)
        f = CloudField(runs["field"].values[r[sl]].contiguous(), runs["field"].grid)
        out = follow(gpu(q[sl]), runs["guide"][r[sl]], runs["cloud"][r[sl]], field=f, v_init=gpu(v[sl]), progress=gpu(pg[sl]),
                     max_steps=1)
        for k in got:
            got[k].append(out[k].cpu())
    got = {k: torch.cat(t) for k, t in got.items()}
    assert bool((got["status"] != 2).all())
    keep = ~fragile
    dq = np.abs(got["q_end"].double().numpy() - q64).max(-1)
    dv = np.abs(got["v_end"].double().numpy() - v64).max(-1)
    print(f"one step, {len(rows)} states: max |dq'| {dq[keep].max():.3e} (bar {4 * ONE_STEP_REFERENCE['q']:.1e}), max |dv'| "
          f"{dv[keep].max():.3e} (bar {4 * ONE_STEP_REFERENCE['v']:.1e}), left out {fragile.mean():.4f}, largest |repel g| "
          f"{repel.max():.2f}")
    assert np.array_equal(got["progress_end"].numpy()[keep], p64[keep])
    assert np.array_equal(got["steps"].numpy()[keep], 1 - p64[keep, 2])  # (a state that stops takes no step)
    assert dq[keep].max() <= 4 * ONE_STEP_REFERENCE["q"]
    assert dv[keep].max() <= 4 * ONE_STEP_REFERENCE["v"]


def test_whole_rollouts_against_float64(runs):
    """Step counts and progress_end equal and the dense path within 4 x ROLLOUT_REFERENCE (9.1e-6 rad: the bar is 3.64e-5)
    of the float64 restatement.  Both sides read ONE field: the device is handed the host-built one, so the reference is the
    host test's float64 run (computed once) and the rows left out for a fragile step are the ones measured on the CPU, 7 of
    32; the cap is that share plus 5 points and at most 25 %."""
    from mpinets_amd.field import CloudField
    from test_follow_cloud_host import host_field, reference

    field, _ = host_field()
    ref = reference()
    out = follow(runs["q"], runs["guide"], runs["cloud"], field=CloudField(gpu(field), runs["field"].grid))
    fragile = ref["fragile"].any(1)
    assert fragile.mean() <= LEFT_OUT_CAP <= 0.25
    keep = ~fragile
    steps = out["steps"].cpu().numpy()
    path = out["path"].double().cpu().numpy()
    worst = 0.0
    for b in np.nonzero(keep)[0]:
        n = int(ref["steps"][b])
        if steps[b] == n:
            worst = max(worst, float(np.abs(path[b, :n + 1] - ref["path"][b, :n + 1]).max()))
    print(f"steps {steps.min()} .. {steps.max()}, {int(fragile.sum())} rows left out, dense path within {worst:.3e} rad of float64 "
          f"(bar {4 * ROLLOUT_REFERENCE:.2e}), steps differ on {int((steps != ref['steps'])[keep].sum())} kept rows")
    assert np.array_equal(steps[keep], ref["steps"][keep])
    assert np.array_equal(out["progress_end"].cpu().numpy()[keep], ref["progress_end"][keep])
    assert worst <= 4 * ROLLOUT_REFERENCE


@pytest.mark.parametrize("kind", ["cube", "repel0"])
def test_retiming_and_verdict_on_the_devices_own_path(runs, kind):
    """traj_any within 2e-6 rad of the restatement's retiming of the DEVICE's path and arc; waypoints 0 and T-1 bit-equal
    to path[0] and path[n]; bits = the restatement's jerk, self and miss bits on the device's trajectory plus the ENV bit of
    an independent ``check_cloud`` call on its refined configurations with the same point_radius and reach; rows whose
    verdict changes when the margins move by their own rounding (MARGIN_ROUNDING) are left out, at most 2 %."""
    out = runs[kind]
    steps = out["steps"].cpu().numpy()
    path, arc = out["path"].cpu().numpy(), out["arc"].cpu().numpy()
    for b, n in enumerate(steps):  # (rows behind n are not written: keep them out of the arithmetic)
        path[b, n + 1:], arc[b, n + 1:] = 0, 0
    got = out["traj_any"].cpu().numpy()
    want = ff.retime(path, arc, steps, T)
    print(f"{kind}: retimed waypoints within {np.abs(got - want).max():.3e} rad of the float64 retiming")
    assert np.abs(got - want).max() <= 2e-6
    rows = np.arange(len(steps))
    assert np.array_equal(got[:, 0], path[:, 0]) and np.array_equal(got[:, -1], path[rows, steps])
    assert all(arc[b, 0] == 0 and (np.diff(arc[b, :n + 1]) >= 0).all() for b, n in enumerate(steps))
    guide = runs["guide"].cpu().numpy()
    opt = ff.options()
    r = MARGIN_ROUNDING

    def verdict(sign):  # the margins moved by their rounding: +1 makes every test stricter
        o = dict(opt, check_margin=opt["check_margin"] + sign * r["check_margin"], max_jerk=opt["max_jerk"] * (1 - sign * r["max_jerk"]),
                 miss_tol=opt["miss_tol"] * (1 - sign * r["miss_tol"]))
        env = env_hit(out["traj_any"], runs["cloud"], reach=REACH + sign * r["check_margin"]).cpu().numpy()
        return ff.verdict(got, guide, None, o) | env.astype(np.int32) * ffc.BIT_ENV

    bits, loose, tight = verdict(0), verdict(-1), verdict(+1)
    drop = loose != tight
    assert drop.mean() <= VERDICT_LEFT_OUT_CAP
    dbits = out["bits"].cpu().numpy()
    print(f"{kind}: bits histogram {np.bincount(dbits, minlength=16).tolist()}, {int(drop.sum())} rows within the margins' rounding")
    assert np.array_equal(dbits[~drop], bits[~drop])
    assert np.array_equal(out["status"].cpu().numpy(), (dbits != 0).astype(np.int32))
    bad = out["status"] != 0
    assert bool(torch.isnan(out["traj"][bad]).all()) and same(out["traj"][~bad], out["traj_any"][~bad])
    assert not bool(torch.isnan(out["traj_any"]).any())


def test_an_empty_environment_equals_the_primitive_follower(runs):
    """counts = 0 (the field of an empty cloud: saturated everywhere) through the wrapper, and field = NULL with N = 0
    through the entry: every output bit-equal to ``franka_follow`` without primitives on the same inputs."""
    from mpinets_amd import _lib, robot

    q, g = runs["q"], runs["guide"]
    ref = dict(zip(OUTPUTS, robot.franka_follow(q, g, T=T, return_path=True, return_state=True)))
    for name in OUTPUTS:
        assert same(written(runs["free"], name), written(ref, name)), name
    assert int((ref["status"] == 0).sum()) > 0
    B = q.size(0)
    lim = torch.from_numpy(ft.limits_float32_inward(ft.JOINT_LIMITS_REAL)).to(dev())
    sc, sr, sl = robot._ik_sphere_table(dev(), False)
    f32, i32 = torch.float32, torch.int32
    shapes = dict(path=((B, 1025, 7), f32), arc=((B, 1025), f32), status=((B,), i32), bits=((B,), i32), steps=((B,), i32),
                  traj=((B, T, 7), f32), traj_any=((B, T, 7), f32), q_end=((B, 7), f32), v_end=((B, 7), f32), progress_end=((B, 3), i32))
    for S in (int(sc.size(0)), 0):
        o = {k: torch.full(s, 7 if d is i32 else 7.0, dtype=d, device=dev()) for k, (s, d) in shapes.items()}
        nbytes = int(_lib.load().mpx_franka_follow_cloud_scratch(B, T, 4))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev())
        _lib.call("mpx_franka_follow_cloud", _lib.ptr(q), _lib.ptr(g), B, 8, T, ft.FINGER_OPENING, _lib.ptr(lim),
                  *((_lib.ptr(sc), _lib.ptr(sr), _lib.ptr(sl)) if S else (None, None, None)), S, None, None, None, 0, 3, 0, None,
                  0.0, None, None, None, *(_lib.ptr(o[k]) for k in ("path", "arc", "status", "bits", "steps", "traj", "traj_any",
                                                                      "q_end", "v_end", "progress_end")), buf.data_ptr(), nbytes)
        for name in OUTPUTS:
            assert same(written(o, name), written(ref, name)), (S, name)


def test_the_field_steers_and_the_cloud_judges(runs):
    """A field of the cube with counts = 0: the path differs from free space and no row carries the ENV bit.  A field of an
    empty cloud with the cube as cloud: the path is free space's bit for bit and the ENV bit is ``check_cloud``'s answer on
    that trajectory -- which hits on at least one row."""
    free, steered, judged = runs["free"], runs["steered"], runs["judged"]
    moved = (steered["path"][:, :65] - free["path"][:, :65]).abs().amax((1, 2))  # (every row takes more than 64 steps)
    assert int(torch.minimum(steered["steps"], free["steps"]).min()) >= 64 and float(moved.max()) > 1e-3
    assert int((steered["bits"] & ffc.BIT_ENV).sum()) == 0
    for name in ("path", "arc", "steps", "traj_any", "q_end", "v_end", "progress_end"):
        assert same(written(judged, name), written(free, name)), name
    hit = env_hit(judged["traj_any"], runs["cloud"])
    print(f"the free-space rollouts judged against the cube's cloud: {int(hit.sum())} of {hit.numel()} rows hit")
    assert int(hit.sum()) >= 1
    assert torch.equal((judged["bits"] & ffc.BIT_ENV) != 0, hit)
    assert torch.equal(judged["bits"] & ~ffc.BIT_ENV, free["bits"] & ~ffc.BIT_ENV)
    # (the same rollouts with the field given but switched off: repel = 0 is another way to say it)
    assert same(written(runs["repel0"], "path"), written(free, "path")) and torch.equal(runs["repel0"]["bits"], judged["bits"])


def test_the_obstacle_term_helps(runs):
    """Fewer rows carry the ENV bit with the defaults than with repel = 0: strictly (verified for the restatement on the CPU
    when the seed was chosen, tests/test_follow_cloud_host.py)."""
    with_term = int(((runs["cube"]["bits"] & ffc.BIT_ENV) != 0).sum())
    without = int(((runs["repel0"]["bits"] & ffc.BIT_ENV) != 0).sum())
    print(f"rows with the ENV bit: {with_term} with the defaults, {without} with repel = 0; valid {int((runs['cube']['status'] == 0).sum())} "
          f"against {int((runs['repel0']['status'] == 0).sum())} of 32")
    assert with_term < without


def test_chunked_calls_walk_the_single_calls_path(runs):
    """One call of max_steps = 1024 against four calls of 256 with (q_end, v_end, progress_end) carried over: q_end, v_end,
    progress_end and the concatenated dense path bit for bit; a finished row takes no further step."""
    whole = runs["cube"]
    q, v, pg = runs["q"], None, None
    B = q.size(0)
    at = torch.zeros(B, dtype=torch.long, device=dev())
    path = torch.full_like(whole["path"], float("nan"))
    path[:, 0] = q
    cols = torch.arange(1, 257, device=dev())[None, :]
    for _ in range(4):
        out = follow(q, runs["guide"], runs["cloud"], field=runs["field"], v_init=v, progress=pg, max_steps=256)
        assert bool((out["status"] != 2).all())
        took = cols <= out["steps"][:, None]  # [B,256]
        dst = (at[:, None] + cols)[took]
        path[torch.nonzero(took)[:, 0], dst] = out["path"][:, 1:][took]
        at += out["steps"]
        q, v, pg = out["q_end"], out["v_end"], out["progress_end"]
    assert torch.equal(at.int(), whole["steps"])
    keep = torch.arange(path.size(1), device=dev())[None, :] <= whole["steps"][:, None]
    assert torch.equal(path[keep], whole["path"][keep])
    assert torch.equal(pg, whole["progress_end"]) and torch.equal(q, whole["q_end"]) and torch.equal(v, whole["v_end"])
    done = pg[:, 2] == 1
    assert bool(done.any())
    again = follow(q, runs["guide"], runs["cloud"], field=runs["field"], v_init=v, progress=pg, max_steps=8)
    assert bool((again["steps"][done] == 0).all()) and torch.equal(again["q_end"][done], q[done])


def test_slabs_and_rows_give_the_batchs_result(runs):
    """B = 32 equals two calls of 16 (each with its own rows of the field), and the run in which FOLLOW_PATH_BYTES forces
    slabs of 5 problems."""
    from mpinets_amd import robot, solvers
    from mpinets_amd.field import CloudField

    q, g, c, field, whole = runs["q"], runs["guide"], runs["cloud"], runs["field"], runs["cube"]
    for half in (slice(0, 16), slice(16, 32)):
        out = follow(q[half], g[half], c[half], field=CloudField(field.values[half], field.grid))
        part = {k: v[half] for k, v in whole.items()}
        for name in OUTPUTS:
            assert same(written(out, name), written(part, name)), name
    saved = solvers.FOLLOW_PATH_BYTES
    solvers.FOLLOW_PATH_BYTES = 5 * 32 * 1025
    try:
        got = robot.franka_follow_cloud(q, g, c, None, field, PR, return_state=True)
    finally:
        solvers.FOLLOW_PATH_BYTES = saved
    for name, t in zip(("traj", "status", "bits", "steps", "q_end", "v_end", "progress_end"), got):
        assert same(t, whole[name]), name


def test_strided_clouds_are_read_in_place(runs):
    """A [B,N,4] cloud and the slice big[:, 100:100+N, :3] of a larger slab give the contiguous copy's result (the field is
    built from each form too)."""
    q, g, c, whole = runs["q"], runs["guide"], runs["cloud"], runs["cube"]
    B, N = c.shape[:2]
    four = torch.full((B, N, 4), 9.0, device=dev())
    four[:, :, :3] = c
    big = torch.full((B, N + 200, 4), float("nan"), device=dev())
    big[:, :100, :3], big[:, 100 + N:, :3] = 0.3, 0.3  # (points the view must not see: inside the arm's reach)
    big[:, 100:100 + N, :3] = c
    for cloud in (four, big[:, 100:100 + N, :3]):
        assert not cloud.is_contiguous() or cloud.size(2) == 4
        out = follow(q, g, cloud)
        for name in OUTPUTS:
            assert same(written(out, name), written(whole, name)), name


def test_bad_input(runs):
    """A start inside the cube's cloud is status 2 only without ``progress`` (with an all-zero one it runs); a NaN pose, a
    start outside the limits and a non-finite v_init give status 2, bits 15, steps 0, NaN traj and the state as given; the
    neighbouring rows are what they are in the whole batch."""
    from oracle import oracle as orc

    qs, _, guide, cloud, _ = shared_problems()
    qs, guide, cloud = qs[:8].copy(), guide[:8].copy(), cloud[:8].copy()
    v = np.zeros((8, 7), np.float32)
    cloud[1] += orc.franka_fk(qs[1:2])[0, ff.RIGHT_GRIPPER, 9:] - cloud[1].mean(0)  # the lattice moved onto row 1's gripper
    guide[3, 4, 1, 2] = np.nan
    qs[5, 0] = 3.0
    v[6, 2] = np.inf
    q, g, c, vi = gpu(qs), gpu(guide), gpu(cloud), gpu(v)
    out = follow(q, g, c, v_init=vi)
    bad = [1, 3, 5, 6]
    assert out["status"].tolist() == [2 if b in bad else out["status"][b].item() for b in range(8)]
    assert bool((out["status"][[0, 2, 4, 7]] != 2).all())
    assert out["bits"][bad].tolist() == [15] * 4 and out["steps"][bad].tolist() == [0] * 4
    assert bool(torch.isnan(out["traj"][bad]).all()) and bool(torch.isnan(out["traj_any"][bad]).all())
    assert same(out["q_end"][bad], q[bad]) and same(out["v_end"][bad], vi[bad]) and bool((out["progress_end"][bad] == 0).all())
    whole = runs["cube"]
    for b in (0, 2, 4, 7):  # (the same cloud, guide and start as in the whole batch: the same row)
        for name in OUTPUTS:
            a, e = out[name][b], whole[name][b]
            n = int(whole["steps"][b])
            if name in ("path", "arc"):
                a, e = a[:n + 1], e[:n + 1]
            assert same(a, e), (b, name)
    again = follow(q, g, c, v_init=vi, progress=torch.zeros(8, 3, dtype=torch.int32, device=dev()), max_steps=16)
    assert again["status"].tolist()[1] != 2 and int(again["steps"][1]) == 16  # a continued rollout may stand in collision
    assert [again["status"][b].item() for b in (3, 5, 6)] == [2, 2, 2]


def test_make_problem_batch_against_the_cloud():
    """``make_problem_batch(8, ..., expert_from="cloud", hybrid=True, hybrid_against="cloud")``: the keys, hybrid_valid within
    expert_valid, every hybrid_valid trajectory free by ``check_cloud`` at the same radius and reach,
    ``problems_to_dataset(prob, "hybrid_solutions")`` keeps exactly those rows, and the call without the two new arguments
    returns what it returns (a second call of the unchanged path)."""
    from mpinets_amd import scenes
    from mpinets_amd.robot import FrankaCollisionSampler, franka_fk, frames_to_matrix

    torch.cuda.set_device(0)
    kw = dict(seed=3, collision_free=True, expert=True, expert_from="cloud")
    plain, again = scenes.make_problem_batch(8, **kw), scenes.make_problem_batch(8, **kw)
    prob = scenes.make_problem_batch(8, hybrid=True, hybrid_against="cloud", **kw)
    assert set(again) == set(plain) and set(prob) - set(plain) == {"hybrid_solutions", "hybrid_valid", "hybrid_target_pose"}
    for k, v in plain.items():
        for other in (again, prob):
            assert same(v, other[k]) if torch.is_tensor(v) else v == other[k], k
    hv, ev = prob["hybrid_valid"], prob["expert_valid"]
    print(f"8 tabletop problems against their scene clouds: expert_valid {int(ev.sum())}, hybrid_valid {int(hv.sum())}")
    assert bool((hv <= ev).all())
    assert prob["hybrid_solutions"].shape == (8, 50, 7) and prob["hybrid_target_pose"].shape == (8, 4, 4)
    assert bool(torch.isnan(prob["hybrid_solutions"][~hv]).all()) and not bool(torch.isnan(prob["hybrid_solutions"][hv]).any())
    arrays = scenes.problems_to_dataset(prob, "hybrid_solutions")
    assert arrays["hybrid_solutions"].shape == (int(hv.sum()), 50, 7) == arrays["global_solutions"].shape
    assert np.array_equal(arrays["hybrid_solutions"], prob["hybrid_solutions"][hv].cpu().numpy())
    if bool(hv.any()):
        traj = prob["hybrid_solutions"][hv]
        fine = gpu(fcp.refine32(traj.cpu().numpy(), 4))
        hit = FrankaCollisionSampler(dev()).check_cloud(fine, prob["xyz"][hv][:, 2048:6144, :3].contiguous(),
                                                        point_radius=scenes.EXPERT_CLOUD_POINT_RADIUS, clearance=REACH)
        assert not bool(hit.any())
        assert torch.equal(traj[:, 0], prob["q"][hv])
        gripper = ft.LINK_ID["right_gripper"]
        assert torch.equal(prob["hybrid_target_pose"][hv], frames_to_matrix(franka_fk(traj[:, -1].contiguous())[:, gripper]))


def test_plan_to_poses_with_the_follower():
    """``capture.plan_to_poses(..., follow=True)`` on 4 rows: the followed trajectories with status 0 pass ``check_cloud``, a
    row without a plan comes back with status 2, and with ``follow=False`` the return is what it was."""
    from mpinets_amd import capture, scenes
    from mpinets_amd.robot import FrankaCollisionSampler

    torch.cuda.set_device(0)
    B, pr = 4, scenes.EXPERT_CLOUD_POINT_RADIUS
    prob = scenes.make_problem_batch(B, device=dev(), device_clouds=True, seed=4, kinds=("tabletop", "cubby", "dresser"), M1=40,
                                     M2=16, collision_free=True)
    cloud = prob["xyz"][:, 2048:6144, :3]
    base = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4)
    out = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4, follow=True)
    assert sorted(base) == ["ik_status", "plan_status", "q_goal", "trajectory", "valid"]
    assert set(out) - set(base) == {"followed_trajectory", "follow_status", "follow_bits", "follow_steps"}
    for k, v in base.items():
        assert same(v, out[k]), k
    st = out["follow_status"]
    print(f"plan_to_poses(follow=True): plan status {out['plan_status'].tolist()}, follow status {st.tolist()}, bits "
          f"{out['follow_bits'].tolist()}, steps {out['follow_steps'].tolist()}")
    assert out["followed_trajectory"].shape == (B, 50, 7) and st.dtype == torch.int32
    assert bool((st[out["plan_status"] != 0] == 2).all())
    ok = st == 0
    assert bool(torch.isnan(out["followed_trajectory"][~ok]).all())
    if bool(ok.any()):
        traj = out["followed_trajectory"][ok]
        fine = gpu(fcp.refine32(traj.cpu().numpy(), 4))
        assert not bool(FrankaCollisionSampler(dev()).check_cloud(fine, cloud[ok].contiguous(), point_radius=pr, clearance=REACH).any())
        assert torch.equal(traj[:, 0], prob["q"][ok])
