"""GPU: ``mpx_franka_follow`` (csrc/follow.hip) -- the reactive follower that stands in for the reference's Geometric
Fabrics expert (NOT Lula), its retiming and its verdict -- against the float64 restatement (tests/float64_follow.py), against
the kernels that predate it, chunked, row by row, at its edges and through ``make_problem_batch(hybrid=True)``.

Inputs: ``float64_follow.problems(32, PROBLEM_SEED)`` -- 32 starts and goals, the guide = the right_gripper poses of the
straight joint line at 8 points, and for the BESIDE-CUBOID problems one 0.1 m cube 0.13 m beside the fourth guide pose (the
construction and the seed are recorded there); the free-space problems are the same rows without the cube.  The float64
runs of the restatement and the bars come from tests/test_follow_host.py (computed once per session, never written)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_follow as ff  # noqa: E402
import float64_plan as fp  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_follow_host import CUBOID_LEFT_OUT_CAP, FREE_LEFT_OUT_CAP, ONE_STEP_LEFT_OUT_CAP, ONE_STEP_REFERENCE, \
    ROLLOUT_REFERENCE, T, one_step, one_step_states, reference, shared_problems  # noqa: E402
from test_gpu_plan import dev, device_scene, judge, prims_of, take  # noqa: E402

pytestmark = pytest.mark.gpu

OUTPUTS = ("traj", "status", "bits", "steps", "traj_any", "path", "arc", "q_end", "v_end", "progress_end")
MARGIN_ROUNDING = dict(check_margin=2e-6, max_jerk=1e-5, miss_tol=1e-5)  # test 3's leave-out rule: metres, relative, relative


def follow(q, poses, cub=None, cyl=None, **kw):
    """``robot.franka_follow`` with every output -> dict by name."""
    from mpinets_amd import robot

    return dict(zip(OUTPUTS, robot.franka_follow(q, poses, cub, cyl, T=kw.pop("T", T), return_path=True, return_state=True, **kw)))


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.fixture(scope="module")
def runs():
    """One launch per scenario: the 32 free-space and the 32 beside-cuboid problems with the default options."""
    torch.cuda.set_device(0)
    qs, qg, guide, scn = shared_problems()
    cub, cyl = prims_of(scn)
    host, device = fp.scene_from_arrays(scn), device_scene(cub, cyl)
    assert all(np.array_equal(host[k], device[k]) for k in host)  # (an axis-aligned cube: both sides read the same frames)
    q, g = gpu(qs), gpu(guide)
    return {"q": q, "guide": g, "cub": cub, "cyl": cyl, "scene": device, "free": follow(q, g), "cuboid": follow(q, g, cub, cyl)}


def test_one_step_teacher_forced(runs):
    """Every 16th state of the float64 rollout beside the cube, rounded to float32, as ONE batch with max_steps = 1,
    v_init and progress: q' and v' within 4 x ONE_STEP_REFERENCE (tests/test_follow_host.py: the float32 against the
    float64 run of the restatement, 1.8e-7 rad and 7.2e-6 rad/s) of the float64 step from the same float32 state, progress
    equal, fragile states left out (at most 2 %; 0.11 % on the CPU), and the obstacle term moves something."""
    rows, q, v, pg = one_step_states()
    q64, v64, p64, fragile, repel = one_step(torch.float64)
    assert fragile.mean() <= ONE_STEP_LEFT_OUT_CAP and repel.max() > 1e-3
    c, y = take((runs["cub"], runs["cyl"]), gpu(rows))
    out = follow(gpu(q), runs["guide"][gpu(rows)], c, y, v_init=gpu(v), progress=gpu(pg), max_steps=1)
    assert bool((out["status"] != 2).all())
    keep = ~fragile
    dq = np.abs(out["q_end"].double().cpu().numpy() - q64).max(-1)
    dv = np.abs(out["v_end"].double().cpu().numpy() - v64).max(-1)
    print(f"one step, {len(rows)} states: max |dq'| {dq[keep].max():.3e} (bar {4 * ONE_STEP_REFERENCE['q']:.1e}), max |dv'| "
          f"{dv[keep].max():.3e} (bar {4 * ONE_STEP_REFERENCE['v']:.1e}), left out {fragile.mean():.4f}")
    assert np.array_equal(out["progress_end"].cpu().numpy()[keep], p64[keep])
    assert np.array_equal(out["steps"].cpu().numpy()[keep], 1 - p64[keep, 2])  # (a state that stops takes no step)
    assert dq[keep].max() <= 4 * ONE_STEP_REFERENCE["q"]
    assert dv[keep].max() <= 4 * ONE_STEP_REFERENCE["v"]


@pytest.mark.parametrize("kind", ["free", "cuboid"])
def test_whole_rollouts_against_float64(runs, kind):
    """Step counts equal and the dense path within 4 x ROLLOUT_REFERENCE (2.7e-5 rad: the bar is 1.08e-4) of the float64
    restatement; rows with any fragile step are left out: at most 10 % in free space (2 of 32 on the CPU), and beside the
    cube what the CPU measurement of the reference alone shows plus 5 points (6 of 32 + 5 % = 23.75 %, below the 25 % at
    which the comparison of the obstacle rows would be dropped: it is kept)."""
    ref, out = reference(kind), runs[kind]
    fragile = ref["fragile"].any(1)
    assert fragile.mean() <= (FREE_LEFT_OUT_CAP if kind == "free" else CUBOID_LEFT_OUT_CAP)
    keep = ~fragile
    steps = out["steps"].cpu().numpy()
    path = out["path"].double().cpu().numpy()
    worst = 0.0
    for b in np.nonzero(keep)[0]:
        n = int(ref["steps"][b])
        if steps[b] == n:
            worst = max(worst, float(np.abs(path[b, :n + 1] - ref["path"][b, :n + 1]).max()))
    print(f"{kind}: steps {steps.min()} .. {steps.max()}, {int(fragile.sum())} rows left out, dense path within {worst:.3e} rad "
          f"of float64 (bar {4 * ROLLOUT_REFERENCE:.2e}), steps differ on {int((steps != ref['steps'])[keep].sum())} kept rows")
    assert np.array_equal(steps[keep], ref["steps"][keep])
    assert worst <= 4 * ROLLOUT_REFERENCE
    assert np.array_equal(out["progress_end"].cpu().numpy()[keep], ref["progress_end"][keep])


@pytest.mark.parametrize("kind", ["free", "cuboid"])
def test_retiming_and_verdict_on_the_devices_own_path(runs, kind):
    """traj_any within 2e-6 rad of the restatement's retiming of the DEVICE's path and arc; waypoints 0 and T-1 bit-equal
    to path[0] and path[n]; bits = float64_plan.validity plus the miss test on the device's trajectory, rows whose verdict
    changes when the margins move by their own rounding (MARGIN_ROUNDING) left out, at most 2 %."""
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
    scene = runs["scene"] if kind == "cuboid" else None
    guide = runs["guide"].cpu().numpy()
    opt = ff.options()
    bits = ff.verdict(got, guide, scene, opt)
    r = MARGIN_ROUNDING

    def moved(sign):  # the margins moved by their rounding: +1 makes every test stricter
        return dict(opt, check_margin=opt["check_margin"] + sign * r["check_margin"],
                    max_jerk=opt["max_jerk"] * (1 - sign * r["max_jerk"]), miss_tol=opt["miss_tol"] * (1 - sign * r["miss_tol"]))

    loose, tight = ff.verdict(got, guide, scene, moved(-1)), ff.verdict(got, guide, scene, moved(+1))
    drop = loose != tight
    assert drop.mean() <= 0.02
    dbits = out["bits"].cpu().numpy()
    print(f"{kind}: bits histogram {np.bincount(dbits, minlength=16).tolist()}, {int(drop.sum())} rows within the margins' rounding")
    assert np.array_equal(dbits[~drop], bits[~drop])
    assert np.array_equal(out["status"].cpu().numpy(), (dbits != 0).astype(np.int32))


def judged_valid(traj, guide_last, cub, cyl):
    """The judges that predate the follower on traj [N,T,7]: ``FrankaCollisionSampler.check`` on the refined
    configurations, ``mpx_trajectory_metrics``' self flag, a third-difference test in float64 and the position miss through
    ``mpx_franka_fk`` -> bool [N] per judge."""
    from mpinets_amd.robot import franka_fk

    env, self_hit, jerk, _ = judge(traj, cub, cyl)
    p = franka_fk(traj[:, -1].contiguous())[:, ft.LINK_ID["right_gripper"], 9:].double()
    miss = torch.linalg.norm(guide_last[:, :3, 3].double() - p, dim=-1)
    return ~env, ~self_hit.bool(), jerk <= 0.15, miss <= 0.05


def test_valid_means_valid_by_the_kernels_that_predate_the_follower(runs):
    """Status-0 rows pass every older judge; status-1 rows have bits and a NaN row; beside the cube the device finds at
    least as many valid rows as the restatement minus the rows left out as fragile.  (CPU, float64: 28 of 32 beside the
    cube, 29 of 32 in free space; the free-space rollouts judged in the cube's scene are printed for context.)"""
    for kind in ("free", "cuboid"):
        out, ref = runs[kind], reference(kind)
        cub, cyl = runs["cub"], runs["cyl"]
        if kind == "free":  # (the judges want primitives: the cube far away)
            cub, cyl = prims_of({k: (v + 50.0 if k == "cuboid_centers" else v) for k, v in shared_problems()[3].items()})
        ok = out["status"] == 0
        rows = torch.nonzero(ok)[:, 0]
        assert rows.numel() > 0
        c, y = take((cub, cyl), rows)
        for name, passed in zip(("env", "self", "jerk", "miss"), judged_valid(out["traj"][rows], runs["guide"][rows, -1], c, y)):
            assert bool(passed.all()), (kind, name)
        assert torch.equal(out["traj"][rows], out["traj_any"][rows])
        bad = out["status"] == 1
        assert bool((out["bits"][bad] != 0).all()) and bool(torch.isnan(out["traj"][bad]).all()) and bool((out["bits"][ok] == 0).all())
        assert not bool(torch.isnan(out["traj_any"][bad]).any()) and int((out["status"] == 2).sum()) == 0
        n_dev, n_ref, left_out = int(ok.sum()), int((ref["status"] == 0).sum()), int(ref["fragile"].any(1).sum())
        line = f"{kind}: device valid {n_dev} of 32, float64 restatement {n_ref}, rows left out {left_out}"
        if kind == "free":
            c, y = take((runs["cub"], runs["cyl"]), rows)
            e, s, j, m = judged_valid(out["traj"][rows], runs["guide"][rows, -1], c, y)
            line += f"; of the free-space rollouts {int((e & s & j & m).sum())} are valid when judged beside the cube"
        print(line)
        assert n_dev >= n_ref - left_out


def test_chunked_calls_walk_the_single_calls_path(runs):
    """One call of max_steps = 1024 against four calls of 256 with (q_end, v_end, progress_end) carried over: the dense
    path bit for bit, progress equal; a finished row takes no further step."""
    whole = runs["cuboid"]
    q, v, pg = runs["q"], None, None
    B = q.size(0)
    at = torch.zeros(B, dtype=torch.long, device=dev())
    path = torch.full_like(whole["path"], float("nan"))
    path[:, 0] = q
    cols = torch.arange(1, 257, device=dev())[None, :]
    for _ in range(4):
        out = follow(q, runs["guide"], runs["cub"], runs["cyl"], v_init=v, progress=pg, max_steps=256)
        assert bool((out["status"] != 2).all())
        took = cols <= out["steps"][:, None]  # [B,256]
        dst = (at[:, None] + cols)[took]
        path[torch.nonzero(took)[:, 0], dst] = out["path"][:, 1:][took]
        at += out["steps"]
        q, v, pg = out["q_end"], out["v_end"], out["progress_end"]
    assert torch.equal(at.int(), whole["steps"])
    written = torch.arange(path.size(1), device=dev())[None, :] <= whole["steps"][:, None]
    assert torch.equal(path[written], whole["path"][written])
    assert torch.equal(pg, whole["progress_end"]) and torch.equal(q, whole["q_end"]) and torch.equal(v, whole["v_end"])
    done = pg[:, 2] == 1
    assert bool(done.any())
    again = follow(q, runs["guide"], runs["cub"], runs["cyl"], v_init=v, progress=pg, max_steps=8)
    assert bool((again["steps"][done] == 0).all()) and torch.equal(again["q_end"][done], q[done])
    assert torch.equal(again["progress_end"][done], pg[done])


def test_rows_do_not_depend_on_the_batch(runs):
    """A batch of 65 (the 32 cube rows, the same 32 with the cube's row dead, one more) against rows 0, 31 and 64 run
    alone: every output bit-equal (path and arc over the rows that are written)."""
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    cub, cyl = runs["cub"], runs["cyl"]
    pick = torch.cat([torch.arange(32), torch.arange(32), torch.tensor([5])]).to(dev())
    dims = cub.dims[pick].clone()
    dims[32:64] = 0  # a dead row: free space
    c65 = TorchCuboids(cub.centers[pick], dims, cub.quats[pick])
    y65 = TorchCylinders(cyl.centers[pick], cyl.radii[pick], cyl.heights[pick], cyl.quats[pick])
    q, g = runs["q"][pick], runs["guide"][pick]
    full = follow(q, g, c65, y65)
    assert torch.equal(full["steps"][:32], runs["cuboid"]["steps"]) and torch.equal(full["steps"][32:64], runs["free"]["steps"])
    assert torch.equal(torch.nan_to_num(full["traj"][32:64]), torch.nan_to_num(runs["free"]["traj"]))  # dead row = no primitives
    for b in (0, 31, 64):
        rows = torch.tensor([b], device=dev())
        c, y = take((c65, y65), rows)
        one = follow(q[rows], g[rows], c, y)
        n = int(full["steps"][b])
        for name in OUTPUTS:
            a, e = full[name][b], one[name][0]
            if name in ("path", "arc"):
                a, e = a[:n + 1], e[:n + 1]
            a, e = a.float(), e.float()
            assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(e)) and torch.equal(torch.isnan(a), torch.isnan(e)), (b, name)


def test_slabs_of_problems_give_the_batchs_result(runs):
    """Without ``return_path`` a bounded path buffer runs the batch in slabs (here 5 problems each): the same rows."""
    from mpinets_amd import robot, solvers

    saved = solvers.FOLLOW_PATH_BYTES
    solvers.FOLLOW_PATH_BYTES = 5 * 32 * 1025
    try:
        got = robot.franka_follow(runs["q"], runs["guide"], runs["cub"], runs["cyl"], return_state=True)
    finally:
        solvers.FOLLOW_PATH_BYTES = saved
    for name, t in zip(("traj", "status", "bits", "steps", "q_end", "v_end", "progress_end"), got):
        a, e = t.float(), runs["cuboid"][name].float()
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(e)) and torch.equal(torch.isnan(a), torch.isnan(e)), name


def _guarded(shape, dtype, fill):
    """A tensor with a guard row in front and behind: -> (whole, view)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev())
    return whole, whole[1:-1]


def _edge_inputs(B, W):
    """B rows of the cube problems (tiled), the guide cut or repeated to W poses; at B = 65 row 3 has a NaN pose, row 4 a
    start outside the limits and row 5 its cube moved onto the gripper of its start."""
    from oracle import oracle as orc

    qs, _, guide, scn = shared_problems()
    pick = np.arange(B) % 32
    qs, guide, scn = qs[pick].copy(), guide[pick].copy(), {k: v[pick].copy() for k, v in scn.items()}
    guide = guide[:, -1:] if W == 1 else np.repeat(guide, W // 8, axis=1)
    if B == 65:
        guide[3, W // 2, 1, 3] = np.nan
        qs[4, 0] = 3.0
        scn["cuboid_centers"][5, 0] = orc.franka_fk(qs[5:6])[0, ff.RIGHT_GRIPPER, 9:]
    return qs, guide, scn


@pytest.mark.parametrize("B", [0, 1, 65])
@pytest.mark.parametrize("W", [1, 8, 64])
@pytest.mark.parametrize("T_", [2, 50, 64])
@pytest.mark.parametrize("max_steps", [1, 37])
def test_edges_sizes_and_guard_rows(B, W, T_, max_steps):
    """Every output buffer is written exactly: guard rows around all ten keep their fill; a NaN pose, a start outside the
    limits and a start in collision give status 2, bits 15, NaN rows, no steps and the state as given."""
    from mpinets_amd import _lib, robot

    torch.cuda.set_device(0)
    qs, guide, scn = _edge_inputs(B, W)
    cub, cyl = prims_of(scn)
    q, g = gpu(qs), gpu(guide)
    lim = torch.from_numpy(ft.limits_float32_inward(ft.JOINT_LIMITS_REAL)).to(dev())
    sc, sr, sl = robot._ik_sphere_table(dev(), False)
    f32, i32, N = torch.float32, torch.int32, max_steps + 1
    shapes = dict(path=((B, N, 7), f32), arc=((B, N), f32), status=((B,), i32), bits=((B,), i32), steps=((B,), i32),
                  traj=((B, T_, 7), f32), traj_any=((B, T_, 7), f32), q_end=((B, 7), f32), v_end=((B, 7), f32),
                  progress_end=((B, 3), i32))
    bufs = {k: _guarded(s, d, 7.0 if d is f32 else -9) for k, (s, d) in shapes.items()}
    opt = robot._follow_options("test", dict(max_steps=max_steps))[0]
    _lib.call("mpx_franka_follow", _lib.ptr(q), _lib.ptr(g), B, W, T_, ft.FINGER_OPENING, _lib.ptr(lim), _lib.ptr(sc), _lib.ptr(sr),
              _lib.ptr(sl), int(sc.size(0)), _lib.ptr(cub.inv_frames), _lib.ptr(cub.dims), 1, _lib.ptr(cyl.inv_frames),
              _lib.ptr(cyl.radii), _lib.ptr(cyl.heights), 1, None, None, ctypes.byref(opt),
              *(_lib.ptr(bufs[k][1]) for k in ("path", "arc", "status", "bits", "steps", "traj", "traj_any", "q_end", "v_end",
                                               "progress_end")))
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        fill = 7.0 if whole.dtype is f32 else -9
        assert bool((whole[0] == fill).all()) and bool((whole[-1] == fill).all()), k
    if B == 0:
        return
    o = {k: v for k, (_, v) in bufs.items()}
    status, steps = o["status"], o["steps"]
    assert bool(((status >= 0) & (status <= 2)).all()) and bool(((steps >= 0) & (steps <= max_steps)).all())
    ok = status == 0
    assert not bool(torch.isnan(o["traj"][ok]).any()) and bool(torch.isnan(o["traj"][~ok]).all())
    assert torch.equal(ok, o["bits"] == 0) and bool((o["bits"][status == 2] == 15).all())
    ran = status != 2
    assert not bool(torch.isnan(o["traj_any"][ran]).any()) and torch.equal(o["traj_any"][ran][:, 0], q[ran])
    assert torch.equal(o["path"][:, 0], q) and bool((o["arc"][:, 0] == 0).all())
    rows = torch.arange(B, device=dev())
    assert torch.equal(o["traj_any"][ran][:, -1], o["path"][rows, steps.long()][ran])
    assert torch.equal(o["q_end"][ran], o["path"][rows, steps.long()][ran])
    if B == 65:
        assert status[3:6].tolist() == [2, 2, 2] and o["bits"][3:6].tolist() == [15, 15, 15] and steps[3:6].tolist() == [0, 0, 0]
        assert bool(torch.isnan(o["traj_any"][3:6]).all()) and torch.equal(o["q_end"][3:6], q[3:6])
        assert bool((o["v_end"][3:6] == 0).all()) and bool((o["progress_end"][3:6] == 0).all())
        assert int((status != 2).sum()) == 62


@pytest.mark.parametrize("form", ["no spheres", "spheres", "dead rows"])
def test_no_live_primitives(runs, form):
    """M1 = M2 = 0 with and without the sphere table, and primitive rows that are all dead: the free-space result."""
    from mpinets_amd import _lib, robot

    q, g, ref = runs["q"], runs["guide"], runs["free"]
    if form == "dead rows":
        scn = {k: v.copy() for k, v in shared_problems()[3].items()}
        scn["cuboid_dims"][:] = 0
        out = follow(q, g, *prims_of(scn))
        for name in ("traj", "status", "bits", "steps", "q_end", "v_end", "progress_end"):
            assert torch.equal(torch.nan_to_num(out[name].float()), torch.nan_to_num(ref[name].float())), name
        return
    B = q.size(0)
    lim = torch.from_numpy(ft.limits_float32_inward(ft.JOINT_LIMITS_REAL)).to(dev())
    sc, sr, sl = robot._ik_sphere_table(dev(), False) if form == "spheres" else (None, None, None)
    path, arc = torch.empty((B, 1025, 7), device=dev()), torch.empty((B, 1025), device=dev())
    traj = torch.empty((B, T, 7), device=dev())
    status, bits, steps = (torch.empty(B, dtype=torch.int32, device=dev()) for _ in range(3))
    _lib.call("mpx_franka_follow", _lib.ptr(q), _lib.ptr(g), B, 8, T, ft.FINGER_OPENING, _lib.ptr(lim), _lib.ptr(sc), _lib.ptr(sr),
              _lib.ptr(sl), int(sc.size(0)) if form == "spheres" else 0, None, None, 0, None, None, None, 0, None, None, None,
              _lib.ptr(path), _lib.ptr(arc), _lib.ptr(status), _lib.ptr(bits), _lib.ptr(steps), _lib.ptr(traj), None, None,
              None, None)  # (NULL options: the defaults; every optional output NULL)
    assert torch.equal(status, ref["status"]) and torch.equal(bits, ref["bits"]) and torch.equal(steps, ref["steps"])
    assert torch.equal(torch.nan_to_num(traj), torch.nan_to_num(ref["traj"])) and int((status == 0).sum()) > 0


def test_closing_the_loop():
    """``make_problem_batch(64, collision_free=True, expert=True, hybrid=True)``: every key of the ``hybrid=False`` batch is
    bit-equal, the ``hybrid_valid`` rows pass the older judges, ``hybrid_target_pose`` is the FK of the last waypoint, and
    ``problems_to_dataset(..., "hybrid_solutions")`` loads through ``PointCloudTrajectoryDataset``.  The share
    hybrid_valid / expert_valid is printed and recorded in profiles/follow_timing.md, not asserted."""
    from mpinets_amd import scenes
    from mpinets_amd.data import DatasetType, PointCloudTrajectoryDataset
    from mpinets_amd.robot import franka_fk, frames_to_matrix

    torch.cuda.set_device(0)
    kw = dict(seed=3, collision_free=True, expert=True, device_clouds=True)
    plain, prob = scenes.make_problem_batch(64, **kw), scenes.make_problem_batch(64, hybrid=True, **kw)
    assert set(prob) - set(plain) == {"hybrid_solutions", "hybrid_valid", "hybrid_target_pose"}
    for k, v in plain.items():
        if torch.is_tensor(v):
            assert torch.equal(torch.nan_to_num(v.float()), torch.nan_to_num(prob[k].float())) and \
                torch.equal(torch.isnan(v.float()), torch.isnan(prob[k].float())), k
        else:
            assert v == prob[k], k
    hv, ev = prob["hybrid_valid"], prob["expert_valid"]
    print(f"closing the loop, 64 tabletop problems: expert_valid {int(ev.sum())}, hybrid_valid {int(hv.sum())}, share "
          f"{int(hv.sum()) / max(int(ev.sum()), 1):.4f}")
    assert bool((hv <= ev).all()) and int(hv.sum()) > 0
    assert prob["hybrid_solutions"].shape == (64, 50, 7) and prob["hybrid_target_pose"].shape == (64, 4, 4)
    assert bool(torch.isnan(prob["hybrid_solutions"][~hv]).all())
    rows = torch.nonzero(hv)[:, 0]
    traj = prob["hybrid_solutions"][rows]
    cub, cyl = prims_of({k: prob[k][rows] for k in ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers",
                                                    "cylinder_radii", "cylinder_heights", "cylinder_quats")})
    gripper = ft.LINK_ID["right_gripper"]
    goal = frames_to_matrix(franka_fk(prob["global_solutions"][rows, -1].contiguous())[:, gripper])
    for name, passed in zip(("env", "self", "jerk", "miss"), judged_valid(traj, goal, cub, cyl)):
        assert bool(passed.all()), name
    assert torch.equal(traj[:, 0], prob["q"][rows])
    assert torch.equal(prob["hybrid_target_pose"][rows], frames_to_matrix(franka_fk(traj[:, -1].contiguous())[:, gripper]))
    arrays = scenes.problems_to_dataset(prob, "hybrid_solutions")
    assert arrays["hybrid_solutions"].shape == (int(hv.sum()), 50, 7) == arrays["global_solutions"].shape
    assert np.array_equal(arrays["hybrid_solutions"], traj.cpu().numpy())
    ds = PointCloudTrajectoryDataset(arrays, "hybrid_solutions", 2048, 4096, 128, DatasetType.VAL, device=dev())
    assert len(ds) == int(hv.sum())
    item = ds.get_batch([0])
    assert item["xyz"].shape[1:] == (2048 + 4096 + 128, 4)
    plain_arrays = scenes.problems_to_dataset(prob)
    assert "hybrid_solutions" not in plain_arrays and plain_arrays["global_solutions"].shape[0] == int(ev.sum())
