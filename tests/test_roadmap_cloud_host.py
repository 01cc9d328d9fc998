"""CPU: the float64 restatement of ``mpx_franka_roadmap_cloud`` (tests/float64_roadmap_cloud.py) on the forced detour drawn as
a cloud, in float64 and in float32 -- the recorded statuses, the band of the GPU edge-state test and the cap of its left-out
problems are derived here --, the seeded cloud planner's restatement solving more of those problems than the plain one,
what the Python wrappers hand to C, and the refusals both new entries make on the host, before any launch."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_field as fcf  # noqa: E402
import float64_cloud_plan as fcp  # noqa: E402
import float64_plan as fp  # noqa: E402
import float64_roadmap as fr  # noqa: E402
import float64_roadmap_cloud as frc  # noqa: E402
import solver_call_grid as grid_calls  # noqa: E402

from mpinets_amd import _lib, capture, robot, scenes  # noqa: E402

DETOUR_ROWS = 96
DETOUR_PLAN_SEED = 9  # the Philox seed of tests/test_gpu_cloud_plan.py's forced detour (the roadmap's draws use it too)
POINT_RADIUS = fcp.WALL_POINT_RADIUS
LEFT_OUT_CAP = 0.10  # tests/test_roadmap_host.py's value: share of the problems that may have a tested configuration in the band

# recorded by test_restatement_on_the_detour_cloud (float64; the float32 run gives the same)
DETOUR_STATUS = [44, 3, 49]  # status 0 / 1 / 2 over the 96 rows
DETOUR_HOPS = [0, 0, 41, 3]  # histogram over the rows with a path: the cube sits on the line, no one-edge path
DETOUR_ROUNDS_MAX, DETOUR_ROUNDS_USED_UP = 64, 3
DETOUR_DISAGREEMENTS = 0  # rows on which the float32 run's status, path or edge_state differs from the float64 run's
# recorded by test_band_of_the_edge_state_comparison: the largest |d_float32 - d_float64| over the unsaturated sphere samples
# of the 96 x 64 nodes [m].  Radii and distances are below 0.2 m, where a float32 ulp is 1.5e-8: the interpolation's eight
# corner values, three fractions and seven lerps and the FK chain in front of them account for the rest.
BAND_DIFFERENCE = 2.2e-7
BAND = 2 * BAND_DIFFERENCE  # twice: the edge configurations are not in that sample
# recorded by test_seeded_restatement_solves_more (the first 24 rows, float64, default options)
DETOUR_PLANNED, DETOUR_PLAIN_SOLVED, DETOUR_SEEDED_SOLVED = 13, 7, 11  # (tests/test_cloud_plan_host.py records 13 and 7)


def detour_field(B=DETOUR_ROWS):
    """The forced detour as a cloud and its field on the default grid, as ``robot.franka_roadmap_cloud`` builds it."""
    qs, qg, lim, cloud, _ = fcp.detour_problems(B)
    grid = fcp.default_grid(fcp.truncation(POINT_RADIUS))
    return qs, qg, lim, cloud, grid, fcf.build_fast(cloud, None, grid)


@pytest.fixture(scope="module")
def detour():
    qs, qg, lim, cloud, grid, field = detour_field()
    runs = {dt: frc.solve(qs, qg, field, grid, POINT_RADIUS, limits=lim, seed=DETOUR_PLAN_SEED, dtype=dt)
            for dt in (np.float64, np.float32)}
    return qs, qg, lim, cloud, grid, field, runs


def test_restatement_on_the_detour_cloud(detour):
    qs, qg, lim, cloud, grid, field, runs = detour
    for dt, (traj, st, path, hops, nodes, state, rounds) in runs.items():
        print(f"detour cloud, {np.dtype(dt).name} restatement: status 0 / 1 / 2 {np.bincount(st, minlength=3).tolist()}, hops "
              f"histogram {np.bincount(hops[st == 0]).tolist()}, rounds histogram {np.bincount(rounds).tolist()}")
        assert np.bincount(st, minlength=3).tolist() == DETOUR_STATUS
        assert np.bincount(hops[st == 0]).tolist() == DETOUR_HOPS
        assert rounds.max() == DETOUR_ROUNDS_MAX and int((rounds[st == 1] == DETOUR_ROUNDS_MAX).sum()) == DETOUR_ROUNDS_USED_UP
        assert (rounds[st == 2] == 0).all() and np.isnan(traj[st != 0]).all() and (path[st != 0] == -1).all()
        found = st == 0
        assert np.array_equal(traj[found][:, 0], qs[found].astype(dt)) and np.array_equal(traj[found][:, -1], qg[found].astype(dt))
        assert all(np.array_equal(s, s.T) for s in state)
    a, b = runs[np.float64], runs[np.float32]
    differ = [r for r in range(DETOUR_ROWS)
              if a[1][r] != b[1][r] or not np.array_equal(a[2][r], b[2][r]) or not np.array_equal(a[5][r], b[5][r])]
    print(f"float32 against float64: {len(differ)} rows differ {differ}")
    assert len(differ) == DETOUR_DISAGREEMENTS
    assert np.array_equal(a[4], fr.draw_nodes(qs, qg, lim, 64, DETOUR_PLAN_SEED))  # the primitive roadmap's nodes


def test_band_of_the_edge_state_comparison(detour):
    """The band is measured, not fixed in advance: twice the largest |d_float32 - d_float64| over the unsaturated sphere
    samples of the 96 x 64 nodes.  The measurement is repeated and must land within a factor 2 of the recorded figure; with
    the band the share of problems left out of a float32-against-float64 comparison stays below the cap, and everywhere else
    the float32 run's graph carries the float64 verdicts."""
    qs, qg, lim, cloud, grid, field, runs = detour
    nodes = runs[np.float64][4]
    worst, samples = 0.0, 0
    for b in range(DETOUR_ROWS):
        q = torch.from_numpy(np.nan_to_num(nodes[b]))
        d64, l64 = frc.margins(q.double(), field[b], grid, POINT_RADIUS, want_samples=True)[2:]
        d32, l32 = frc.margins(q.float(), field[b], grid, POINT_RADIUS, want_samples=True)[2:]
        both = l64 & l32
        samples += int(both.sum())
        if both.any():
            worst = max(worst, float(np.abs(d64 - d32)[both].max()))
    print(f"|d_float32 - d_float64| over {samples} unsaturated sphere samples: max {worst:.3e} m; band {2 * worst:.3e} m")
    assert samples > 1000 and BAND_DIFFERENCE / 2 <= worst <= BAND_DIFFERENCE * 2
    left = {dt: 0 for dt in runs}
    wrong = 0
    for b in range(DETOUR_ROWS):
        for dt, run in runs.items():
            want, in_band = frc.graph_verdicts(run[4][b], run[5][b], field[b], grid, BAND, point_radius=POINT_RADIUS)
            left[dt] += in_band
            tested = want != 0
            wrong += (not in_band) and not np.array_equal(want[tested], run[5][b][tested])
    print(f"left out of {DETOUR_ROWS}: " + ", ".join(f"{np.dtype(dt).name} graph {n}" for dt, n in left.items())
          + f"; {wrong} graphs disagree outside the band")
    assert max(left.values()) / DETOUR_ROWS <= LEFT_OUT_CAP and wrong == 0


def test_seeded_restatement_solves_more(detour):
    """The roadmap's trajectory as a ninth starting trajectory of the cloud planner's restatement, on the first 24 rows: the
    seed is valid by the exact swept-sphere test on every row where the roadmap found a path, the solved count rises from 7
    to 11 of 13 planned, and the rows the plain restatement solves keep their choice."""
    qs, qg, lim, cloud, grid, field, runs = detour
    n, K = fcp.DETOUR_B, fp.DEFAULTS["candidates"]
    road = runs[np.float64]
    traj, st, choice, all_traj, bits = frc.solve_seeded(qs[:n], qg[:n], road[0][:n, None], cloud[:n], None, field[:n], grid,
                                                        POINT_RADIUS, limits=lim, seed=DETOUR_PLAN_SEED)
    planned = st != 2
    plain_ok = (bits[:, :K] == 0).any(1) & planned
    found = (road[1][:n] == 0) & planned
    print(f"forced detour as a cloud, float64 restatement: planned {int(planned.sum())}, plain solves {int(plain_ok.sum())}, "
          f"with the roadmap seed {int((st == 0).sum())}; the roadmap finds a path on {int(found.sum())} planned rows, seed bits "
          f"histogram {np.bincount(bits[found, K], minlength=8).tolist()}")
    assert (int(planned.sum()), int(plain_ok.sum()), int((st == 0).sum())) == (DETOUR_PLANNED, DETOUR_PLAIN_SOLVED, DETOUR_SEEDED_SOLVED)
    assert int((st == 0).sum()) > int(plain_ok.sum())
    first = np.where((bits[:, :K] == 0).any(1), (bits[:, :K] == 0).argmax(1), -1)
    assert bool((st[plain_ok] == 0).all()) and np.array_equal(choice[plain_ok], first[plain_ok])
    assert (bits[planned & ~found, K] == 7).all() and np.isnan(all_traj[planned & ~found, K]).all()
    won = (st == 0) & ~plain_ok
    assert (choice[won] == K).all()
    assert np.array_equal(traj[won][:, 0], qs[:n][won].astype(np.float64)) and np.array_equal(traj[won][:, -1], qg[:n][won].astype(np.float64))


# ---- what the wrappers hand to C -----------------------------------------------------------------------------------------------
T, N = grid_calls.T, grid_calls.N


def _problem(B=3):
    return torch.zeros(B, 7), torch.ones(B, 7) * 0.1, torch.zeros(B, 9, 4)[:, 2:2 + N, :3], torch.full((B,), 4, dtype=torch.int32)


def _plan_cloud_positions(name):
    """Positions of (B, T, field, options, seeds, Ks, scratch_bytes) in an entry's argument list (Ks: None for the plain one)."""
    seeded = name.endswith("_seeded")
    return dict(B=2, T=3, field=10, options=18, seeds=21 if seeded else None, Ks=22 if seeded else None, bytes=-1)


def test_plan_cloud_wrapper_without_and_with_seeds():
    q0, q1, cloud, counts = _problem()
    B, lib = q0.size(0), _lib.load()
    with grid_calls.recording() as plain:
        out = robot.franka_plan_cloud(q0, q1, cloud, counts, point_radius=0.01, T=T, seed=7, env_offset=3, return_all=True)
    assert [c[0] for c in plain] == ["mpx_cloud_field_build", "mpx_franka_plan_cloud"]
    name, args = plain[1]
    assert len(args) == len(_lib.PROTOTYPES[name]) - 1 == 28  # (the stream is appended by _lib.call)
    K, sub = robot.PLAN_DEFAULTS["candidates"], robot.PLAN_DEFAULTS["substeps"]
    assert args[2] == B and args[3] == T and args[-1] == lib.mpx_franka_plan_cloud_scratch(B, T, K, sub)
    assert tuple(out[3].shape) == (B, K, T, 7)

    seeds = torch.zeros(B, 2, T, 7)
    with grid_calls.recording() as calls:
        out = robot.franka_plan_cloud(q0, q1, cloud, counts, point_radius=0.01, T=T, seed=7, env_offset=3, return_all=True,
                                      seeds=seeds)
    name, sargs = calls[1]
    assert name == "mpx_franka_plan_cloud_seeded" and len(sargs) == len(_lib.PROTOTYPES[name]) - 1 == 30
    at = _plan_cloud_positions(name)
    assert sargs[at["seeds"]] == seeds.data_ptr() and sargs[at["Ks"]] == 2
    assert sargs[-1] == lib.mpx_franka_plan_cloud_scratch(B, T, K + 2, sub)  # scratch sized for K + Ks
    assert tuple(out[3].shape) == (B, K + 2, T, 7) and tuple(out[4].shape) == (B, K + 2)
    # everything in front of the seeds is the plain call's (the field and the outputs are fresh tensors)
    given = dict(q_start=q0, q_goal=q1, cloud=cloud, counts=counts)
    a, s = grid_calls.describe("mpx_franka_plan_cloud", args, given)["args"], grid_calls.describe(name, sargs, given)["args"]
    assert a[:21] == s[:21] and a[21:26] == s[23:28] == ["other"] * 5  # (21 .. 25 of the plain call: its five outputs)
    # no seeds at all: the seeded entry with Ks = 0 and no pointer (it launches the plain kernel)
    with grid_calls.recording() as calls:
        robot.franka_plan_cloud(q0, q1, cloud, counts, T=T, seeds=torch.zeros(B, 0, T, 7))
    assert calls[1][0] == "mpx_franka_plan_cloud_seeded" and calls[1][1][21] is None and calls[1][1][22] == 0

    # slabs: the seed pointer moves with the rows
    per = int(lib.mpx_franka_plan_cloud_scratch(1, T, K + 2, sub))
    from mpinets_amd import solvers

    saved, Bs = solvers.PLAN_CLOUD_SCRATCH_BYTES, 5
    solvers.PLAN_CLOUD_SCRATCH_BYTES = 2 * per
    try:
        q0, q1, cloud, counts = _problem(Bs)
        seeds = torch.zeros(Bs, 2, T, 7)
        with grid_calls.recording() as calls:
            robot.franka_plan_cloud(q0, q1, cloud, counts, T=T, env_offset=3, seeds=seeds)
    finally:
        solvers.PLAN_CLOUD_SCRATCH_BYTES = saved
    slabs = [a for n, a in calls if n == "mpx_franka_plan_cloud_seeded"]
    assert [a[2] for a in slabs] == [2, 2, 1] and [a[20] for a in slabs] == [3, 5, 7]  # rows, env_offset
    assert [a[21] - seeds.data_ptr() for a in slabs] == [4 * b0 * 2 * T * 7 for b0 in (0, 2, 4)]
    assert [a[0] - q0.data_ptr() for a in slabs] == [4 * b0 * 7 for b0 in (0, 2, 4)]


def test_global_cloud_wrapper_builds_one_field_for_both_stages():
    q0, q1, cloud, counts = _problem()
    B = q0.size(0)
    with grid_calls.recording() as calls:
        out = robot.franka_plan_global_cloud(q0, q1, cloud, counts, point_radius=0.01, T=T, seed=7, env_offset=3,
                                             roadmap=dict(nodes=8), clearance=0.01, check_self=False)
    assert [c[0] for c in calls] == ["mpx_cloud_field_build", "mpx_franka_roadmap_cloud", "mpx_franka_plan_cloud_seeded"]
    build, road, plan = (c[1] for c in calls)
    assert len(road) == len(_lib.PROTOTYPES["mpx_franka_roadmap_cloud"]) - 1
    assert road[10] == plan[10] == build[7] and road[10]  # one field, the one that was built
    assert road[12] == pytest.approx(0.01) and road[13] == 0.0  # point_radius, field_slack
    ropt, popt = road[14]._obj, plan[18]._obj
    assert ropt.nodes == 8 and ropt.clearance == popt.clearance == pytest.approx(0.01) and ropt.check_self == popt.check_self == 0
    assert ropt.check_margin == popt.check_margin
    assert road[15] == plan[19] == 7 and road[16] == plan[20] == 3  # seed, env_offset
    assert plan[22] == 1 and plan[21] == road[17]  # the roadmap's traj is the one seed
    assert len(out) == 3 and out[2].data_ptr() == road[18]  # ... and its status comes back last
    # a field of the caller's is built by nobody
    with grid_calls.recording():
        field = grid_calls.CloudField.build(cloud)
    with grid_calls.recording() as calls:
        robot.franka_plan_global_cloud(q0, q1, cloud, counts, field=field, T=T)
    assert [c[0] for c in calls] == ["mpx_franka_roadmap_cloud", "mpx_franka_plan_cloud_seeded"]
    assert calls[0][1][10] == calls[1][1][10] == field.values.data_ptr()
    # the roadmap alone: no cloud and no field is no environment
    with grid_calls.recording() as calls:
        res = robot.franka_roadmap_cloud(q0, q1, None, T=T, return_graph=True, field_slack=0.026)
    assert [c[0] for c in calls] == ["mpx_franka_roadmap_cloud"] and calls[0][1][10] is None and calls[0][1][11] is None
    assert calls[0][1][13] == pytest.approx(0.026) and len(res) == 7 and tuple(res[5].shape) == (B, 64, 64)
    assert inspect.signature(robot.franka_roadmap_cloud).parameters["field_slack"].default == 0.0
    assert inspect.signature(robot.franka_plan_cloud).parameters["seeds"].default is None
    with grid_calls.recording(), pytest.raises(TypeError):
        robot.franka_roadmap_cloud(q0, q1, cloud, T=T, node=3)
    with pytest.raises(_lib.MpxError):  # (no CPU fallback)
        robot.franka_roadmap_cloud(q0, q1, cloud, T=T)


def test_plan_to_poses_and_the_expert_keep_their_default_calls():
    q0, q1, cloud, counts = _problem()
    poses = torch.eye(4).repeat(q0.size(0), 1, 1)
    with grid_calls.recording() as calls:
        res = capture.plan_to_poses(cloud, q0, poses, counts=counts, T=T)
    assert [c[0] for c in calls] == ["mpx_franka_ik_cloud", "mpx_cloud_field_build", "mpx_franka_plan_cloud"]
    assert sorted(res) == ["ik_status", "plan_status", "q_goal", "trajectory", "valid"]
    with grid_calls.recording() as calls:
        res = capture.plan_to_poses(cloud, q0, poses, counts=counts, T=T, global_plan=True, roadmap_options=dict(nodes=16))
    assert [c[0] for c in calls] == ["mpx_franka_ik_cloud", "mpx_cloud_field_build", "mpx_franka_roadmap_cloud",
                                     "mpx_franka_plan_cloud_seeded"]
    assert sorted(res) == ["ik_status", "plan_status", "q_goal", "roadmap_status", "trajectory", "valid"]
    assert calls[2][1][14]._obj.nodes == 16
    assert inspect.signature(capture.plan_to_poses).parameters["global_plan"].default is False

    valid = torch.ones(q0.size(0), dtype=torch.bool)
    big = torch.zeros(q0.size(0), N, 3)
    with grid_calls.recording() as calls:
        scenes._expert_trajectories_cloud(big, q0, q1, valid, 5, 2, 0.02)
    assert [c[0] for c in calls] == ["mpx_cloud_field_build", "mpx_franka_plan_cloud"]
    assert calls[1][1][3] == scenes.EXPERT_LENGTH and calls[1][1][19] == 5 and calls[1][1][20] == 2
    with grid_calls.recording() as calls:
        out = scenes._expert_trajectories_cloud(big, q0, q1, valid, 5, 2, 0.02, roadmap=True)
    assert [c[0] for c in calls] == ["mpx_cloud_field_build", "mpx_franka_roadmap_cloud", "mpx_franka_plan_cloud_seeded"]
    assert sorted(out) == ["expert_valid", "global_solutions"]
    for bad in ("cloud", "cloud_roadmap"):
        with pytest.raises(ValueError, match="hybrid"):
            scenes.make_problem_batch(2, collision_free=True, expert=True, expert_from=bad, hybrid=True)
    with pytest.raises(ValueError, match="cloud_roadmap"):
        scenes.make_problem_batch(2, collision_free=True, expert=True, expert_from="roadmap_cloud")


# ---- refusals ------------------------------------------------------------------------------------------------------------------
GOOD = dict(nodes=64, resolution=0.05, connect_radius=float("inf"), max_rounds=8, smooth_passes=4, check_margin=1e-4,
            clearance=0.0, check_self=1)
PLAN_GOOD = dict(candidates=8, iterations=10, step=1e-3, smooth_weight=1.0, epsilon=0.05, spread=0.5, substeps=4,
                 check_margin=1e-4, clearance=0.0, max_jerk=0.15, check_self=1)


def _grid(trunc=0.2, n=(8, 8, 8), h=0.05):
    return _lib.FieldGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), h, n[0], n[1], n[2], trunc)


def _p(v):  # any non-NULL "device pointer": refused before it is touched
    return ctypes.c_void_p(v) if v else None


def _roadmap_cloud(lib, B=4, T=50, S=56, field=256, grid="good", point_radius=0.02, field_slack=0.0, opts=None, env_offset=0,
                   traj=256, status=256, path=256, hops=256, qs=256, lim=256, table=256):
    g = _grid() if grid == "good" else grid
    return lib.mpx_franka_roadmap_cloud(_p(qs), _p(256), B, T, 0.025, _p(lim), _p(table), _p(table), _p(table), S, _p(field),
                                        None if g is None else ctypes.byref(g), point_radius, field_slack,
                                        None if opts is None else ctypes.byref(opts), 0, env_offset, _p(traj), _p(status),
                                        _p(path), _p(hops), None, None, None, None)


def test_roadmap_cloud_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    opt = lambda **kw: _lib.RoadmapOptions(**dict(GOOD, **kw))  # noqa: E731
    err = lib.mpx_last_error
    # what mpx_franka_roadmap refuses
    for bad in (1, 65):
        assert _roadmap_cloud(lib, T=bad) != 0 and b"waypoints" in err()
    assert _roadmap_cloud(lib, B=-1) != 0 and b"negative size" in err()
    assert _roadmap_cloud(lib, S=65) != 0 and b"65" in err()
    for bad in (-1, 1 << 32):
        assert _roadmap_cloud(lib, env_offset=bad) != 0 and b"env_offset" in err()
    for V in (-1, 0, 1, 257):
        assert _roadmap_cloud(lib, opts=opt(nodes=V)) != 0 and b"nodes" in err()
    for res in (0.0, -0.05, float("nan")):
        assert _roadmap_cloud(lib, opts=opt(resolution=res)) != 0 and b"resolution" in err()
    assert _roadmap_cloud(lib, opts=opt(connect_radius=float("nan"))) != 0 and b"connect_radius" in err()
    assert _roadmap_cloud(lib, opts=opt(max_rounds=0)) != 0 and b"max_rounds" in err()
    assert _roadmap_cloud(lib, opts=opt(smooth_passes=-1)) != 0 and b"smooth_passes" in err()
    assert _roadmap_cloud(lib, opts=opt(check_margin=-1e-4)) != 0 and b"check_margin" in err()
    assert _roadmap_cloud(lib, opts=opt(clearance=float("nan"))) != 0 and b"clearance" in err()
    for out in ("traj", "status", "path", "hops"):
        assert _roadmap_cloud(lib, **{out: 0}) != 0 and b"NULL output" in err()
    assert _roadmap_cloud(lib, qs=0) != 0 and b"NULL operand" in err()
    assert _roadmap_cloud(lib, lim=0) != 0 and b"NULL operand" in err()
    assert _roadmap_cloud(lib, table=0) != 0 and b"sphere table" in err()
    # what the grid check refuses
    assert _roadmap_cloud(lib, grid=None) != 0 and b"NULL grid" in err()
    assert _roadmap_cloud(lib, grid=_grid(n=(1, 8, 8))) != 0 and b"nodes" in err()
    assert _roadmap_cloud(lib, grid=_grid(h=0.0)) != 0 and b"spacing" in err()
    assert _roadmap_cloud(lib, grid=_grid(trunc=float("inf"))) != 0 and b"trunc" in err()
    # its own
    for bad in (-0.01, float("nan"), float("inf")):
        assert _roadmap_cloud(lib, field_slack=bad) != 0 and b"field_slack" in err()
        assert _roadmap_cloud(lib, point_radius=bad) != 0 and b"point_radius" in err()
    assert _roadmap_cloud(lib, S=0, table=0) != 0 and b"without collision spheres" in err()
    # trunc must exceed 0.08 + point_radius + max(clearance, 0) + check_margin + field_slack: 0.1001 here ...
    assert _roadmap_cloud(lib, grid=_grid(trunc=0.1)) != 0 and b"trunc" in err()
    assert _roadmap_cloud(lib, B=0, grid=_grid(trunc=0.1002)) == 0
    # ... 0.1261 with a slack of 0.866 x 3 cm, 0.1501 with a clearance of 5 cm (a negative clearance gives no room back)
    assert _roadmap_cloud(lib, B=0, grid=_grid(trunc=0.126), field_slack=0.026) != 0 and b"trunc" in err()
    assert _roadmap_cloud(lib, B=0, grid=_grid(trunc=0.1262), field_slack=0.026) == 0
    assert _roadmap_cloud(lib, B=0, grid=_grid(trunc=0.15), opts=opt(clearance=0.05)) != 0 and b"trunc" in err()
    assert _roadmap_cloud(lib, B=0, grid=_grid(trunc=0.1), opts=opt(clearance=-0.05)) != 0 and b"trunc" in err()
    assert frc.refused(fcf.make_grid((8, 8, 8), trunc=0.1), 0.02, 0.0) and not frc.refused(fcf.make_grid((8, 8, 8), trunc=0.1002), 0.02, 0.0)
    assert not frc.refused(fcp.default_grid(fcp.truncation(POINT_RADIUS)), POINT_RADIUS, 0.866 * fcp.VOXEL)
    # nothing to do, nothing touched: without a field no grid is read; a bad option is refused even then
    assert _roadmap_cloud(lib, B=0, traj=0, status=0, path=0, hops=0, qs=0, lim=0, table=0) == 0
    assert _roadmap_cloud(lib, B=0, field=0, grid=None, S=0, table=0) == 0
    assert _roadmap_cloud(lib, B=0, opts=opt(nodes=1)) != 0 and _roadmap_cloud(lib, B=0, field_slack=-1.0) != 0


def _seeded(lib, B=4, T=50, opts=None, seeds=256, Ks=1, K_scratch=None, traj=256, status=256, env_offset=0, scratch=256):
    o = opts if opts is not None else _lib.PlanOptions(**PLAN_GOOD)
    need = lib.mpx_franka_plan_cloud_scratch(max(B, 0), T, o.candidates + Ks if K_scratch is None else K_scratch, o.substeps)
    return lib.mpx_franka_plan_cloud_seeded(_p(256), _p(256), B, T, 0.025, _p(256), None, None, None, 0, None, None, None, 0, 3, 0,
                                            None, 0.0, ctypes.byref(o), 0, env_offset, _p(seeds), Ks, _p(traj), _p(status), None,
                                            None, None, _p(scratch), max(need, 0), None)


def test_seeded_cloud_planner_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    err = lib.mpx_last_error
    assert _seeded(lib, Ks=2, seeds=0) != 0 and b"Ks > 0 without seeds" in err()
    assert _seeded(lib, Ks=9) != 0 and b"candidates + seeds" in err()  # 8 + 9 = 17
    assert _seeded(lib, Ks=1, opts=_lib.PlanOptions(**dict(PLAN_GOOD, candidates=16))) != 0 and b"candidates + seeds" in err()
    assert _seeded(lib, Ks=-1) != 0 and b"negative size" in err()
    assert _seeded(lib, Ks=2, K_scratch=8) != 0 and b"scratch" in err()  # sized for the drawn candidates alone
    # mpx_franka_plan_cloud's own refusals, under this entry's name
    assert _seeded(lib, T=65) != 0 and b"mpx_franka_plan_cloud_seeded" in err()
    assert _seeded(lib, traj=0) != 0 and b"NULL output" in err()
    assert _seeded(lib, scratch=8) != 0 and b"aligned" in err()
    assert _seeded(lib, opts=_lib.PlanOptions(**dict(PLAN_GOOD, step=0.0))) != 0 and b"step" in err()
    assert _seeded(lib, env_offset=-1) != 0 and b"env_offset" in err()
    assert _seeded(lib, B=0, traj=0, status=0, seeds=0, Ks=3) == 0


def test_new_kernels_use_no_scratch():
    """The roadmap kernel and the seeded planner's <= 8-wave form keep everything in registers and LDS."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    meta = kernel_metadata(LIB)
    for key in ("franka_roadmap_cloud_kernel", "franka_plan_cloud_seeded_kernelILi8E"):
        hits = {n: f for n, f in meta.items() if key in n}
        assert len(hits) == 1, key
        (f,) = hits.values()
        print(key, {k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0
