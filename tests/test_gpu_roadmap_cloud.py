"""GPU: ``mpx_franka_roadmap_cloud`` (csrc/roadmap_cloud.hip), ``mpx_franka_plan_cloud_seeded`` (csrc/cloud_field.hip) and
``robot.franka_plan_global_cloud`` against the float64 restatement (tests/float64_roadmap_cloud.py), against the judge that
predates the planner (``FrankaCollisionSampler.check_cloud``) and at their edges.  One module-scoped fixture per scenario: a
launch runs once.  The field the verdicts are recomputed from is the one the DEVICE built, copied to the host, so these tests
judge the roadmap kernel and not the field build (tests/test_gpu_cloud_field.py holds that)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_plan as fcp  # noqa: E402
import float64_plan as fp  # noqa: E402
import float64_roadmap as fr  # noqa: E402
import float64_roadmap_cloud as frc  # noqa: E402
from test_cloud_plan_host import RECORDED_DISAGREEMENTS  # noqa: E402
from test_gpu_cloud_plan import SUBSTEPS, build_field, dev, grid_dict, same, up  # noqa: E402
from test_gpu_roadmap import _check_search  # noqa: E402
from test_roadmap_cloud_host import BAND, DETOUR_PLAN_SEED, DETOUR_ROWS, DETOUR_SEEDED_SOLVED, LEFT_OUT_CAP, POINT_RADIUS  # noqa: E402
from test_roadmap_host import SEED_REFERENCE  # noqa: E402

pytestmark = pytest.mark.gpu

V, T, K = 64, 50, 8
PLAN_ROWS = fcp.DETOUR_B  # the 24 rows the planners run on


def host(out):
    return tuple(x.cpu().numpy() for x in out)


def sliced(field, rows):
    from mpinets_amd.field import CloudField

    return CloudField(field.values[rows].contiguous(), field.grid)


@pytest.fixture(scope="module")
def detour():
    """The forced detour drawn as a cloud (96 rows, one 10 cm cube lattice of 152 points each), its field as the device
    builds it, and the roadmap with its graph at the planner's seed."""
    from mpinets_amd import robot

    torch.cuda.set_device(0)
    qs, qg, lim, cloud, _ = fcp.detour_problems(DETOUR_ROWS)
    a, b, c = up(qs), up(qg), up(cloud)
    field = build_field(c, POINT_RADIUS)
    kw = dict(field=field, point_radius=POINT_RADIUS, seed=DETOUR_PLAN_SEED, limits=lim)
    road = robot.franka_roadmap_cloud(a, b, c, return_graph=True, **kw)
    return dict(qs=qs, qg=qg, lim=lim, a=a, b=b, c=c, field=field, values=field.values.cpu().numpy(), grid=grid_dict(field.grid),
                kw=kw, road=road, host=host(road))


def test_nodes_are_the_primitive_roadmaps(detour):
    """``nodes`` is bit-equal to the restatement's draw (stream 16, keyed by seed, global problem id and node) and to
    ``franka_roadmap``'s nodes at the same seed."""
    from mpinets_amd import robot

    nodes = detour["road"][4]
    assert np.array_equal(nodes.cpu().numpy(), fr.draw_nodes(detour["qs"], detour["qg"], detour["lim"], V, seed=DETOUR_PLAN_SEED))
    prim = robot.franka_roadmap(detour["a"], detour["b"], seed=DETOUR_PLAN_SEED, limits=detour["lim"], return_graph=True)
    assert same(nodes, prim[4])
    assert torch.equal(nodes[:, 0], detour["a"]) and torch.equal(nodes[:, 1], detour["b"])


def test_edge_state_against_float64(detour):
    """The diagonal and every tested edge of ``edge_state`` carry the float64 verdict, recomputed from the device's own
    float32 nodes, the stated pieces and the device's own field; a problem is left out when a configuration that decides one
    of its verdicts has a sphere (or a self distance) within BAND of its threshold (tests/test_roadmap_cloud_host.py: 4.4e-7
    m).  The count left out is printed and capped at LEFT_OUT_CAP of the problems.  Untested entries are 0, the matrix is
    symmetric, status-2 rows hold their diagonal only."""
    traj, st, path, hops, nd, es, rounds = detour["host"]
    assert np.array_equal(es, es.transpose(0, 2, 1)) and es.max() <= 2
    off = es * (1 - np.eye(V, dtype=np.uint8))
    assert (off[st == 2] == 0).all() and (rounds[st == 2] == 0).all()
    left, wrong, tested = 0, [], 0
    for b in range(DETOUR_ROWS):
        want, in_band = frc.graph_verdicts(nd[b], es[b], detour["values"][b], detour["grid"], BAND, point_radius=POINT_RADIUS)
        left += in_band
        known = want != 0
        tested += int(np.triu(known, 1).sum())
        assert (es[b][~known] == 0).all()
        if not in_band and not np.array_equal(want[known], es[b][known]):
            wrong.append(b)
    print(f"edge_state against float64: {DETOUR_ROWS} problems, {tested} tested edges, {left} problems left out "
          f"({left / DETOUR_ROWS:.4f}), disagreeing problems {wrong}")
    assert left / DETOUR_ROWS <= LEFT_OUT_CAP
    assert not wrong
    assert ((es[:, 0, 0] == 1) & (es[:, 1, 1] == 1))[st != 2].all() and ((es[:, 0, 0] == 2) | (es[:, 1, 1] == 2))[st == 2].all()


def test_search_invariant_on_the_devices_own_edge_state(detour):
    """Status 0: every edge of ``path`` is free and the float64 cost of ``path`` equals, within V 2^-23 relative, the cost of
    the shortest path over "valid nodes, edges not blocked" found by a heap on the device's ``edge_state``.  Status 1: node
    1 cannot be reached in that graph, or the rounds ran out (a second run with 3 rounds makes them run out)."""
    from mpinets_amd import robot

    traj, st, path, hops, nd, es, rounds = detour["host"]
    _check_search(nd, es, st, path, hops, rounds, fr.DEFAULTS["max_rounds"])
    print(f"cloud roadmap on the detour: status 0 / 1 / 2 = {np.bincount(st, minlength=3).tolist()}, hops histogram "
          f"{np.bincount(hops[st == 0]).tolist()}, rounds histogram {np.bincount(rounds).tolist()}")
    assert (st == 0).sum() >= 30 and (hops[st == 0] >= 2).all()  # (the cube sits on the line)
    short = host(robot.franka_roadmap_cloud(detour["a"], detour["b"], detour["c"], return_graph=True, max_rounds=3, **detour["kw"]))
    _check_search(short[4], short[5], short[1], short[2], short[3], short[6], 3)
    ran_out = (short[1] == 1) & (short[6] == 3)
    assert ran_out.sum() >= 4 and (st[ran_out] != 2).all()
    ends = (short[6] <= 2) & (short[1] == 0)  # a search that ends within the budget does not see the budget
    assert np.array_equal(short[2][ends], path[ends])


def test_seed_trajectory(detour):
    """``traj`` equals the float64 resample-and-smooth of the device's own ``path`` and ``nodes`` within the bar of
    tests/test_gpu_roadmap.py for the same arithmetic (4 x SEED_REFERENCE of tests/test_roadmap_host.py = 3.1e-6 rad);
    waypoints 0 and T-1 are bit-equal to the endpoints; rows with status != 0 are NaN."""
    tr, st, pa, hp, nd, _, _ = detour["host"]
    ok = st == 0
    worst = 0.0
    for b in np.flatnonzero(ok):
        want = fr.seed_trajectory(nd[b], pa[b, :hp[b] + 1].tolist(), T, fr.DEFAULTS["smooth_passes"])
        worst = max(worst, float(np.abs(tr[b].astype(np.float64) - want).max()))
    print(f"seed trajectory against float64 over {int(ok.sum())} paths: max {worst:.3e} (bar {4 * SEED_REFERENCE:.2e})")
    assert worst <= 4 * SEED_REFERENCE
    assert np.array_equal(tr[ok][:, 0], detour["qs"][ok]) and np.array_equal(tr[ok][:, -1], detour["qg"][ok])
    assert np.isnan(tr[~ok]).all() and not np.isnan(tr[ok]).any()
    lim32 = fp.limits32(detour["lim"])
    assert ((tr[ok] >= lim32[:, 0]) & (tr[ok] <= lim32[:, 1])).all()


def test_no_environment_gives_the_planners_line():
    """Without a field (no cloud, no field) and with a cloud of ``counts`` = 0 (a field saturated everywhere) only the limits
    and the self test can refuse anything: every planned row is the path 0 -> 1 in one round and ``traj`` is the planner's
    line bit for bit; both equal ``franka_roadmap`` without primitives, every output."""
    from mpinets_amd import robot, scenes

    torch.cuda.set_device(0)
    B = 64
    qs, qg = scenes.random_configurations(B, 31), scenes.random_configurations(B, 32)
    a, b = up(qs), up(qg)
    want = robot.franka_roadmap(a, b, return_graph=True, seed=3)
    cloud = up(np.random.default_rng(1).uniform(-0.5, 0.5, size=(B, 64, 3)).astype(np.float32))
    counts = torch.zeros(B, dtype=torch.int32, device=dev())
    for got in (robot.franka_roadmap_cloud(a, b, None, return_graph=True, seed=3),
                robot.franka_roadmap_cloud(a, b, cloud, counts, point_radius=0.01, return_graph=True, seed=3)):
        for name, g, w in zip(("traj", "status", "path", "hops", "nodes", "edge_state", "rounds"), got, want):
            assert same(g, w), name
        traj, st, path, hops, nodes, es, rounds = host(got)
        planned = st != 2  # (a uniform draw can itself be a self collision)
        assert planned.sum() >= 16 and (st[planned] == 0).all() and (hops[planned] == 1).all() and (rounds[planned] == 1).all()
        assert np.array_equal(traj[planned], fp.line(qs, qg, T)[planned])


def _restated(detour, rows, **options):
    return frc.solve(detour["qs"][rows], detour["qg"][rows], detour["values"][rows], detour["grid"], POINT_RADIUS,
                     limits=detour["lim"], seed=DETOUR_PLAN_SEED, env_offset=int(rows[0]), T=options.pop("T", T), **options)


@pytest.mark.parametrize("options", [dict(nodes=2), dict(nodes=3), dict(nodes=256), dict(T=2), dict(resolution=1e3),
                                     dict(max_rounds=1)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_edges_of_the_shape_space(detour, options):
    """Two problems (one for T = 2) at the edges of the options: the run finishes, its graph passes the search invariants and
    the statuses, hops and rounds are the float64 restatement's on the device's field.  ``resolution`` = 1000 rad makes
    every edge one piece (no interior configuration: every edge between valid nodes is free, one round)."""
    from mpinets_amd import robot

    found = np.flatnonzero(detour["host"][1] == 0)
    rows = found[:1] if "T" in options else found[:2]
    rows = np.arange(rows[0], rows[-1] + 1)  # (a contiguous range: env_offset keys the draws)
    idx = torch.as_tensor(rows, device=dev())
    o = dict(options)
    T_ = o.pop("T", T)
    kw = dict(detour["kw"], field=sliced(detour["field"], idx))
    got = host(robot.franka_roadmap_cloud(detour["a"][idx], detour["b"][idx], detour["c"][idx], T=T_, env_offset=int(rows[0]),
                                          return_graph=True, **kw, **o))
    traj, st, path, hops, nd, es, rounds = got
    want = _restated(detour, rows, T=T_, **o)
    print(f"{options}: rows {rows.tolist()}, status {st.tolist()}, hops {hops.tolist()}, rounds {rounds.tolist()}")
    assert np.array_equal(st, want[1]) and np.array_equal(hops, want[3]) and np.array_equal(rounds, want[6])
    assert np.array_equal(nd, want[4])
    _check_search(nd, es, st, path, hops, rounds, o.get("max_rounds", fr.DEFAULTS["max_rounds"]))
    ok = st == 0
    assert np.isnan(traj[~ok]).all() and traj.shape == (len(rows), T_, 7)
    assert np.array_equal(traj[ok][:, 0], detour["qs"][rows][ok]) and np.array_equal(traj[ok][:, -1], detour["qg"][rows][ok])
    if "resolution" in options:
        assert (st == 0).all() and (hops == 1).all() and (rounds == 1).all()
    if options.get("nodes") == 2 or "max_rounds" in options:
        assert (st == 1).all()  # (the cube sits on the line: the one edge, or the first round's path, is blocked)


def test_bad_endpoints_and_centres_outside_the_grid(detour):
    """An endpoint outside the limits and a NaN endpoint give status 2 and touch nothing else; on a field whose grid covers
    only a corner of the workspace the sphere centres outside it count as free, as the restatement has it."""
    from mpinets_amd import robot
    from mpinets_amd.field import CloudField

    n = 8
    a, b, c = detour["a"][:n].clone(), detour["b"][:n].clone(), detour["c"][:n]
    a[2, 3] = float("nan")
    b[3, 0] = 3.0  # outside the limits
    kw = dict(detour["kw"], field=sliced(detour["field"], slice(0, n)))
    traj, st, path, hops, nd, es, rounds = host(robot.franka_roadmap_cloud(a, b, c, return_graph=True, **kw))
    whole = detour["host"]
    assert st[2] == 2 and st[3] == 2 and rounds[2] == 0 and rounds[3] == 0 and es[2, 0, 0] == 2 and es[3, 1, 1] == 2
    assert np.isnan(traj[[2, 3]]).all() and (path[[2, 3]] == -1).all()
    keep = np.array([0, 1, 4, 5, 6, 7])
    for got, want in zip((traj, st, path, hops, nd, es, rounds), whole):
        assert np.array_equal(got[keep], want[:n][keep], equal_nan=True)
    # a grid over the cube's neighbourhood only: x, y in [0, 0.9], z in [0, 1.2]
    small = CloudField.build(c, lo=(0.0, 0.0, 0.0), hi=(0.9, 0.9, 1.2), truncation=detour["field"].truncation)
    got = host(robot.franka_roadmap_cloud(detour["a"][:n], detour["b"][:n], c, return_graph=True, **dict(detour["kw"], field=small)))
    want = frc.solve(detour["qs"][:n], detour["qg"][:n], small.values.cpu().numpy(), grid_dict(small.grid), POINT_RADIUS,
                     limits=detour["lim"], seed=DETOUR_PLAN_SEED)
    print(f"small grid: status {got[1].tolist()}, restatement {want[1].tolist()}")
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    _check_search(got[4], got[5], got[1], got[2], got[3], got[6], fr.DEFAULTS["max_rounds"])
    assert not np.array_equal(got[5], whole[5][:n])  # (the smaller grid does see less)


def test_sharding(detour):
    """Rows 48 .. 95 run alone with ``env_offset`` = 48 equal the same rows of the whole batch, every output; B = 1 too."""
    from mpinets_amd import robot

    for o, n in ((48, 48), (95, 1)):
        rows = slice(o, o + n)
        kw = dict(detour["kw"], field=sliced(detour["field"], rows))
        part = robot.franka_roadmap_cloud(detour["a"][rows], detour["b"][rows], detour["c"][rows], return_graph=True,
                                          env_offset=o, **kw)
        for name, g, w in zip(("traj", "status", "path", "hops", "nodes", "edge_state", "rounds"), part, detour["road"]):
            assert same(g, w[rows]), name


@pytest.fixture(scope="module")
def planners(detour):
    """The first 24 rows: the plain cloud planner, the seeded one from the roadmap's trajectory, and the two in one call."""
    from mpinets_amd import robot

    n = PLAN_ROWS
    a, b, c = detour["a"][:n], detour["b"][:n], detour["c"][:n]
    kw = dict(detour["kw"], field=sliced(detour["field"], slice(0, n)), return_all=True)
    plain = robot.franka_plan_cloud(a, b, c, **kw)
    seeds = detour["road"][0][:n, None].contiguous()
    seeded = robot.franka_plan_cloud(a, b, c, seeds=seeds, **kw)
    glob = robot.franka_plan_global_cloud(a, b, c, **kw)
    return a, b, c, kw, seeds, plain, seeded, glob


def test_seeded_planner(detour, planners, monkeypatch):
    """Candidates 0 .. K-1 of the seeded entry are bit-equal to the plain entry's; an empty seed tensor is the plain call; a
    NaN seed gets bits 7 and a NaN candidate and leaves every other row as it was; two seeds give K + 2 rows; two slabs
    equal one."""
    from mpinets_amd import robot, solvers

    a, b, c, kw, seeds, plain, seeded, glob = planners
    n = PLAN_ROWS
    assert seeded[3].shape == (n, K + 1, T, 7) and seeded[4].shape == (n, K + 1)
    assert same(seeded[3][:, :K], plain[3]) and same(seeded[4][:, :K], plain[4])
    for g, w in zip(robot.franka_plan_cloud(a, b, c, seeds=seeds[:, :0], **kw), plain):
        assert same(g, w)
    planned = plain[1] != 2
    found = torch.isfinite(seeds).all(dim=(1, 2, 3))
    assert int((planned & found).sum()) > 0 and int((planned & ~found).sum()) > 0
    dead = planned & ~found  # (the roadmap's NaN rows are NaN seeds)
    assert bool((seeded[4][dead, K] == 7).all()) and bool(torch.isnan(seeded[3][dead, K]).all())
    assert not bool(torch.isnan(seeded[3][planned & found]).any())
    # a NaN put into one live seed: that row's seed dies, nothing else moves
    row = int(torch.nonzero(planned & found)[0, 0])
    hurt = seeds.clone()
    hurt[row, 0, 7, 2] = float("nan")
    got = robot.franka_plan_cloud(a, b, c, seeds=hurt, **kw)
    assert int(got[4][row, K]) == 7 and bool(torch.isnan(got[3][row, K]).all())
    assert same(got[3][row, :K], seeded[3][row, :K]) and same(got[4][row, :K], seeded[4][row, :K])
    others = torch.arange(n, device=dev()) != row
    for g, w in zip(got, seeded):
        assert same(g[others], w[others])
    # two seeds: K + 2 rows, the first K + 1 as before (the line as a second seed)
    two = torch.cat([seeds, up(fp.line(detour["qs"][:n], detour["qg"][:n], T))[:, None]], 1).contiguous()
    got2 = robot.franka_plan_cloud(a, b, c, seeds=two, **kw)
    assert got2[3].shape == (n, K + 2, T, 7) and same(got2[3][:, :K + 1], seeded[3]) and same(got2[4][:, :K + 1], seeded[4])
    for g, w in zip(got2[:3], seeded[:3]):  # (a later candidate never displaces an earlier valid one: the line is blocked anyway)
        assert same(g, w)
    per = int(robot._lib.load().mpx_franka_plan_cloud_scratch(1, T, K + 1, SUBSTEPS))
    monkeypatch.setattr(solvers, "PLAN_CLOUD_SCRATCH_BYTES", 13 * per)  # 24 rows in slabs of 13 and 11
    for g, w in zip(robot.franka_plan_cloud(a, b, c, seeds=seeds, **kw), seeded):
        assert same(g, w)


def test_global_cloud_planner_on_the_forced_detour(detour, planners):
    """``franka_plan_global_cloud`` solves more of the 24 rows than ``franka_plan_cloud`` and at least the restatement's count
    minus the tolerance of tests/test_gpu_cloud_plan.py::test_forced_detour; every row the plain planner solves comes back
    identical; every returned trajectory is free by ``check_cloud`` on its refined configurations, inside the limits, its
    endpoints bit-equal."""
    from mpinets_amd.robot import FrankaCollisionSampler

    a, b, c, kw, seeds, plain, seeded, glob = planners
    traj, status, choice, all_traj, all_status, rm_status = glob
    for g, w in zip(glob[:5], seeded):  # the call is the two stages
        assert same(g, w)
    assert torch.equal(rm_status, detour["road"][1][:PLAN_ROWS])
    ok, plain_ok = status == 0, plain[1] == 0
    n_glob, n_plain = int(ok.sum()), int(plain_ok.sum())
    print(f"forced detour as a cloud, {PLAN_ROWS} rows: plain solves {n_plain}, with the roadmap {n_glob} of "
          f"{int((status != 2).sum())} planned; restatement {DETOUR_SEEDED_SOLVED}; choice histogram "
          f"{torch.bincount(choice[ok], minlength=K + 1).tolist()}; roadmap status {rm_status.tolist()}")
    assert n_glob > n_plain
    assert n_glob >= DETOUR_SEEDED_SOLVED - max(2, 2 * RECORDED_DISAGREEMENTS)
    assert bool(ok[plain_ok].all()) and same(traj[plain_ok], plain[0][plain_ok]) and torch.equal(choice[plain_ok], plain[2][plain_ok])
    rows = torch.nonzero(ok)[:, 0]
    fine = fp.refine(traj[rows].double().cpu(), SUBSTEPS).float().to(dev()).contiguous()
    assert not bool(FrankaCollisionSampler(dev()).check_cloud(fine, c[rows].contiguous(), point_radius=POINT_RADIUS).any())
    lim32 = up(fp.limits32(detour["lim"]))
    assert bool(((traj[rows] >= lim32[:, 0]) & (traj[rows] <= lim32[:, 1])).all())
    assert torch.equal(traj[rows][:, 0], a[rows]) and torch.equal(traj[rows][:, -1], b[rows])
    assert bool(torch.isnan(traj[~ok]).all())


def test_plan_to_poses_and_the_expert_with_the_roadmap():
    """``plan_to_poses(global_plan=True)`` and ``make_problem_batch(expert_from="cloud_roadmap")`` on 8 rows: the keys are
    there, valid rows are free by ``check_cloud``, and every row the default solves is returned as the default returns it;
    the defaults equal the calls they are made of."""
    from mpinets_amd import capture, robot, scenes
    from mpinets_amd.robot import FrankaCollisionSampler

    torch.cuda.set_device(0)
    B, pr = 8, scenes.EXPERT_CLOUD_POINT_RADIUS
    kw = dict(seed=4, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16, collision_free=True)
    coll = FrankaCollisionSampler(dev())

    def free(traj, cloud):
        fine = fp.refine(traj.double().cpu(), SUBSTEPS).float().to(dev()).contiguous()
        return not bool(coll.check_cloud(fine, cloud.contiguous(), point_radius=pr).any())

    prob = scenes.make_problem_batch(B, device=dev(), device_clouds=True, **kw)
    cloud = prob["xyz"][:, 2048:6144, :3]
    base = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4)
    q_goal, ik_st = robot.franka_ik_cloud(prob["target_pose"], cloud, point_radius=pr, seed=4)
    t0, s0 = robot.franka_plan_cloud(prob["q"], q_goal, cloud, point_radius=pr, seed=4)
    assert same(base["q_goal"], q_goal) and same(base["trajectory"], t0) and torch.equal(base["plan_status"], s0)
    assert sorted(base) == ["ik_status", "plan_status", "q_goal", "trajectory", "valid"]
    out = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4, global_plan=True)
    assert sorted(out) == ["ik_status", "plan_status", "q_goal", "roadmap_status", "trajectory", "valid"]
    print(f"plan_to_poses: plan status {base['plan_status'].tolist()}, global {out['plan_status'].tolist()}, roadmap "
          f"{out['roadmap_status'].tolist()}")
    assert same(out["q_goal"], base["q_goal"]) and out["roadmap_status"].shape == (B,) and out["roadmap_status"].dtype == torch.int32
    assert bool(out["valid"][base["valid"]].all()) and same(out["trajectory"][base["valid"]], base["trajectory"][base["valid"]])
    assert torch.equal(out["valid"], (out["ik_status"] == 0) & (out["plan_status"] == 0))
    v = out["valid"]
    if bool(v.any()):
        assert free(out["trajectory"][v], cloud[v])
        assert torch.equal(out["trajectory"][v][:, 0], prob["q"][v]) and torch.equal(out["trajectory"][v][:, -1], q_goal[v])

    plain = scenes.make_problem_batch(B, expert=True, expert_from="cloud", **kw)
    road = scenes.make_problem_batch(B, expert=True, expert_from="cloud_roadmap", **kw)
    assert set(road) == set(plain)
    ev, pv = road["expert_valid"], plain["expert_valid"]
    print(f"expert_from='cloud': {int(pv.sum())} of {B} planned; 'cloud_roadmap': {int(ev.sum())}")
    assert all(same(road[k], plain[k]) for k in road if torch.is_tensor(road[k]) and k not in ("global_solutions", "expert_valid"))
    assert bool(ev[pv].all()) and same(road["global_solutions"][pv], plain["global_solutions"][pv])
    sol = road["global_solutions"]
    assert sol.shape == (B, 50, 7) and bool(torch.isnan(sol[~ev]).all()) and not bool(torch.isnan(sol[ev]).any())
    if bool(ev.any()):
        assert free(sol[ev], road["xyz"][ev][:, 2048:6144, :3])
        assert torch.equal(sol[ev][:, 0], road["q"][ev]) and torch.equal(sol[ev][:, -1], road["q_goal"][ev])
    assert scenes.problems_to_dataset(road)["global_solutions"].shape == (int(ev.sum()), 50, 7)
