"""GPU: ``mpx_franka_roadmap`` (csrc/roadmap.hip), ``mpx_franka_plan_seeded`` (csrc/plan.hip) and ``robot.franka_plan_global``
against the float64 restatement (tests/float64_roadmap.py), against the judges that predate the planner
(tests/test_gpu_plan.py's ``judge``) and at their edges.  One module-scoped fixture per scenario: a launch runs once.

The search is checked on the DEVICE's own ``edge_state`` (every path edge free, the path's float64 cost that of an
independent shortest-path routine over the edges the device did not block), so no test depends on how float32 breaks a
tie between two paths; the verdicts in ``edge_state`` are checked one by one against float64."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_plan as fp  # noqa: E402
import float64_roadmap as fr  # noqa: E402
from float64_collision import SDF_BAR  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_plan import both_limits, dev, device_scene, judge, prims_of, take  # noqa: E402
from test_plan_host import MIXED, RECORDED_DISAGREEMENTS  # noqa: E402
from test_roadmap_host import DETOUR_GLOBAL_SOLVED, DETOUR_PLAN_SEED, LEFT_OUT_CAP, SEED_REFERENCE, detour_problems, \
    graph_verdicts  # noqa: E402

pytestmark = pytest.mark.gpu

V, T = 64, 50
# A refined configuration is interpolated in float32 on the device and in float64 by ``float64_plan.refine``: up to one ulp
# (2^-22 below 4 rad) on each of 7 joints, each moving a sphere by at most its lever arm (< 1 m), on top of the SDF's own
# float32 band.  Verdicts of ``float64_plan.validity`` are compared where moving the margin by this much changes nothing.
VALIDITY_BAND = SDF_BAR + 7 * 2.0 ** -22


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@pytest.fixture(scope="module")
def detour():
    """The 256 forced-detour problems of tests/test_gpu_plan.py (one 10 cm cube on the straight line): the roadmap with its
    graph, the plain planner, and the roadmap followed by the seeded planner, all at the planner's seed."""
    from mpinets_amd import robot

    torch.cuda.set_device(0)
    qs, qg, lim, scn = detour_problems()
    cub, cyl = prims_of(scn)
    a, b = _t(qs), _t(qg)
    kw = dict(seed=DETOUR_PLAN_SEED, limits=lim)
    road = robot.franka_roadmap(a, b, cub, cyl, return_graph=True, **kw)
    plain = robot.franka_plan(a, b, cub, cyl, return_all=True, **kw)
    glob = robot.franka_plan_global(a, b, cub, cyl, return_all=True, **kw)
    return qs, qg, lim, cub, cyl, road, plain, glob


def test_nodes_are_the_restatements_philox_draws(detour):
    """``nodes`` is bit-equal to the restatement's draw (stream 16, keyed by seed, global problem id and node); nodes 0 and
    1 are the endpoints."""
    qs, qg, lim, cub, cyl, (traj, status, path, hops, nodes, state, rounds), _, _ = detour
    want = fr.draw_nodes(qs, qg, lim, V, seed=DETOUR_PLAN_SEED)
    assert np.array_equal(nodes.cpu().numpy(), want)
    assert torch.equal(nodes[:, 0], _t(qs)) and torch.equal(nodes[:, 1], _t(qg))


def test_edge_state_against_float64(detour):
    """The diagonal and every tested edge of ``edge_state`` carry the float64 verdict, recomputed from the device's own
    float32 nodes and the stated pieces; a problem is left out when a configuration that decides one of its verdicts lies
    within SDF_BAR (tests/float64_collision.py, 9e-7 m) of its threshold.  The count left out is printed and capped at
    LEFT_OUT_CAP of the problems (tests/test_roadmap_host.py holds the restatement itself to the cap at this seed).
    Untested entries are 0, the matrix is symmetric, status-2 rows hold their diagonal only."""
    qs, qg, lim, cub, cyl, (traj, status, path, hops, nodes, state, rounds), _, _ = detour
    scene = device_scene(cub, cyl)
    nd, es, st = nodes.cpu().numpy(), state.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(es, es.transpose(0, 2, 1)) and es.max() <= 2
    off = es * (1 - np.eye(V, dtype=np.uint8))
    assert (off[st == 2] == 0).all() and (rounds.cpu().numpy()[st == 2] == 0).all()
    left, wrong, tested = 0, [], 0
    for b in range(len(qs)):
        want, in_band = graph_verdicts(nd[b], es[b], {k: v[b:b + 1] for k, v in scene.items()})
        left += in_band
        known = want != 0
        tested += int(np.triu(known, 1).sum())
        if not in_band and not np.array_equal(want[known], es[b][known]):
            wrong.append(b)
    print(f"edge_state against float64: {len(qs)} problems, {tested} tested edges, {left} problems left out "
          f"({left / len(qs):.4f}), disagreeing problems {wrong}")
    assert left / len(qs) <= LEFT_OUT_CAP
    assert not wrong
    assert ((es[:, 0, 0] == 1) & (es[:, 1, 1] == 1))[st != 2].all() and ((es[:, 0, 0] == 2) | (es[:, 1, 1] == 2))[st == 2].all()


def _check_search(nd, es, st, pa, hp, rd, max_rounds):
    for b in range(len(st)):
        cost = fr.dijkstra_cost(nd[b], es[b])
        if st[b] == 0:
            p = pa[b, :hp[b] + 1]
            assert p[0] == 0 and p[-1] == 1 and (pa[b, hp[b] + 1:] == -1).all() and len(set(p.tolist())) == len(p)
            assert all(es[b, u, v] == fr.FREE for u, v in zip(p[:-1], p[1:])), b
            assert abs(fr.path_cost(nd[b], p) - cost) <= len(nd[b]) * 2.0 ** -23 * cost, b
            assert 1 <= rd[b] <= max_rounds
        else:
            assert hp[b] == 0 and (pa[b] == -1).all()
            if st[b] == 1:
                assert not np.isfinite(cost) or rd[b] == max_rounds, b


def test_search_invariant_on_the_devices_own_edge_state(detour):
    """Status 0: every edge of ``path`` is in state 1 and the float64 cost of ``path`` equals, within V 2^-23 relative,
    the cost of the shortest path over "valid nodes, edges not in state 2" found by a heap on the device's ``edge_state``.
    Status 1: node 1 cannot be reached in that graph, or the rounds ran out (a second run with 3 rounds makes them run out)."""
    from mpinets_amd import robot

    qs, qg, lim, cub, cyl, road, _, _ = detour
    traj, status, path, hops, nodes, state, rounds = (x.cpu().numpy() for x in road)
    _check_search(nodes, state, status, path, hops, rounds, fr.DEFAULTS["max_rounds"])
    print(f"roadmap on the detour problems: status 0 / 1 / 2 = {np.bincount(status, minlength=3).tolist()}, hops histogram "
          f"{np.bincount(hops[status == 0]).tolist()}, rounds histogram {np.bincount(rounds).tolist()}")
    assert (status == 0).sum() >= 100 and (hops[status == 0] >= 2).all()  # (the cube sits on the line)
    n = 96
    c, y = take((cub, cyl), torch.arange(n, device=dev()))
    short = robot.franka_roadmap(_t(qs[:n]), _t(qg[:n]), c, y, seed=DETOUR_PLAN_SEED, limits=lim, return_graph=True, max_rounds=3)
    s_traj, s_status, s_path, s_hops, s_nodes, s_state, s_rounds = (x.cpu().numpy() for x in short)
    _check_search(s_nodes, s_state, s_status, s_path, s_hops, s_rounds, 3)
    ran_out = (s_status == 1) & (s_rounds == 3)
    assert ran_out.sum() >= 4 and (status[:n][ran_out] != 2).all()
    same = s_rounds <= 2  # a search that ends within the budget does not see the budget
    assert np.array_equal(s_path[same & (s_status == 0)], path[:n][same & (s_status == 0)])


@pytest.fixture(scope="module")
def free():
    from mpinets_amd import robot, scenes

    torch.cuda.set_device(0)
    B = 64
    qs, qg = scenes.random_configurations(B, 31), scenes.random_configurations(B, 32)
    out = robot.franka_roadmap(_t(qs), _t(qg), return_graph=True)
    return qs, qg, out


def test_seed_trajectory(detour, free):
    """``traj`` equals the float64 resample-and-smooth of the device's own ``path`` and ``nodes`` within 4 x SEED_REFERENCE
    (tests/test_roadmap_host.py: the float32 against the float64 run of the restatement on the detour paths, 7.7e-7 rad:
    the bar is 3.1e-6 rad); a one-edge path is the planner's line bit for bit; waypoints 0 and T-1 are bit-equal to the
    endpoints; rows with status != 0 are NaN."""
    qs, qg, lim, cub, cyl, (traj, status, path, hops, nodes, state, rounds), _, _ = detour
    tr, st, pa, hp, nd = (x.cpu().numpy() for x in (traj, status, path, hops, nodes))
    ok = st == 0
    worst = 0.0
    for b in np.flatnonzero(ok):
        want = fr.seed_trajectory(nd[b], pa[b, :hp[b] + 1].tolist(), T, fr.DEFAULTS["smooth_passes"])
        worst = max(worst, float(np.abs(tr[b].astype(np.float64) - want).max()))
    print(f"seed trajectory against float64 over {int(ok.sum())} paths: max {worst:.3e} (bar {4 * SEED_REFERENCE:.2e})")
    assert worst <= 4 * SEED_REFERENCE
    assert np.array_equal(tr[ok][:, 0], qs[ok]) and np.array_equal(tr[ok][:, -1], qg[ok])
    assert np.isnan(tr[~ok]).all() and not np.isnan(tr[ok]).any()
    lim32 = fp.limits32(lim)
    assert ((tr[ok] >= lim32[:, 0]) & (tr[ok] <= lim32[:, 1])).all()
    # free space: one round, the path 0 -> 1, the line itself
    fqs, fqg, (ftraj, fstatus, fpath, fhops, fnodes, fstate, frounds) = free
    fst = fstatus.cpu().numpy()
    planned = fst != 2  # (a uniform draw can itself be a self collision)
    assert planned.sum() >= 16
    L = fp.line(fqs, fqg, T)
    one = planned & (fhops.cpu().numpy() == 1)
    assert one.sum() >= 8
    assert np.array_equal(ftraj.cpu().numpy()[one], L[one])
    assert (frounds.cpu().numpy()[one] == 1).all() and (fpath.cpu().numpy()[one][:, :2] == [0, 1]).all()


def _guarded(shape, dtype, fill):
    """A tensor with a guard row in front and behind: -> (whole, view)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev())
    return whole, whole[1:-1]


@pytest.mark.parametrize("B,nodes,T_,with_prims", [(0, 64, 50, True), (1, 64, 50, True), (65, 64, 50, True), (65, 2, 50, True),
                                                   (65, 64, 2, True), (65, 3, 3, True), (65, 64, 50, False), (4, 256, 64, True),
                                                   (33, 100, 7, True)])
def test_edges_sizes_and_guard_rows(B, nodes, T_, with_prims):
    """Every output buffer is written exactly: guard rows around traj / status / path / hops / nodes / edge_state / rounds
    keep their fill.  V = 2: status 0 exactly when the straight edge is free.  T = 2: the endpoints.  No primitives (S = 0):
    one round, the path 0 -> 1.  An endpoint in collision, outside the limits or NaN gives status 2 and nothing else.
    V = 256 on 4 problems, V = 100 (no multiple of a wave) on 33."""
    from mpinets_amd import _lib, robot, scenes

    torch.cuda.set_device(0)
    M1, M2 = (12, 4) if with_prims else (0, 0)
    scn = scenes.make_scenes(max(B, 1), 5, MIXED, 12, 4)
    cub, cyl = prims_of({k: v[:B] for k, v in scn.items()})
    qs = _t(scenes.random_configurations(B, 41))
    qg = _t(scenes.random_configurations(B, 42))
    if B == 65:
        qs[3, 2] = float("nan")
        qg[4, 0] = 3.0  # outside the limits
        qs[5] = torch.tensor([0.0, 1.4, 0.0, -0.5, 0.0, 1.0, 0.0])  # reaches down through the mount table
    lim = _t(ft.limits_float32_inward(ft.JOINT_LIMITS_REAL))
    sc, sr, sl = robot._ik_sphere_table(dev(), False) if with_prims else (None, None, None)
    (wt, traj), (ws, status), (wh, hops), (wr, rounds) = _guarded((B, T_, 7), torch.float32, 7.0), \
        _guarded((B,), torch.int32, -9), _guarded((B,), torch.int32, -9), _guarded((B,), torch.int32, -9)
    (wp, path), (wn, nd), (we, es) = _guarded((B, nodes), torch.int32, -9), _guarded((B, nodes, 7), torch.float32, 7.0), \
        _guarded((B, nodes, nodes), torch.uint8, 9)
    opt = _lib.RoadmapOptions(nodes, 0.05, float("inf"), 16, 3, 1e-4, 0.0, 1)
    _lib.call("mpx_franka_roadmap", _lib.ptr(qs), _lib.ptr(qg), B, T_, ft.FINGER_OPENING, _lib.ptr(lim), _lib.ptr(sc), _lib.ptr(sr),
              _lib.ptr(sl), int(sc.size(0)) if with_prims else 0, _lib.ptr(cub.inv_frames) if with_prims else None,
              _lib.ptr(cub.dims) if with_prims else None, M1, _lib.ptr(cyl.inv_frames) if with_prims else None,
              _lib.ptr(cyl.radii) if with_prims else None, _lib.ptr(cyl.heights) if with_prims else None, M2,
              ctypes.byref(opt), 1, 0, _lib.ptr(traj), _lib.ptr(status), _lib.ptr(path), _lib.ptr(hops), _lib.ptr(nd),
              _lib.ptr(es), _lib.ptr(rounds))
    torch.cuda.synchronize()
    for whole, fill in ((wt, 7.0), (wn, 7.0), (ws, -9), (wh, -9), (wr, -9), (wp, -9), (we, 9)):
        assert bool((whole[0] == fill).all()) and bool((whole[-1] == fill).all())
    if B == 0:
        return
    assert bool(((status >= 0) & (status <= 2)).all())
    ok = status == 0
    assert int(ok.sum()) > 0
    assert not bool(torch.isnan(traj[ok]).any()) and bool(torch.isnan(traj[~ok]).all())
    assert torch.equal(traj[ok][:, 0], qs[ok]) and torch.equal(traj[ok][:, -1], qg[ok])
    assert bool((hops[ok] >= 1).all()) and bool((hops[ok] < nodes).all()) and bool((hops[~ok] == 0).all())
    assert bool((path[~ok] == -1).all()) and bool((path[ok][:, 0] == 0).all())
    last = torch.gather(path[ok], 1, hops[ok].long()[:, None])[:, 0]
    assert bool((last == 1).all())
    assert bool((es <= 2).all()) and torch.equal(es, es.transpose(1, 2))
    _check_search(nd.cpu().numpy(), es.cpu().numpy(), status.cpu().numpy(), path.cpu().numpy(), hops.cpu().numpy(),
                  rounds.cpu().numpy(), 16)
    if nodes == 2:  # the graph is its one edge
        planned = status != 2
        assert torch.equal(ok[planned], es[planned][:, 0, 1] == 1) and torch.equal((status == 1)[planned], es[planned][:, 0, 1] == 2)
        assert bool((rounds[ok] == 1).all()) and bool((rounds[status == 1] == 2).all()) and bool((hops[ok] == 1).all())
        assert int((status == 1).sum()) > 0  # (the scenes do block some straight edges)
    if T_ == 2:
        assert torch.equal(traj[ok], torch.stack([qs[ok], qg[ok]], 1))
    if not with_prims:  # only the self test and the limits can refuse anything: the straight edge is tested, once
        L = _t(fp.line(qs.cpu().numpy(), qg.cpu().numpy(), T_))
        direct = ok & (hops == 1)
        assert int(direct.sum()) > B // 2 and bool((rounds[direct] == 1).all())
        assert torch.equal(traj[direct], L[direct])
    if B == 65:
        bad = 3 if with_prims else 2  # (the third reaches into a primitive)
        assert status[3:3 + bad].tolist() == [2] * bad and rounds[3:3 + bad].tolist() == [0] * bad
        assert es[3, 0, 0] == 2 and es[4, 1, 1] == 2 and (not with_prims or es[5, 0, 0] == 2)
        off = es[3:3 + bad] * (1 - torch.eye(nodes, dtype=torch.uint8, device=dev()))
        assert bool((off == 0).all())


def test_determinism_sharding_and_seeds(detour):
    """Two runs are bit-equal; rows [o, o + n) of a batch equal the same problems run alone with env_offset = o, for the
    roadmap and for the roadmap followed by the seeded planner; another seed changes the nodes but not the endpoints."""
    from mpinets_amd import robot

    qs, qg, lim, cub, cyl, road, _, glob = detour
    a, b = _t(qs), _t(qg)
    kw = dict(seed=DETOUR_PLAN_SEED, limits=lim)
    again = robot.franka_roadmap(a, b, cub, cyl, return_graph=True, **kw)
    for got, want in zip(again, road):
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    o, n = 100, 60
    rows = torch.arange(o, o + n, device=dev())
    c, y = take((cub, cyl), rows)
    shard = robot.franka_roadmap(a[rows], b[rows], c, y, env_offset=o, return_graph=True, **kw)
    for got, want in zip(shard, road):
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want[rows]))
    unshifted = robot.franka_roadmap(a[rows], b[rows], c, y, return_graph=True, **kw)
    assert not torch.equal(unshifted[4][:, 2:], road[4][rows][:, 2:])
    gshard = robot.franka_plan_global(a[rows], b[rows], c, y, env_offset=o, return_all=True, **kw)
    for got, want in zip(gshard, glob):
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want[rows]))
    other = robot.franka_roadmap(a[rows], b[rows], c, y, env_offset=o, return_graph=True, seed=DETOUR_PLAN_SEED + 1, limits=lim)
    assert torch.equal(other[4][:, :2], road[4][rows][:, :2]) and not torch.equal(other[4][:, 2:], road[4][rows][:, 2:])


def test_seeded_optimiser(detour):
    """Ks = 0: every output, ``all_traj`` and ``all_status`` included, is bit-equal to ``franka_plan``'s.  Ks = 2: candidates
    0 .. K-1 are bit-equal; a NaN seed yields NaN rows and bits 7; the seeds' ``all_status`` equals the verdict of
    ``float64_plan.validity`` on the device's ``all_traj`` wherever moving the margin by VALIDITY_BAND (the jerk bound by
    1e-6) does not change that verdict."""
    from mpinets_amd import robot

    qs, qg, lim, cub, cyl, road, plain, _ = detour
    n, K = 96, fp.DEFAULTS["candidates"]
    rows = torch.arange(n, device=dev())
    c, y = take((cub, cyl), rows)
    a, b = _t(qs[:n]), _t(qg[:n])
    kw = dict(seed=DETOUR_PLAN_SEED, limits=lim, return_all=True)
    none = robot.franka_plan(a, b, c, y, seeds=torch.empty((n, 0, T, 7), device=dev()), **kw)
    for got, want in zip(none, plain):
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(want[:n]))
    # seed 0: the roadmap's trajectory (NaN where it found none); seed 1: the same pushed past the limits on joint 0 of its
    # interior (clamped back by the planner), NaN on every fourth row
    s0 = road[0][:n]
    s1 = s0.clone()
    s1[:, 1:-1, 0] += 10.0
    s1[:, 0] = 99.0  # (endpoints of a seed are replaced)
    s1[::4, 7, 3] = float("nan")
    traj, status, choice, all_traj, all_status = robot.franka_plan(a, b, c, y, seeds=torch.stack([s0, s1], 1), **kw)
    assert all_traj.shape == (n, K + 2, T, 7) and all_status.shape == (n, K + 2)
    p_traj, p_status, p_choice, p_all, p_bits = (x[:n] for x in plain)
    planned = p_status != 2
    assert torch.equal(status == 2, ~planned)
    assert torch.equal(torch.nan_to_num(all_traj[:, :K]), torch.nan_to_num(p_all)) and torch.equal(all_status[:, :K], p_bits)
    solved = p_status == 0
    assert torch.equal(traj[solved], p_traj[solved]) and torch.equal(choice[solved], p_choice[solved])
    dead0 = torch.isnan(s0).any(-1).any(-1)
    dead1 = torch.isnan(s1).any(-1).any(-1)
    assert int((dead0 & planned).sum()) > 0 and int((dead1 & ~dead0 & planned).sum()) > 0
    for k, dead in ((K, dead0), (K + 1, dead1)):
        assert bool((all_status[dead, k] == 7).all()) and bool(torch.isnan(all_traj[dead, k]).all())
        live = planned & ~dead
        assert not bool(torch.isnan(all_traj[live, k]).any())
        assert torch.equal(all_traj[live, k][:, 0], a[live]) and torch.equal(all_traj[live, k][:, -1], b[live])
    lim32 = _t(fp.limits32(lim))
    live1 = planned & ~dead1
    drawn = robot.franka_plan(a, b, c, y, seeds=torch.stack([s0, s1], 1), iterations=0, **kw)[3]  # (the candidates as they start)
    assert bool((drawn[live1, K + 1][:, 1:-1, 0] == lim32[0, 1]).all())  # clamped onto the upper limit of joint 0
    assert torch.equal(drawn[live1, K + 1][:, 1:-1, 1:], s1[live1][:, 1:-1, 1:]) and torch.equal(drawn[live1, K], s0[live1])
    first = torch.where((all_status == 0).any(1), (all_status == 0).int().argmax(1), torch.full_like(choice, -1)).int()
    assert torch.equal(first[planned], choice[planned]) and bool((choice[~planned] == -1).all())
    # the seeds' bits against float64_plan.validity on the device's own trajectories
    scene = {k: v[:n] for k, v in device_scene(cub, cyl).items()}
    live = (planned & ~dead0).cpu().numpy()
    sd = all_traj[:, K:K + 1].double().cpu()[torch.from_numpy(live)]
    sc = {k: v[live] for k, v in scene.items()}
    lo = fp.validity(sd, sc, check_margin=1e-4 - VALIDITY_BAND, max_jerk=0.15 * (1 + 1e-5)).numpy()[:, 0]
    hi = fp.validity(sd, sc, check_margin=1e-4 + VALIDITY_BAND, max_jerk=0.15 * (1 - 1e-5)).numpy()[:, 0]
    got = all_status[:, K].cpu().numpy()[live]
    decided = lo == hi
    print(f"seeded candidates against float64_plan.validity: {len(got)} seeds, {int((~decided).sum())} inside the band, bits "
          f"histogram {np.bincount(got, minlength=8).tolist()}")
    assert decided.mean() >= 1 - LEFT_OUT_CAP
    assert np.array_equal(got[decided], lo[decided])
    assert ((got & ~hi) == 0).all() and ((lo & ~got) == 0).all()  # inside the band: between the two verdicts, bit by bit


def test_global_planner_on_the_forced_detour(detour):
    """Why the roadmap exists.  Every row ``franka_plan`` solves is returned identically by ``franka_plan_global``; every
    returned trajectory passes the judges of tests/test_gpu_plan.py (``FrankaCollisionSampler.check`` on the refined
    configurations, the self test, the limits, third differences <= 0.15) and keeps its endpoints; the device solves at
    least as many problems as the float64 restatement (DETOUR_GLOBAL_SOLVED, recorded and re-derived by
    tests/test_roadmap_host.py) minus 2, the margin of ``test_forced_detour``."""
    qs, qg, lim, cub, cyl, road, plain, (traj, status, choice, all_traj, all_status, rm_status) = detour
    p_traj, p_status, p_choice, p_all, p_bits = plain
    K = p_all.shape[1]
    solved = p_status == 0
    assert torch.equal(traj[solved], p_traj[solved]) and torch.equal(choice[solved], p_choice[solved])
    assert bool((status[solved] == 0).all()) and torch.equal(status == 2, p_status == 2) and torch.equal(rm_status, road[1])
    assert torch.equal(torch.nan_to_num(all_traj[:, :K]), torch.nan_to_num(p_all)) and torch.equal(all_status[:, :K], p_bits)
    ok = status == 0
    rows = torch.nonzero(ok)[:, 0]
    c, y = take((cub, cyl), rows)
    env, self_hit, jerk, limit_violation = judge(traj[rows], c, y)
    assert not bool(env.any()) and not bool(self_hit.any()) and not bool(limit_violation.any())
    assert float(jerk.max()) <= 0.15
    assert torch.equal(traj[rows, 0], _t(qs)[rows]) and torch.equal(traj[rows, -1], _t(qg)[rows])
    assert bool(torch.isnan(traj[~ok]).all())
    n_plain, n_dev = int(solved.sum()), int(ok.sum())
    print(f"forced detour, 256 problems: franka_plan solves {n_plain}, franka_plan_global {n_dev} ({n_dev / 256:.4f}; "
          f"{int((status != 2).sum())} planned, roadmap status 0 / 1 / 2 = {torch.bincount(rm_status, minlength=3).tolist()}, choice "
          f"histogram {torch.bincount(choice[ok], minlength=K + 1).tolist()}); float64 restatement {DETOUR_GLOBAL_SOLVED}")
    assert n_dev >= DETOUR_GLOBAL_SOLVED - max(2, 2 * RECORDED_DISAGREEMENTS)
    assert n_dev > n_plain
    won = ok & ~solved
    assert bool((choice[won] == K).all())


def test_problem_batches_can_ask_for_the_roadmap():
    """``make_problem_batch(expert_from="roadmap")``: opt-in; everything but the demonstrations is what the default gives,
    every row the default solves is returned identically, and no fewer rows are solved."""
    from mpinets_amd import scenes

    torch.cuda.set_device(0)
    kw = dict(seed=4, kinds=MIXED, M1=40, M2=16, device_clouds=True, collision_free=True, expert=True)
    base = scenes.make_problem_batch(48, **kw)
    road = scenes.make_problem_batch(48, expert_from="roadmap", **kw)
    assert set(base) == set(road)
    for k in base:
        if torch.is_tensor(base[k]) and k not in ("global_solutions", "expert_valid"):
            assert torch.equal(torch.nan_to_num(base[k]), torch.nan_to_num(road[k])), k
    ev = base["expert_valid"]
    assert bool(road["expert_valid"][ev].all()) and torch.equal(road["global_solutions"][ev], base["global_solutions"][ev])
    assert bool(torch.isnan(road["global_solutions"][~road["expert_valid"]]).all())
