"""GPU: ``mpx_gripper_roadmap_cloud`` (csrc/gripper_roadmap_cloud.hip) and its two callers against the float64 restatement
(tests/float64_gripper_roadmap_cloud.py), against the primitive form (``robot.gripper_roadmap``), against the judge that
predates both (``FrankaCollisionSampler.check_cloud``) and at their edges, on three scenarios of 64 problems (the wall and the
upright cylinder of tests/float64_gripper_roadmap.py drawn as clouds, and no cloud; 64 nodes, 8 guide poses).  One
module-scoped fixture per launch: each runs once.

As for the primitive form, the search is checked on the DEVICE's own ``nodes`` and ``edge_state``; the verdicts in
``edge_state`` are recomputed in float64 from the device's float32 nodes and the field the DEVICE built, copied to the host, so
these tests judge the roadmap kernel and not the field build (tests/test_gpu_cloud_field.py holds that), outside ``CLOUD_BAND``
(tests/test_gripper_roadmap_cloud_host.py derives it, and holds the restatement to the left-out cap at this seed)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_plan as fcp  # noqa: E402
import float64_gripper_roadmap as fg  # noqa: E402
import float64_gripper_roadmap_cloud as fgc  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_cloud_plan import build_field, grid_dict  # noqa: E402
from test_gpu_gripper_roadmap import check_nodes, check_search, same  # noqa: E402
from test_gpu_roadmap_cloud import sliced  # noqa: E402
from test_gripper_roadmap_cloud_host import CLOUD_BAND, CONSERVATIVE_SLACK, LIPSCHITZ, PROMISE_BAND, promised_margin  # noqa: E402
from test_gripper_roadmap_host import FOUND_SHARE, LEFT_OUT_CAP  # noqa: E402

pytestmark = pytest.mark.gpu

B, V, W = 64, 64, 8
SEED = fgc.ROADMAP_SEED
PR = fgc.POINT_RADIUS
MAX_ROUNDS = fg.DEFAULTS["max_rounds"]
KINDS = fgc.KINDS
NAMES = ("poses", "status", "path", "hops", "nodes", "edge_state", "rounds")
REACH = float(np.float32(0.0) + np.float32(1e-4))  # clearance + check_margin of the defaults, summed in float32


def dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(out):
    return tuple(x.cpu().numpy() for x in out)


@pytest.fixture(scope="module")
def problems():
    torch.cuda.set_device(0)
    return fg.problems(B)


@pytest.fixture(scope="module")
def scenario():
    """kind -> dict(cloud tensor [B,N,3] or None, points [N,3], field (built by the device, one per problem and all alike),
    values: row 0 of it on the host, grid)."""
    torch.cuda.set_device(0)
    out = {}
    for kind in KINDS:
        pts = fgc.surface_cloud(kind)
        if pts is None:
            out[kind] = dict(cloud=None, points=None, field=None, values=None, grid=None)
            continue
        cloud = _t(pts)[None].repeat(B, 1, 1)
        field = build_field(cloud, PR)
        assert torch.equal(field.values, field.values[:1].expand_as(field.values))  # (one cloud: one field)
        grid = grid_dict(field.grid)
        assert (grid["nx"], grid["ny"], grid["nz"]) == tuple(fgc.scenario_grid()[k] for k in ("nx", "ny", "nz"))
        out[kind] = dict(cloud=cloud, points=pts, field=field, values=field.values[0].cpu().numpy(), grid=grid)
    return out


def plan(scenario, sp, gp, kind, rows=slice(None), **kw):
    from mpinets_amd import robot

    s = scenario[kind]
    kw.setdefault("seed", SEED)
    if "field" not in kw:
        kw["field"] = None if s["field"] is None else sliced(s["field"], rows)
    cloud = kw.pop("cloud", None if s["cloud"] is None else s["cloud"][rows])
    return robot.gripper_roadmap_cloud(_t(sp), _t(gp), cloud, point_radius=kw.pop("point_radius", PR), W=kw.pop("W", W),
                                       return_graph=True, **kw)


@pytest.fixture(scope="module")
def runs(problems, scenario):
    """kind -> (the seven outputs as tensors, the same as numpy): one launch per scenario."""
    sp, gp = problems
    out = {}
    for kind in KINDS:
        res = plan(scenario, sp, gp, kind)
        out[kind] = (res, host(res))
    return out


@pytest.fixture(scope="module")
def bare(problems):
    """``robot.gripper_roadmap`` without primitives at the same seed: the primitive form's nodes, and what "no environment" gives."""
    from mpinets_amd import robot

    sp, gp = problems
    return robot.gripper_roadmap(_t(sp), _t(gp), W=W, seed=SEED, return_graph=True)


# ---- the checks of the cloud rule, on numpy outputs ----------------------------------------------------------------------------
def check_edge_state(s, st, nodes, es, rounds, what, **rule):
    rule.setdefault("point_radius", PR)
    n, v = es.shape[:2]
    assert np.array_equal(es, es.transpose(0, 2, 1)) and es.max() <= 2
    off = es * (1 - np.eye(v, dtype=np.uint8))
    assert (off[st == 2] == 0).all() and (rounds[st == 2] == 0).all()
    left, wrong, tested = 0, [], 0
    for b in range(n):
        want, in_band, _ = fgc.graph_verdicts(nodes[b], np.ones(v, bool), es[b], s["values"], s["grid"], CLOUD_BAND, **rule)
        left += in_band
        known = want != 0
        tested += int(np.triu(known, 1).sum())
        if not in_band and not np.array_equal(want[known], es[b][known]):
            wrong.append(b)
    print(f"{what}: edge_state against float64, {n} problems, {tested} tested edges, {left} problems left out "
          f"({left / n:.4f}), disagreeing problems {wrong}")
    assert left / n <= LEFT_OUT_CAP
    assert not wrong
    assert ((es[:, 0, 0] == 1) & (es[:, 1, 1] == 1))[st != 2].all() and ((es[:, 0, 0] == 2) | (es[:, 1, 1] == 2))[st == 2].all()


def check_poses(s, gp, poses, st, pa, hp, nd, what, **rule):
    rule.setdefault("point_radius", PR)
    found = st == 0
    assert np.isnan(poses[~found]).all() and (pa[~found] == -1).all() and (hp[~found] == 0).all()  # NaN rows exactly where status != 0
    assert not np.isnan(poses[found]).any()
    assert np.array_equal(poses[found][:, -1], gp[found])  # the goal as given, bit for bit
    R = poses[found][:, :, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max() <= 1e-6
    assert np.array_equal(poses[found][:, :, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), poses[found][:, :, 3].shape))
    worst_p = worst_r = 0.0
    low = np.inf
    for b in np.flatnonzero(found):
        want = fg.resample(nd[b], pa[b, :hp[b] + 1], poses.shape[1])
        worst_p = max(worst_p, float(np.abs(poses[b, :-1, :3, 3] - want[:-1, :3, 3]).max(initial=0.0)))
        worst_r = max(worst_r, float(np.abs(poses[b, :-1, :3, :3] - want[:-1, :3, :3]).max(initial=0.0)))
        env, own = fgc.margins(fg.pose_nodes(poses[b].astype(np.float64)), s["values"], s["grid"], **rule)
        low = min(low, float(np.minimum(env, own).min()))
    print(f"{what}: poses against the float64 resampling of the device's own path, position {worst_p:.3e} m, rotation entries "
          f"{worst_r:.3e}; smallest float64 margin of a guide pose {low:.3e} m")
    assert worst_p <= 2e-6 and worst_r <= 2e-6  # (the primitive form's bars: the same arithmetic)
    assert low > -CLOUD_BAND  # every pose valid by the float64 rule, outside the band


# ---- 1: nodes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nodes_are_the_primitive_forms(problems, runs, bare, kind):
    """Bit-equal to ``robot.gripper_roadmap``'s at the same seed; positions bit-equal to the float32 restatement of the draw,
    quaternions within 2^-22 of it."""
    assert torch.equal(runs[kind][0][4], bare[4])
    check_nodes(*problems, runs[kind][1][4])


# ---- 2: edge state -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_edge_state_against_float64(scenario, runs, kind):
    poses, st, pa, hp, nd, es, rd = runs[kind][1]
    check_edge_state(scenario[kind], st, nd, es, rd, kind)


# ---- 3: search -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_search_invariant_on_the_devices_own_edge_state(runs, kind):
    poses, st, pa, hp, nd, es, rd = runs[kind][1]
    check_search(nd, es, st, pa, hp, rd, MAX_ROUNDS)
    print(f"{kind}: status 0 / 1 / 2 = {np.bincount(st, minlength=3).tolist()}, hops histogram {np.bincount(hp[st == 0]).tolist()}, "
          f"rounds histogram {np.bincount(rd).tolist()}")
    if kind != "free":  # the obstacle is gone round, on at least FOUND_SHARE of the rows (the restatement does at this seed)
        assert (hp[st == 0] >= 2).all() and (st == 0).mean() >= FOUND_SHARE


def test_rounds_run_out_and_a_search_within_the_budget_does_not_see_it(problems, scenario, runs):
    sp, gp = problems
    poses, st, pa, hp, nd, es, rd = runs["wall"][1]
    s_poses, s_st, s_pa, s_hp, s_nd, s_es, s_rd = host(plan(scenario, sp, gp, "wall", max_rounds=3))
    check_search(s_nd, s_es, s_st, s_pa, s_hp, s_rd, 3)
    ran_out = (s_st == 1) & (s_rd == 3)
    assert ran_out.sum() >= 4 and (st[ran_out] != 2).all()
    within = s_rd <= 2
    assert np.array_equal(s_pa[within & (s_st == 0)], pa[within & (s_st == 0)])
    assert np.array_equal(s_nd, nd)
    assert np.isnan(s_poses[s_st != 0]).all() and not np.isnan(s_poses[s_st == 0]).any()


def test_connect_radius_below_the_direct_edge(problems, scenario, runs):
    sp, gp = problems
    nd = runs["cylinder"][1][4]
    direct = np.array([fg.lengths(nd[b, :2], dtype=np.float32)[0, 1] for b in range(B)])
    radius = float(direct.min()) * 0.75
    poses, st, pa, hp, nd2, es, rd = host(plan(scenario, sp, gp, "cylinder", connect_radius=radius))
    assert np.array_equal(nd2, nd)
    check_search(nd2, es, st, pa, hp, rd, MAX_ROUNDS, connect_radius=radius)
    assert (hp[st == 0] >= 2).all() and (st != 2).all() and (st == 0).any()
    for b in np.flatnonzero(st == 0):
        p = pa[b, :hp[b] + 1]
        w = fg.lengths(nd2[b][p], dtype=np.float32)
        assert all(w[i, i + 1] <= np.float32(radius) for i in range(hp[b]))


# ---- 4: guide poses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_poses(problems, scenario, runs, kind):
    (t_poses, t_st, *_), (poses, st, pa, hp, nd, es, rd) = runs[kind]
    check_poses(scenario[kind], problems[1], poses, st, pa, hp, nd, kind)
    assert torch.equal(t_poses[t_st == 0][:, -1], _t(problems[1])[t_st == 0])


# ---- 5: what the field promises ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("wall", "cylinder"))
def test_what_the_field_promises(problems, scenario, runs, kind):
    """``field_slack = 0.866 x voxel``: every sphere of every guide pose of a found row is free by the exact float64
    brute-force distance to the cloud, ``dist - point_radius - r - clearance > check_margin - PROMISE_BAND``; with no slack
    the same margin is above ``-(sqrt(3)/2) voxel - PROMISE_BAND`` (tests/test_gripper_roadmap_cloud_host.py derives both)."""
    sp, gp = problems
    s = scenario[kind]
    slack = host(plan(scenario, sp, gp, kind, field_slack=CONSERVATIVE_SLACK))
    for name, (poses, st), floor in (("no slack", runs[kind][1][:2], -LIPSCHITZ * fcp.VOXEL - PROMISE_BAND),
                                     ("0.866 voxel", slack[:2], fg.DEFAULTS["check_margin"] - PROMISE_BAND)):
        found = np.flatnonzero(st == 0)
        assert len(found)
        low = min(promised_margin(poses[b], s["points"]) for b in found)
        print(f"{kind}, {name}: {len(found)} of {len(st)} rows found; smallest exact margin of a guide pose's sphere {low:.4e} m "
              f"(floor {floor:.4e})")
        assert low > floor
    check_search(slack[4], slack[5], slack[1], slack[2], slack[3], slack[6], MAX_ROUNDS)
    check_edge_state(s, slack[1][:16], slack[4][:16], slack[5][:16], slack[6][:16], f"{kind}, slack, 16 rows",
                     field_slack=CONSERVATIVE_SLACK)


# ---- 6: no environment ---------------------------------------------------------------------------------------------------------
def test_no_environment_is_the_primitive_form_without_primitives(problems, scenario, runs, bare):
    """``cloud=None`` without a field, and a cloud with ``counts = 0`` (a saturated field), both give ``gripper_roadmap``
    without primitives, every output bit for bit; a free row is one edge in one round."""
    sp, gp = problems
    for name, got, want in zip(NAMES, runs["free"][0], bare):
        assert same(got, want), name
    cloud = scenario["wall"]["cloud"]
    empty = plan(scenario, sp, gp, "wall", cloud=cloud, counts=torch.zeros(B, dtype=torch.int32, device=dev()), field=None)
    for name, got, want in zip(NAMES, empty, bare):
        assert same(got, want), name
    poses, st, pa, hp, nd, es, rd = runs["free"][1]
    assert (st == 0).all() and (hp == 1).all() and (rd == 1).all()
    f = np.arange(1, W + 1) / W
    for b in range(B):
        line = fg.pose_matrix(fg.edge_pose(nd[b, 0], nd[b, 1], f))
        assert np.abs(poses[b, :, :3].astype(np.float64) - line[:, :3]).max() <= 1e-6


# ---- 7: status 2 ---------------------------------------------------------------------------------------------------------------
def test_bad_endpoints_are_status_2(problems, scenario):
    from mpinets_amd import robot

    sp, gp = (a[:4].copy() for a in problems)
    sp[0, :3, 3] = fg.WALL_CENTRE      # a start inside the wall's cloud
    sp[1, 1, 2] = np.nan               # a NaN entry
    gp[2, 0, 1] = np.inf               # ... and an infinite one, in the goal
    poses, st, pa, hp, nd, es, rd = host(plan(scenario, sp, gp, "wall", rows=slice(0, 4)))
    assert st[:3].tolist() == [2, 2, 2] and st[3] != 2
    assert (rd[:3] == 0).all() and (hp[:3] == 0).all() and (pa[:3] == -1).all() and np.isnan(poses[:3]).all()
    assert es[0, 0, 0] == 2 and es[1, 0, 0] == 2 and es[2, 1, 1] == 2
    assert ((es * (1 - np.eye(V, dtype=np.uint8)))[:3] == 0).all()
    # a start outside the bounds: a box that holds every goal and every other start, but not row 0's start
    sp, gp = (a[:4].copy() for a in problems)
    bounds = np.float32([[0.0, -0.6, 0.0], [0.9, 0.6, 0.9]])
    sp[0, 2, 3] = 0.95
    poses, st, pa, hp, nd, es, rd = host(plan(scenario, sp, gp, "free", bounds=_t(bounds)))
    assert st.tolist() == [2, 0, 0, 0] and rd[0] == 0 and hp[0] == 0 and (pa[0] == -1).all() and np.isnan(poses[0]).all()
    # the body column, with and without the self test (no field: no sphere is read, the self test still runs)
    sp[0, :3, 3] = (0.0, 0.0, 0.2)
    for check_self, want in ((True, 2), (False, 0)):
        poses, st, pa, hp, _, _, rd = host(robot.gripper_roadmap_cloud(_t(sp), _t(gp), None, W=W, seed=SEED, return_graph=True,
                                                                       check_self=check_self))
        assert st.tolist() == [want, 0, 0, 0]
        assert want == 0 or (rd[0] == 0 and hp[0] == 0 and (pa[0] == -1).all() and np.isnan(poses[0]).all())


# ---- 8: smallest shapes --------------------------------------------------------------------------------------------------------
def test_two_nodes_is_the_direct_edge(problems, scenario):
    sp, gp = problems
    for kind, want in (("free", 0), ("wall", 1)):
        poses, st, pa, hp, nd, es, rd = host(plan(scenario, sp, gp, kind, nodes=2))
        assert (st == want).all() and es.shape == (B, 2, 2)
        assert (es[:, 0, 1] == (1 if want == 0 else 2)).all() and (rd == (1 if want == 0 else 2)).all()
        assert np.isnan(poses).all() if want else np.array_equal(poses[:, -1], gp)


def test_256_nodes(problems, scenario, runs):
    sp, gp = problems
    s = scenario["wall"]
    poses, st, pa, hp, nd, es, rd = host(plan(scenario, sp, gp, "wall", nodes=256))
    check_nodes(sp, gp, nd)
    assert np.array_equal(nd[:, :V], runs["wall"][1][4])  # (a node's draw does not depend on V)
    check_search(nd, es, st, pa, hp, rd, MAX_ROUNDS)
    check_poses(s, gp, poses, st, pa, hp, nd, "wall, 256 nodes")
    print(f"wall, 256 nodes: status {np.bincount(st, minlength=3).tolist()}, rounds max {rd.max()}")
    assert (st != 2).all() and (st == 0).any()


@pytest.mark.parametrize("w", (1, 64))
def test_one_and_64_guide_poses(problems, scenario, runs, w):
    sp, gp = problems
    ref = runs["wall"][1]
    poses, st, pa, hp, nd, es, rd = host(plan(scenario, sp, gp, "wall", W=w))
    assert poses.shape == (B, w, 4, 4)
    for got, want in zip((st, pa, hp, nd, es, rd), ref[1:]):  # (the search does not see W)
        assert np.array_equal(got, want)
    check_poses(scenario["wall"], gp, poses, st, pa, hp, nd, f"wall, W = {w}")


def test_one_problem_and_none(problems, scenario, runs):
    from mpinets_amd import robot

    sp, gp = problems
    one = plan(scenario, sp[:1], gp[:1], "wall", rows=slice(0, 1))
    for name, got, want in zip(NAMES, one, runs["wall"][0]):
        assert same(got, want[:1]), name
    s = scenario["wall"]
    for cloud, field in ((None, None), (s["cloud"][:0], sliced(s["field"], slice(0, 0)))):
        none = robot.gripper_roadmap_cloud(_t(sp[:0]), _t(gp[:0]), cloud, field=field, point_radius=PR, W=W, return_graph=True)
        assert [tuple(x.shape) for x in none] == [(0, W, 4, 4), (0,), (0, V), (0,), (0, V, 7), (0, V, V), (0,)]


def test_the_smallest_grid_and_a_grid_that_ends_inside_the_bounds(problems, scenario, runs):
    """A 2 x 2 x 2 grid (one cell of 0.3 m at a corner of the wall: every sample inside it lands in that cell, every other
    centre is outside the grid; a point radius of 0.09 m makes its coarse distances decide -- on the CPU the restatement
    needs 1 to 3 hops and up to 31 rounds there), and the default voxels over y <= 0 only: centres outside count as free and
    read nothing.  The device's verdicts are the float64 ones on the field the device built, and the half grid sees less
    than the whole."""
    from mpinets_amd.field import CloudField

    sp, gp = (a[:16] for a in problems)
    cloud = scenario["wall"]["cloud"][:16]
    trunc = scenario["wall"]["field"].truncation
    cell = CloudField.build(cloud, lo=(0.4, -0.1, 0.4), hi=(0.7, 0.2, 0.7), voxel=0.3, truncation=trunc)
    assert (cell.grid.nx, cell.grid.ny, cell.grid.nz) == (2, 2, 2)
    half = CloudField.build(cloud, lo=(-0.9, -0.9, -0.3), hi=(0.9, 0.0, 1.2), truncation=trunc)
    for what, field, pr in (("2 x 2 x 2", cell, 0.09), ("y <= 0", half, PR)):
        poses, st, pa, hp, nd, es, rd = host(plan(scenario, sp, gp, "wall", cloud=cloud, field=field, point_radius=pr))
        s = dict(values=field.values[0].cpu().numpy(), grid=grid_dict(field.grid))
        print(f"{what}: status 0 / 1 / 2 = {np.bincount(st, minlength=3).tolist()}, hops {np.bincount(hp[st == 0]).tolist()}, "
              f"rounds max {rd.max()}")
        assert rd.max() > 1  # (the field is seen)
        check_search(nd, es, st, pa, hp, rd, MAX_ROUNDS)
        check_edge_state(s, st, nd, es, rd, what, point_radius=pr)
        check_poses(s, gp, poses, st, pa, hp, nd, what, point_radius=pr)
        assert np.array_equal(nd, runs["wall"][1][4][:16])
    assert not np.array_equal(es, runs["wall"][1][5][:16])  # (the half grid does see less)


# ---- 9: sharding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("wall", "free"))
def test_a_shard_computes_the_rows_one_process_computes(problems, scenario, runs, kind):
    sp, gp = problems
    shard = plan(scenario, sp[32:], gp[32:], kind, rows=slice(32, 64), env_offset=32)
    for name, got, want in zip(NAMES, shard, runs[kind][0]):
        assert same(got, want[32:]), name


# ---- 10, 11: the two callers ---------------------------------------------------------------------------------------------------
def env_hit(traj, cloud, point_radius):
    """``check_cloud`` on the refined configurations of traj [N,T,7] (float32, the device's fma) -> bool [N]."""
    from mpinets_amd.robot import FrankaCollisionSampler

    fine = _t(fcp.refine32(traj.cpu().numpy(), 4))
    return FrankaCollisionSampler(dev()).check_cloud(fine, cloud.contiguous(), point_radius=point_radius, clearance=REACH)


def test_make_problem_batch_with_the_gripper_cloud_guide():
    """``hybrid_guide="gripper_cloud"``: the two new keys; the non-hybrid keys equal the "global" run's; ``hybrid_valid`` never
    set where the guide status is != 0 or ``expert_valid`` is false; every ``hybrid_valid`` row free by ``check_cloud`` at
    ``expert_point_radius`` and ending within 5 cm of its last guide pose; at least one valid row.  The counts under both
    guides are printed, not asserted (profiles/gripper_roadmap_cloud_timing.md)."""
    from mpinets_amd import scenes
    from mpinets_amd.robot import franka_fk

    torch.cuda.set_device(0)
    kw = dict(seed=3, collision_free=True, expert=True, expert_from="cloud", hybrid=True, hybrid_against="cloud")
    glob = scenes.make_problem_batch(64, hybrid_guide="global", **kw)
    grip = scenes.make_problem_batch(64, hybrid_guide="gripper_cloud", **kw)
    assert set(grip) - set(glob) == {"hybrid_guide_poses", "hybrid_guide_status"} and not set(glob) - set(grip)
    for k in glob:
        assert k.startswith("hybrid_") or same(glob[k], grip[k]), k  # the guide changes the hybrid keys only
    guide, gst, ok = grip["hybrid_guide_poses"], grip["hybrid_guide_status"], grip["hybrid_valid"]
    assert guide.shape == (64, 8, 4, 4) and gst.shape == (64,) and gst.dtype == torch.int32
    assert torch.isnan(guide[gst != 0]).all() and not torch.isnan(guide[gst == 0]).any()
    assert not (ok & (gst != 0)).any() and not (ok & ~grip["expert_valid"]).any()  # no fall-back between the guides
    print(f"hybrid_valid of 64 against the scene clouds (expert_valid {int(grip['expert_valid'].sum())}): global guide "
          f"{int(glob['hybrid_valid'].sum())}, gripper_cloud guide {int(ok.sum())}; gripper roadmap status 0 / 1 / 2 = "
          f"{torch.bincount(gst, minlength=3).tolist()}")
    assert int(ok.sum()) >= 1
    traj = grip["hybrid_solutions"][ok].contiguous()
    assert not bool(env_hit(traj, grip["xyz"][ok][:, 2048:6144, :3], scenes.EXPERT_CLOUD_POINT_RADIUS).any())
    end = franka_fk(traj[:, -1].contiguous())[:, ft.LINK_ID["right_gripper"], 9:]
    assert float((end - guide[ok][:, -1, :3, 3]).norm(dim=-1).max()) <= 0.05


def test_plan_to_poses_with_the_gripper_guide():
    """``follow=True, follow_guide="gripper"``: the two new keys, every key of the default call on the same inputs unchanged,
    every ``follow_status == 0`` row free by ``check_cloud``; a row without an IK goal has guide status 2."""
    from mpinets_amd import capture, scenes

    torch.cuda.set_device(0)
    n, pr = 8, scenes.EXPERT_CLOUD_POINT_RADIUS
    prob = scenes.make_problem_batch(n, device=dev(), device_clouds=True, seed=4, kinds=("tabletop", "cubby", "dresser"), M1=40,
                                     M2=16, collision_free=True)
    cloud = prob["xyz"][:, 2048:6144, :3]
    base = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4)
    plain = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4, follow=True)
    out = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], point_radius=pr, seed=4, follow=True, follow_guide="gripper")
    assert set(out) - set(plain) == {"follow_guide_poses", "follow_guide_status"} and not set(plain) - set(out)
    for k, v in base.items():
        assert same(v, out[k]), k
    st, gst = out["follow_status"], out["follow_guide_status"]
    print(f"plan_to_poses(follow_guide='gripper'): ik status {out['ik_status'].tolist()}, plan status {out['plan_status'].tolist()}, "
          f"guide status {gst.tolist()}, follow status {st.tolist()} (along the plan: {plain['follow_status'].tolist()})")
    assert out["follow_guide_poses"].shape == (n, 8, 4, 4) and gst.dtype == torch.int32 and gst.shape == (n,)
    assert bool((gst[out["ik_status"] != 0] == 2).all()) and bool((st[gst != 0] == 2).all())
    assert bool(torch.isnan(out["follow_guide_poses"][gst != 0]).all())
    ok = st == 0
    assert bool(torch.isnan(out["followed_trajectory"][~ok]).all())
    if bool(ok.any()):
        traj = out["followed_trajectory"][ok]
        assert not bool(env_hit(traj, cloud[ok], pr).any())
        assert torch.equal(traj[:, 0], prob["q"][ok])
