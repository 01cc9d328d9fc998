"""GPU: ``mpx_gripper_roadmap`` (csrc/gripper_roadmap.hip) and ``make_problem_batch(..., hybrid_guide="gripper")`` against the
float64 restatement (tests/float64_gripper_roadmap.py) and at their edges, on three scenarios of 64 problems (a wall, an upright
cylinder, free space; 64 nodes, 8 guide poses).  One module-scoped fixture per launch: each runs once.

As for the joint roadmap, the search is checked on the DEVICE's own ``nodes`` and ``edge_state`` (every path edge free, the
path's float64 cost that of an independent shortest-path routine over the edges the device did not block), so no test depends
on how float32 breaks a tie between two paths; the verdicts in ``edge_state`` are checked one by one against float64, outside
``GRIPPER_BAND`` (tests/test_gripper_roadmap_host.py derives it, and holds the restatement to the left-out cap at this seed)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_gripper_roadmap as fg  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_plan import dev, judge  # noqa: E402
from test_gripper_roadmap_host import FOUND_SHARE, GRIPPER_BAND, LEFT_OUT_CAP  # noqa: E402

pytestmark = pytest.mark.gpu

B, V, W = 64, 64, 8
SEED = fg.ROADMAP_SEED
MAX_ROUNDS = fg.DEFAULTS["max_rounds"]
KINDS = ("wall", "cylinder", "free")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same(a, b):
    """torch.equal with NaN equal to NaN; a non-tensor by ==."""
    if not torch.is_tensor(a):
        return a == b
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def prims(kind, rows=slice(None)):
    """-> (TorchCuboids or None, TorchCylinders or None, the restatement's scene from the DEVICE's inverse frames)."""
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    arrays = fg.scene_arrays(B, kind)
    if arrays is None:
        return None, None, None
    t = {k: _t(v[rows]) for k, v in arrays.items()}
    n = len(next(iter(t.values())))
    scene = {"cub_frames": np.zeros((n, 0, 4, 4), np.float32), "cub_dims": np.zeros((n, 0, 3), np.float32),
             "cyl_frames": np.zeros((n, 0, 4, 4), np.float32), "cyl_radii": np.zeros((n, 0), np.float32),
             "cyl_heights": np.zeros((n, 0), np.float32)}
    cub = cyl = None
    if kind == "wall":
        cub = TorchCuboids(t["cuboid_centers"], t["cuboid_dims"], t["cuboid_quats"])
        scene.update(cub_frames=cub.inv_frames.cpu().numpy(), cub_dims=cub.dims.cpu().numpy())
    else:
        cyl = TorchCylinders(t["cylinder_centers"], t["cylinder_radii"], t["cylinder_heights"], t["cylinder_quats"])
        scene.update(cyl_frames=cyl.inv_frames.cpu().numpy(), cyl_radii=cyl.radii.reshape(n, -1).cpu().numpy(),
                     cyl_heights=cyl.heights.reshape(n, -1).cpu().numpy())
    return cub, cyl, scene


def plan(sp, gp, kind, rows=slice(None), **kw):
    from mpinets_amd import robot

    cub, cyl, _ = prims(kind, rows)
    kw.setdefault("seed", SEED)
    return robot.gripper_roadmap(_t(sp), _t(gp), cub, cyl, W=kw.pop("W", W), return_graph=True, **kw)


@pytest.fixture(scope="module")
def problems():
    torch.cuda.set_device(0)
    return fg.problems(B)


@pytest.fixture(scope="module")
def runs(problems):
    """kind -> (scene, the seven outputs as tensors, the same as numpy): one launch per scenario."""
    sp, gp = problems
    out = {}
    for kind in KINDS:
        res = plan(sp, gp, kind)
        out[kind] = (prims(kind)[2], res, tuple(x.cpu().numpy() for x in res))
    return out


# ---- the checks, on numpy outputs (so that they can be run against the restatement's own outputs too) ----------------------------
def check_nodes(sp, gp, nodes, seed=SEED, env_offset=0, bounds=None):
    bounds = fg.default_bounds(sp, gp) if bounds is None else bounds
    want, ok = fg.draw_nodes(sp, gp, bounds, nodes.shape[1], seed, env_offset)
    assert ok.all()
    assert np.array_equal(nodes[:, 2:, :3], want[:, 2:, :3])  # bit for bit
    assert np.abs(nodes[..., 3:].astype(np.float64) - want[..., 3:]).max() <= 2.0 ** -22
    assert np.abs(np.linalg.norm(nodes[..., 3:].astype(np.float64), axis=-1) - 1).max() <= 2.0 ** -22
    assert np.array_equal(nodes[:, 0, :3], sp[:, :3, 3]) and np.array_equal(nodes[:, 1, :3], gp[:, :3, 3])
    R = fg.rotation(nodes[:, :2, 3:].astype(np.float64))
    assert np.abs(R - np.stack([sp, gp], 1)[:, :, :3, :3]).max() <= 1e-6


def check_edge_state(scene, st, nodes, es, rounds, what):
    n, v = es.shape[:2]
    assert np.array_equal(es, es.transpose(0, 2, 1)) and es.max() <= 2
    off = es * (1 - np.eye(v, dtype=np.uint8))
    assert (off[st == 2] == 0).all() and (rounds[st == 2] == 0).all()
    left, wrong, tested = 0, [], 0
    for b in range(n):
        sc = None if scene is None else {k: a[b:b + 1] for k, a in scene.items()}
        want, in_band, _ = fg.graph_verdicts(nodes[b], np.ones(v, bool), es[b], sc, GRIPPER_BAND)
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


def check_search(nd, es, st, pa, hp, rd, max_rounds, connect_radius=float("inf")):
    for b in range(len(st)):
        cost = fg.dijkstra_cost(nd[b], es[b], connect_radius=connect_radius)
        if st[b] == 0:
            p = pa[b, :hp[b] + 1]
            assert p[0] == 0 and p[-1] == 1 and (pa[b, hp[b] + 1:] == -1).all() and len(set(p.tolist())) == len(p)
            assert all(es[b, u, v] == fg.FREE for u, v in zip(p[:-1], p[1:])), b
            assert abs(fg.path_cost(nd[b], p) - cost) <= len(nd[b]) * 2.0 ** -23 * cost, b
            assert 1 <= rd[b] <= max_rounds
        else:
            assert hp[b] == 0 and (pa[b] == -1).all()
            if st[b] == 1:
                assert not np.isfinite(cost) or rd[b] == max_rounds, b


def check_poses(scene, gp, poses, st, pa, hp, nd, what):
    found = st == 0
    assert np.isnan(poses[~found]).all() and (pa[~found] == -1).all() and (hp[~found] == 0).all()
    assert np.array_equal(poses[found][:, -1], gp[found])  # the goal as given
    R = poses[found][:, :, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 1, 3, 2) - np.eye(3)).max() <= 1e-6
    assert np.array_equal(poses[found][:, :, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), poses[found][:, :, 3].shape))
    worst_p = worst_r = 0.0
    low = np.inf
    for b in np.flatnonzero(found):
        want = fg.resample(nd[b], pa[b, :hp[b] + 1], poses.shape[1])
        worst_p = max(worst_p, float(np.abs(poses[b, :-1, :3, 3] - want[:-1, :3, 3]).max(initial=0.0)))
        worst_r = max(worst_r, float(np.abs(poses[b, :-1, :3, :3] - want[:-1, :3, :3]).max(initial=0.0)))
        sc = None if scene is None else {k: a[b:b + 1] for k, a in scene.items()}
        low = min(low, float(fg.margins(fg.pose_nodes(poses[b].astype(np.float64)), sc).min()))
    print(f"{what}: poses against the float64 resampling of the device's own path, position {worst_p:.3e} m, rotation entries "
          f"{worst_r:.3e}; smallest float64 margin of a guide pose {low:.3e} m")
    assert worst_p <= 2e-6 and worst_r <= 2e-6
    assert low > -GRIPPER_BAND  # every pose valid in float64, outside the band


# ---- 1 - 6 on the three scenarios ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nodes_are_the_restatements_draws(problems, runs, kind):
    """Positions bit-equal to the float32 restatement of the Philox draw (stream 17), quaternions within 2^-22 of it and of
    unit norm; nodes 0 / 1 reproduce the input rotations within 1e-6 and the positions exactly."""
    check_nodes(*problems, runs[kind][2][4])


@pytest.mark.parametrize("kind", KINDS)
def test_edge_state_against_float64(runs, kind):
    scene, _, (poses, st, pa, hp, nd, es, rd) = runs[kind]
    check_edge_state(scene, st, nd, es, rd, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_search_invariant_on_the_devices_own_edge_state(runs, kind):
    scene, _, (poses, st, pa, hp, nd, es, rd) = runs[kind]
    check_search(nd, es, st, pa, hp, rd, MAX_ROUNDS)
    print(f"{kind}: status 0 / 1 / 2 = {np.bincount(st, minlength=3).tolist()}, hops histogram {np.bincount(hp[st == 0]).tolist()}, "
          f"rounds histogram {np.bincount(rd).tolist()}")


def test_rounds_run_out_and_a_search_within_the_budget_does_not_see_it(problems, runs):
    sp, gp = problems
    _, _, (poses, st, pa, hp, nd, es, rd) = runs["wall"]
    s_poses, s_st, s_pa, s_hp, s_nd, s_es, s_rd = (x.cpu().numpy() for x in plan(sp, gp, "wall", max_rounds=3))
    check_search(s_nd, s_es, s_st, s_pa, s_hp, s_rd, 3)
    ran_out = (s_st == 1) & (s_rd == 3)
    assert ran_out.sum() >= 4 and (st[ran_out] != 2).all()
    same = s_rd <= 2
    assert np.array_equal(s_pa[same & (s_st == 0)], pa[same & (s_st == 0)])
    assert np.array_equal(s_nd, nd)
    assert np.isnan(s_poses[s_st != 0]).all() and not np.isnan(s_poses[s_st == 0]).any()


@pytest.mark.parametrize("kind", ("wall", "cylinder"))
def test_the_obstacle_is_gone_round(runs, kind):
    """Every found path has at least two edges, and at least 90 % of the rows find one (the restatement does at this seed:
    tests/test_gripper_roadmap_host.py)."""
    _, _, (poses, st, pa, hp, nd, es, rd) = runs[kind]
    assert (hp[st == 0] >= 2).all()
    print(f"{kind}: {int((st == 0).sum())} of {len(st)} rows found a path; out of rounds {int(((st == 1) & (rd == MAX_ROUNDS)).sum())}")
    assert (st == 0).mean() >= FOUND_SHARE


def test_free_space_is_one_edge(problems, runs):
    sp, gp = problems
    _, _, (poses, st, pa, hp, nd, es, rd) = runs["free"]
    assert (st == 0).all() and (hp == 1).all() and (rd == 1).all()
    f = np.arange(1, W + 1) / W
    for b in range(B):
        line = fg.pose_matrix(fg.edge_pose(nd[b, 0], nd[b, 1], f))
        assert np.abs(poses[b, :, :3].astype(np.float64) - line[:, :3]).max() <= 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_poses(problems, runs, kind):
    """The last pose is the goal bit for bit, rotations orthonormal within 1e-6, every pose valid in float64 outside the band,
    positions within 2e-6 of the float64 resampling of the device's own path and nodes; rows without a path are NaN."""
    scene, (t_poses, t_st, *_), (poses, st, pa, hp, nd, es, rd) = runs[kind]
    check_poses(scene, problems[1], poses, st, pa, hp, nd, kind)
    assert torch.equal(t_poses[t_st == 0][:, -1], _t(problems[1])[t_st == 0])


# ---- 7: status 2 ---------------------------------------------------------------------------------------------------------------
def test_bad_endpoints_are_status_2(problems):
    from mpinets_amd import robot

    sp, gp = (a[:4].copy() for a in problems)
    sp[0, :3, 3] = fg.WALL_CENTRE      # a start inside the wall
    sp[1, 1, 2] = np.nan               # a NaN entry
    gp[2, 0, 1] = np.inf               # ... and an infinite one, in the goal
    poses, st, pa, hp, nd, es, rd = (x.cpu().numpy() for x in plan(sp, gp, "wall", rows=slice(0, 4)))
    assert st[:3].tolist() == [2, 2, 2] and st[3] != 2
    assert (rd[:3] == 0).all() and (hp[:3] == 0).all() and (pa[:3] == -1).all() and np.isnan(poses[:3]).all()
    assert es[0, 0, 0] == 2 and es[1, 0, 0] == 2 and es[2, 1, 1] == 2
    assert ((es * (1 - np.eye(V, dtype=np.uint8)))[:3] == 0).all()
    # a start outside the bounds: a box that holds every goal and every other start, but not row 0's start
    sp, gp = (a[:4].copy() for a in problems)
    bounds = np.float32([[0.0, -0.6, 0.0], [0.9, 0.6, 0.9]])
    sp[0, 2, 3] = 0.95
    _, st, *_ = plan(sp, gp, "free", bounds=_t(bounds))
    assert st.cpu().tolist() == [2, 0, 0, 0]
    # the body column, with and without the self test (free space: no sphere table is passed, the self test still runs)
    sp[0, :3, 3] = (0.0, 0.0, 0.2)
    for check_self, want in ((True, 2), (False, 0)):
        _, st, *_ = robot.gripper_roadmap(_t(sp), _t(gp), W=W, seed=SEED, check_self=check_self)
        assert st.cpu().tolist() == [want, 0, 0, 0]


# ---- 8: shape edges ------------------------------------------------------------------------------------------------------------
def test_two_nodes_is_the_direct_edge(problems):
    sp, gp = problems
    for kind, want in (("free", 0), ("wall", 1)):
        poses, st, pa, hp, nd, es, rd = (x.cpu().numpy() for x in plan(sp, gp, kind, nodes=2))
        assert (st == want).all() and es.shape == (B, 2, 2)
        assert (es[:, 0, 1] == (1 if want == 0 else 2)).all() and (rd == (1 if want == 0 else 2)).all()
        assert np.isnan(poses).all() if want else np.array_equal(poses[:, -1], gp)


def test_256_nodes(problems, runs):
    sp, gp = problems
    scene = runs["wall"][0]
    poses, st, pa, hp, nd, es, rd = (x.cpu().numpy() for x in plan(sp, gp, "wall", nodes=256))
    check_nodes(sp, gp, nd)
    assert np.array_equal(nd[:, :V], runs["wall"][2][4])  # (a node's draw does not depend on V)
    check_search(nd, es, st, pa, hp, rd, MAX_ROUNDS)
    check_poses(scene, gp, poses, st, pa, hp, nd, "wall, 256 nodes")
    check_edge_state({k: a[:16] for k, a in scene.items()}, st[:16], nd[:16], es[:16], rd[:16], "wall, 256 nodes, 16 rows")
    # (recorded, not a floor: with four times the nodes there are more near-wall paths to refute, and rows run out of the
    # 256 rounds that 64 nodes stay below -- 56 found, 8 out of rounds: profiles/gripper_roadmap_timing.md)
    print(f"wall, 256 nodes: status {np.bincount(st, minlength=3).tolist()}, rounds max {rd.max()}")
    assert (st != 2).all() and (st == 0).any()


@pytest.mark.parametrize("w", (1, 64))
def test_one_and_64_guide_poses(problems, runs, w):
    sp, gp = problems
    scene, _, ref = runs["wall"]
    poses, st, pa, hp, nd, es, rd = (x.cpu().numpy() for x in plan(sp, gp, "wall", W=w))
    assert poses.shape == (B, w, 4, 4)
    for got, want in zip((st, pa, hp, nd, es, rd), ref[1:]):  # (the search does not see W)
        assert np.array_equal(got, want)
    check_poses(scene, gp, poses, st, pa, hp, nd, f"wall, W = {w}")


def test_one_problem(problems, runs):
    sp, gp = problems
    one = plan(sp[:1], gp[:1], "wall", rows=slice(0, 1))
    for got, want in zip(one, runs["wall"][1]):
        assert same(got, want[:1])
    from mpinets_amd import robot

    none = robot.gripper_roadmap(_t(sp[:0]), _t(gp[:0]), W=W, return_graph=True)
    assert [tuple(x.shape) for x in none] == [(0, W, 4, 4), (0,), (0, V), (0,), (0, V, 7), (0, V, V), (0,)]


def test_connect_radius_below_the_direct_edge(problems, runs):
    sp, gp = problems
    nd = runs["free"][2][4]
    direct = np.array([fg.lengths(nd[b, :2], dtype=np.float32)[0, 1] for b in range(B)])
    radius = float(direct.min()) * 0.75
    poses, st, pa, hp, nd2, es, rd = (x.cpu().numpy() for x in plan(sp, gp, "free", connect_radius=radius))
    assert np.array_equal(nd2, nd)
    check_search(nd2, es, st, pa, hp, rd, MAX_ROUNDS, connect_radius=radius)
    assert (hp[st == 0] >= 2).all() and (st != 2).all() and (st == 0).sum() >= B // 2
    for b in np.flatnonzero(st == 0):
        p = pa[b, :hp[b] + 1]
        w = fg.lengths(nd2[b][p], dtype=np.float32)
        assert all(w[i, i + 1] <= np.float32(radius) for i in range(hp[b]))


# ---- 9: sharding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("wall", "free"))
def test_a_shard_computes_the_rows_one_process_computes(problems, runs, kind):
    sp, gp = problems
    shard = plan(sp[32:], gp[32:], kind, rows=slice(32, 64), env_offset=32)
    for got, want in zip(shard, runs[kind][1]):
        assert same(got, want[32:])


# ---- 10: closing the loop ------------------------------------------------------------------------------------------------------
def test_make_problem_batch_with_the_gripper_guide():
    """``hybrid_guide="gripper"``: the new keys; every ``hybrid_valid`` row passes the judges that predate the planner and ends
    within 5 cm of the last guide pose; omitting the keyword and passing "global" give one and the same dict, without the
    new keys.  ``hybrid_valid`` under both guides is printed, not asserted (profiles/gripper_roadmap_timing.md)."""
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders
    from mpinets_amd.robot import franka_fk
    from mpinets_amd.scenes import make_problem_batch

    torch.cuda.set_device(0)
    kw = dict(seed=3, collision_free=True, expert=True, hybrid=True)
    plain, glob, grip = make_problem_batch(64, **kw), make_problem_batch(64, hybrid_guide="global", **kw), \
        make_problem_batch(64, hybrid_guide="gripper", **kw)
    assert plain.keys() == glob.keys() and set(grip) - set(plain) == {"hybrid_guide_poses", "hybrid_guide_status"}
    for k in plain:
        assert same(plain[k], glob[k]), k
        assert k.startswith("hybrid_") or same(plain[k], grip[k]), k  # the guide changes the hybrid keys only
    with pytest.raises(ValueError):
        make_problem_batch(4, hybrid_guide="roadmap", **kw)
    guide, gst, ok = grip["hybrid_guide_poses"], grip["hybrid_guide_status"], grip["hybrid_valid"]
    assert guide.shape == (64, 8, 4, 4) and gst.shape == (64,) and gst.dtype == torch.int32
    assert torch.isnan(guide[gst != 0]).all() and not torch.isnan(guide[gst == 0]).any()
    assert not (ok & (gst != 0)).any() and not (ok & ~grip["expert_valid"]).any()  # no fall-back between the guides
    print(f"hybrid_valid of 64 (expert_valid {int(grip['expert_valid'].sum())}): global guide {int(plain['hybrid_valid'].sum())}, "
          f"gripper guide {int(ok.sum())}; gripper roadmap status 0 / 1 / 2 = {torch.bincount(gst, minlength=3).tolist()}")
    assert int(ok.sum()) >= 1
    cub = TorchCuboids(grip["cuboid_centers"][ok], grip["cuboid_dims"][ok], grip["cuboid_quats"][ok])
    cyl = TorchCylinders(grip["cylinder_centers"][ok], grip["cylinder_radii"][ok], grip["cylinder_heights"][ok],
                         grip["cylinder_quats"][ok])
    traj = grip["hybrid_solutions"][ok].contiguous()
    # (``judge``'s fourth flag tests the PUBLISHED joint limits; ``make_problem_batch`` runs its solvers inside the measured
    # ones, which are wider on some joints: tests/test_gpu_follow.py's ``judged_valid`` leaves it out for the same reason)
    env, self_hit, jerk, _ = judge(traj, cub, cyl)
    assert not env.any() and not self_hit.any() and float(jerk.max()) <= 0.15
    end = franka_fk(traj[:, -1].contiguous())[:, ft.LINK_ID["right_gripper"], 9:]
    assert float((end - guide[ok][:, -1, :3, 3]).norm(dim=-1).max()) <= 0.05
