"""CPU: ``mpx_gripper_roadmap`` refuses bad arguments on the host, before any launch; its kernel uses no scratch; the float64
restatement (tests/float64_gripper_roadmap.py) stands on its own -- the draws' keying, the gripper's spheres against the arm's
own, the lazy search against an independent shortest-path routine -- and, run as a planner on the wall and cylinder scenarios
of tests/test_gpu_gripper_roadmap.py with Philox draws, finds a path on at least 90 % of the rows.  The band of the GPU
edge-state comparison and the cap of its left-out problems are derived here, at the seed the GPU tests use (chosen on the
CPU, before any device run)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_gripper_roadmap as fg  # noqa: E402
import float64_plan as fp  # noqa: E402
import float64_roadmap as fr  # noqa: E402
from float64_collision import SDF_BAR  # noqa: E402  (the band of a primitive SDF in float32 against float64, metres)

from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd import scenes  # noqa: E402
from oracle import oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEFT_OUT_CAP = 0.10  # share of the problems that may have a deciding pose inside the band
FOUND_SHARE = 0.90   # share of the wall / cylinder rows that must end with a path
# float32 against float64 placement of the gripper's sphere centres over every tested pose of the two scenarios (the
# restatement's own graphs at ROADMAP_SEED; recorded by test_band_and_left_out_share): 4.8e-8 m
PLACEMENT_REFERENCE = 4.8e-8
GRIPPER_BAND = SDF_BAR + 4 * PLACEMENT_REFERENCE  # 1.09e-6 m: what a float32 verdict may differ by from the float64 one

# ---- refusals ------------------------------------------------------------------------------------------------------------------
GOOD = dict(nodes=64, resolution=0.01, rot_weight=0.12, orient_spread=0.5, connect_radius=float("inf"), max_rounds=8,
            check_margin=1e-4, clearance=0.0, check_self=1)


def _call(lib, B=4, W=8, S=0, M1=0, opts=None, env_offset=0, poses=256, status=256, path=256, hops=256, sp=256, gp=256, bounds=256):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731  (any non-NULL "device pointer": refused before it is touched)
    sph, cub = p(256 if S else 0), p(256 if M1 else 0)
    return lib.mpx_gripper_roadmap(p(sp), p(gp), B, W, p(bounds), 0.025, sph, sph, sph, S, cub, cub, M1, None, None, None, 0,
                                   None if opts is None else ctypes.byref(opts), 0, env_offset, p(poses), p(status), p(path),
                                   p(hops), None, None, None, None)


def test_gripper_roadmap_refuses_bad_arguments_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    opt = lambda **kw: _lib.GripperRoadmapOptions(**dict(GOOD, **kw))  # noqa: E731
    for V in (-1, 0, 1, 257):
        assert _call(lib, opts=opt(nodes=V)) != 0 and b"nodes" in lib.mpx_last_error()
    for W in (-1, 0, 65):
        assert _call(lib, W=W) != 0 and b"guide poses" in lib.mpx_last_error()
    for res in (0.0, -0.01, float("nan")):
        assert _call(lib, opts=opt(resolution=res)) != 0 and b"resolution" in lib.mpx_last_error()
    for rw in (0.0, -0.12, float("nan"), float("inf")):
        assert _call(lib, opts=opt(rot_weight=rw)) != 0 and b"rot_weight" in lib.mpx_last_error()
    for sp in (-0.5, float("nan")):
        assert _call(lib, opts=opt(orient_spread=sp)) != 0 and b"orient_spread" in lib.mpx_last_error()
    assert _call(lib, opts=opt(connect_radius=float("nan"))) != 0 and b"connect_radius" in lib.mpx_last_error()
    assert _call(lib, opts=opt(max_rounds=0)) != 0 and b"max_rounds" in lib.mpx_last_error()
    assert _call(lib, opts=opt(check_margin=-1e-4)) != 0 and b"check_margin" in lib.mpx_last_error()
    assert _call(lib, opts=opt(clearance=float("nan"))) != 0 and b"clearance" in lib.mpx_last_error()
    for out in ("poses", "status", "path", "hops"):
        assert _call(lib, **{out: 0}) != 0 and b"NULL output" in lib.mpx_last_error()
    for operand in ("sp", "gp", "bounds"):
        assert _call(lib, **{operand: 0}) != 0 and b"NULL operand" in lib.mpx_last_error()
    assert _call(lib, B=-1) != 0 and b"negative size" in lib.mpx_last_error()
    assert _call(lib, S=-1) != 0 and b"negative size" in lib.mpx_last_error()
    assert _call(lib, S=65) != 0 and b"65" in lib.mpx_last_error()
    assert _call(lib, M1=65, S=56) != 0 and b"64 cuboids" in lib.mpx_last_error()
    assert _call(lib, M1=4, S=0) != 0 and b"without collision spheres" in lib.mpx_last_error()
    assert _call(lib, env_offset=-1) != 0 and b"env_offset" in lib.mpx_last_error()
    assert _call(lib, env_offset=(1 << 32)) != 0 and b"env_offset" in lib.mpx_last_error()
    assert b"mpx_gripper_roadmap" in lib.mpx_last_error()
    # nothing to do, nothing touched; a bad option is refused even then
    assert _call(lib, B=0, poses=0, status=0, path=0, hops=0, sp=0, gp=0, bounds=0) == 0
    assert _call(lib, B=0, opts=opt(nodes=1)) != 0


def test_python_entry_point_and_defaults_are_one_set():
    import inspect

    from mpinets_amd import _lib, robot, solvers

    M = torch.eye(4).expand(2, 4, 4)
    with pytest.raises(_lib.MpxError):
        robot.gripper_roadmap(M, M)  # (CPU tensors)
    assert robot.gripper_roadmap is solvers.gripper_roadmap
    sig = inspect.signature(robot.gripper_roadmap).parameters
    assert sig["W"].default == 8 and sig["bounds"].default is None and sig["return_graph"].default is False
    with pytest.raises(TypeError):
        robot._gripper_roadmap_options("gripper_roadmap", {"node": 3})
    assert robot.GRIPPER_ROADMAP_DEFAULTS == fg.DEFAULTS and robot.GRIPPER_ROADMAP_BOUNDS_PAD == fg.BOUNDS_PAD == 0.3
    assert [n for n, _ in _lib.GripperRoadmapOptions._fields_] == list(fg.DEFAULTS)
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    for key in ("nodes", "resolution", "rot_weight", "orient_spread", "max_rounds"):
        m = re.search(r"#define MPX_GRIPPER_ROADMAP_DEFAULT_%s\s+([0-9.e+-]+)f?" % key.upper(), text)
        assert m and float(m.group(1)) == pytest.approx(float(fg.DEFAULTS[key]), rel=1e-6), key
    assert fg.DEFAULTS["check_margin"] == fp.DEFAULTS["check_margin"]
    assert inspect.signature(scenes.make_problem_batch).parameters["hybrid_guide"].default == "global"
    assert _lib.load().mpx_version() == 341


def test_gripper_roadmap_kernel_uses_no_scratch():
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "gripper_roadmap_kernel" in n}
    assert len(hits) == 1
    (f,) = hits.values()
    print({k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
def _fk_poses(q):
    R, t = orc.fk_frames_torch(torch.from_numpy(np.asarray(q, np.float64)))
    M = np.tile(np.eye(4), (len(q), 1, 1))
    M[:, :3, :3], M[:, :3, 3] = R[:, 14].numpy(), t[:, 14].numpy()
    return M


def test_draws_are_keyed_by_the_global_problem_id():
    sp, gp = fg.problems(40)
    bounds = fg.default_bounds(sp, gp)
    a, ok = fg.draw_nodes(sp, gp, bounds, V=64, seed=3)
    b, _ = fg.draw_nodes(sp[15:], gp[15:], bounds[15:], V=64, seed=3, env_offset=15)
    assert a.dtype == np.float32 and np.array_equal(a[15:], b) and ok.all()
    assert np.array_equal(a[:, 0, :3], sp[:, :3, 3]) and np.array_equal(a[:, 1, :3], gp[:, :3, 3])
    other, _ = fg.draw_nodes(sp, gp, bounds, V=64, seed=4)
    assert np.array_equal(a[:, :2], other[:, :2]) and not np.array_equal(a[:, 2:], other[:, 2:])
    assert np.array_equal(fg.draw_nodes(sp, gp, bounds, V=16, seed=3)[0], a[:, :16])  # (a node's draw does not depend on V)
    assert ((a[:, 2:, :3] >= bounds[:, None, 0]) & (a[:, 2:, :3] <= bounds[:, None, 1])).all()
    assert np.abs(np.linalg.norm(a[..., 3:].astype(np.float64), axis=-1) - 1).max() <= 2.0 ** -22
    assert len(np.unique(a[:, 2:].reshape(-1))) > 0.99 * a[:, 2:].size  # (seven different words per node)
    # orient_spread = 0: every drawn orientation lies on the start-goal arc (the normalised chord)
    on, _ = fg.draw_nodes(sp, gp, bounds, V=8, seed=3, orient_spread=0.0)
    qs, qg = on[:, 0, 3:].astype(np.float64), on[:, 1, 3:].astype(np.float64)
    qg = qg * np.where((qs * qg).sum(-1) >= 0, 1, -1)[:, None]
    for v in range(2, 8):
        q = on[:, v, 3:].astype(np.float64)
        coef = np.linalg.lstsq(np.stack([qs[0], qg[0]], 1), q[0], rcond=None)
        assert np.abs(np.stack([qs[0], qg[0]], 1) @ coef[0] - q[0]).max() < 1e-6
    # the endpoints reproduce the input rotations
    assert np.abs(fg.rotation(a[:, :2, 3:].astype(np.float64)) - np.stack([sp, gp], 1)[:, :, :3, :3]).max() < 1e-6


def test_shepperd_takes_every_branch():
    """Half turns about x, y and z leave the trace branch; the quaternion reproduces the matrix in each."""
    M = np.tile(np.eye(4, dtype=np.float32), (4, 1, 1))
    M[1, :3, :3], M[2, :3, :3], M[3, :3, :3] = np.diag([1, -1, -1]), np.diag([-1, 1, -1]), np.diag([-1, -1, 1])
    for dt in (np.float64, np.float32):
        n = fg.pose_nodes(M, dt)
        assert np.array_equal(np.abs(n[:, 3:]).argmax(-1), [3, 0, 1, 2])
        assert np.abs(fg.rotation(n[:, 3:]) - M[:, :3, :3]).max() < 1e-6


def test_gripper_spheres_are_the_arms_own():
    """The spheres of links 9 / 12 / 13 placed from the pose FK(q) against ``float64_plan.sphere_centres`` of q itself, and
    the three frame origins against the chain's."""
    q = scenes.random_configurations(64, 11).astype(np.float64)
    x, _, t, radii, link = fp.sphere_centres(torch.from_numpy(q))
    pts, r, rows, origins = fg.gripper_points()
    assert len(rows) == 20 and set(link[rows].tolist()) == {9, 12, 13}
    nodes = fg.pose_nodes(_fk_poses(q))  # (Shepperd in float64 on the float64 matrices)
    assert np.abs(fg.place(nodes, pts) - x[:, rows].numpy()).max() < 1e-12
    assert np.abs(fg.place(nodes, origins) - t[:, list(fg.GRIPPER_LINKS)].numpy()).max() < 1e-12
    assert np.array_equal(r, radii[rows].numpy())
    lever = np.linalg.norm(pts, axis=-1).max()
    assert 0.117 < lever < 0.1175 and lever <= fg.DEFAULTS["rot_weight"]  # (the header's 0.1172 m)


def _toy(seed, V=48):
    """A planar toy: start and goal left and right of a disc in the x-y plane, one orientation, V - 2 uniform nodes."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros((V, 7), np.float32)
    nodes[:, 6] = 1
    nodes[:, :2] = rng.uniform(-1, 1, size=(V, 2))
    nodes[0, :2], nodes[1, :2] = (-0.9, 0.05 * seed), (0.9, -0.03 * seed)
    centre, radius = np.float64([0.05, 0.0]), 0.45

    def is_valid(p):
        return np.linalg.norm(np.asarray(p, np.float64)[:, :2] - centre, axis=-1) > radius
    return nodes, is_valid


@pytest.mark.parametrize("seed", range(4))
def test_lazy_search_ends_with_the_shortest_path_among_edges_not_blocked(seed):
    nodes, is_valid = _toy(seed)
    ok = np.ones(len(nodes), bool)
    st, path, state, rounds = fg.search(nodes, ok, is_valid, resolution=0.02, max_rounds=200)
    assert st == 0 and path[0] == 0 and path[-1] == 1 and len(path) >= 3 and rounds >= 2  # (the disc blocks the direct edge)
    assert state[0, 1] == fg.BLOCKED and np.array_equal(state, state.T)
    assert all(state[u, v] == fg.FREE for u, v in zip(path[:-1], path[1:]))
    assert fg.path_cost(nodes, path) == pytest.approx(fg.dijkstra_cost(nodes, state), rel=1e-12)
    # with one orientation the metric is the distance: the joint roadmap's routine agrees on the cost
    assert fg.path_cost(nodes, path) == pytest.approx(fr.path_cost(nodes, path), rel=1e-12)
    assert fg.search(nodes, ok, is_valid, resolution=0.02, max_rounds=rounds - 1)[0] == 1
    assert fg.search(nodes, ok, is_valid, resolution=0.02, connect_radius=0.05)[0] == 1
    bad = ok.copy()
    bad[1] = False
    assert fg.search(nodes, bad, is_valid)[0] == 2


def test_metric_is_symmetric_and_counts_the_angle():
    sp, gp = fg.problems(4)
    nodes, _ = fg.draw_nodes(sp, gp, fg.default_bounds(sp, gp), V=32, seed=1)
    for dt in (np.float32, np.float64):
        Wm = fg.lengths(nodes[0], 0.12, dt)
        assert np.array_equal(Wm, Wm.T) and (np.diag(Wm) == 0).all()
    # same position, a rotation by theta about z: w = rot_weight x 4 sin(theta / 4)
    th = 0.7
    a = np.float32([0, 0, 0, 0, 0, 0, 1])
    b = np.float32([0, 0, 0, 0, 0, np.sin(th / 2), np.cos(th / 2)])
    w = fg.lengths(np.stack([a, b, -b]), 0.12)
    assert w[0, 1] == pytest.approx(0.12 * 4 * np.sin(th / 4), rel=1e-6) and w[0, 2] == pytest.approx(w[0, 1], rel=1e-12)
    assert fg.pieces(0.0, 0.01) == 1 and fg.pieces(0.0301, 0.01) == 4 and fg.pieces(1e9, 0.01) == fg.MAX_PIECES
    mid = fg.edge_pose(a, -b, [0.5])[0]  # (nlerp takes the short way: toward sigma q_b)
    assert np.abs(mid[3:] - [0, 0, np.sin(th / 4), np.cos(th / 4)]).max() < 1e-7


# ---- the restatement as a planner on the GPU tests' scenarios -------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    B = 64
    sp, gp = fg.problems(B)
    out = {}
    for kind in ("wall", "cylinder"):
        scene = fg.scene_of(fg.scene_arrays(B, kind), B)
        out[kind] = (scene, fg.solve(sp, gp, scene, seed=fg.ROADMAP_SEED))
    return sp, gp, out


def test_restatement_finds_a_way_round_with_philox_draws(planned):
    """Float64, the default options (64 nodes, 256 rounds), Philox draws at ROADMAP_SEED.  Measured: wall 64 of 64 (hops
    2 / 3 / 4: 22 / 40 / 2; rounds at most 192, mean 59), cylinder 64 of 64 (hops 2 / 3: 48 / 16; rounds at most 41, mean 12)."""
    sp, gp, out = planned
    for kind, (scene, (poses, st, path, hops, nodes, es, rounds)) in out.items():
        found = st == 0
        print(f"{kind}: status 0 / 1 / 2 {np.bincount(st, minlength=3).tolist()}, hops histogram {np.bincount(hops[found]).tolist()}, "
              f"rounds max {rounds.max()} mean {rounds.mean():.1f}, out of rounds {int(((st == 1) & (rounds == 256)).sum())}")
        assert found.mean() >= FOUND_SHARE
        assert (hops[found] >= 2).all()  # (the obstacle sits between every start and its goal)
        assert np.isnan(poses[~found]).all() and (path[~found] == -1).all()
        assert np.array_equal(poses[found][:, -1, :3], gp[found][:, :3].astype(np.float64))
        for b in np.flatnonzero(found)[:8]:  # every guide pose is valid, the path costs what Dijkstra says
            sc = {k: v[b:b + 1] for k, v in scene.items()}
            assert (fg.margins(fg.pose_nodes(poses[b].astype(np.float32)), sc) > -1e-6).all()
            p = path[b, :hops[b] + 1]
            assert fg.path_cost(nodes[b], p) == pytest.approx(fg.dijkstra_cost(nodes[b], es[b]), rel=1e-12)


def test_band_and_left_out_share(planned):
    """``GRIPPER_BAND`` = SDF_BAR + 4 x the largest float32-against-float64 difference of a placed sphere centre over every
    tested pose of the two scenarios; the share of problems with a deciding pose inside that band stays below LEFT_OUT_CAP
    for the restatement alone, and its graph agrees with the verdicts recomputed from the float32 poses everywhere else.
    Measured: placement 4.8e-8 m, 0 of 64 left out on either scenario."""
    sp, gp, out = planned
    pts32, pts64 = fg.gripper_points(dtype=np.float32)[0], fg.gripper_points()[0]
    worst = 0.0
    for kind, (scene, (poses, st, path, hops, nodes, es, rounds)) in out.items():
        left = wrong = 0
        for b in range(len(st)):
            sc = {k: v[b:b + 1] for k, v in scene.items()}
            want, in_band, tested = fg.graph_verdicts(nodes[b], np.ones(nodes.shape[1], bool), es[b], sc, GRIPPER_BAND)
            left += in_band
            t = want != 0
            wrong += (not in_band) and not np.array_equal(want[t], es[b][t])
            worst = max(worst, float(np.abs(fg.place(tested, pts32, np.float32).astype(np.float64)
                                            - fg.place(tested.astype(np.float64), pts64)).max()))
        print(f"{kind}: {left} of {len(st)} left out ({left / len(st):.4f}), {wrong} disagree")
        assert left / len(st) <= LEFT_OUT_CAP and wrong == 0
    print(f"placement, float32 vs float64 over the tested poses: max {worst:.3e} m; GRIPPER_BAND {GRIPPER_BAND:.3e} m")
    assert PLACEMENT_REFERENCE / 2 <= worst <= PLACEMENT_REFERENCE * 2
