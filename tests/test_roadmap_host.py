"""CPU: ``mpx_franka_roadmap`` and ``mpx_franka_plan_seeded`` refuse bad arguments on the host, before any launch; the
float64 restatement (tests/float64_roadmap.py) stands on its own -- the node draws' keying, the lazy search against an
independent shortest-path routine, the one-edge path, the resampling's endpoints -- and, run as a planner on the forced-detour
problems of tests/test_gpu_plan.py, solves what the plain restatement solves and more.  The bar of the GPU seed-trajectory
test and the cap of its left-out problems are derived here."""
import ctypes
import os
import re
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_plan as fp  # noqa: E402
import float64_roadmap as fr  # noqa: E402
from float64_collision import SDF_BAR  # noqa: E402  (the band of a primitive SDF in float32 against float64, metres)

from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd import scenes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETOUR_SEED = 77       # the generator seed of tests/test_gpu_plan.py's ``detour`` fixture
DETOUR_PLAN_SEED = 9   # ... and the Philox seed its planner runs with (the roadmap's draws use it too)
LEFT_OUT_CAP = 0.10    # share of the problems that may have a tested configuration inside the band


def both_limits():
    """Inside the measured AND the published joint limits (tests/test_gpu_plan.py)."""
    return np.stack([np.maximum(ft.JOINT_LIMITS_REAL[:, 0], ft.JOINT_LIMITS_PUBLISHED[:, 0]),
                     np.minimum(ft.JOINT_LIMITS_REAL[:, 1], ft.JOINT_LIMITS_PUBLISHED[:, 1])], 1)


def detour_problems(B=256):
    """tests/test_gpu_plan.py's ``detour`` problems, rebuilt with the same generator: free space but for ONE 10 cm cube per
    problem, centred on the first link-4 collision sphere of the configuration halfway along the straight line.
    -> q_start, q_goal (float32 [B,7]), limits, scene arrays (``scenes.make_scenes`` layout)."""
    lim = both_limits()
    rng = np.random.default_rng(DETOUR_SEED)
    qs, qg = ((lim[:, 0] + rng.random((B, 7)) * (lim[:, 1] - lim[:, 0])).astype(np.float32) for _ in range(2))
    mid = torch.from_numpy(fp.line(qs, qg, 3)[:, 1]).double()
    x, _, _, _, link = fp.sphere_centres(mid)
    centre = x[:, int(torch.nonzero(link == 4)[0, 0])].numpy().astype(np.float32)
    scn = {"cuboid_centers": centre[:, None], "cuboid_dims": np.full((B, 1, 3), 0.1, np.float32),
           "cuboid_quats": np.tile(np.float32([1, 0, 0, 0]), (B, 1, 1)), "cylinder_centers": np.zeros((B, 1, 3), np.float32),
           "cylinder_radii": np.zeros((B, 1, 1), np.float32), "cylinder_heights": np.zeros((B, 1, 1), np.float32),
           "cylinder_quats": np.tile(np.float32([1, 0, 0, 0]), (B, 1, 1))}
    return qs, qg, lim, scn


def margins(q, scene_b, reach, check_self, self_margin):
    """q [N,7] float64 (torch) against one problem -> the smallest signed distance to a verdict's threshold per
    configuration: min over spheres of ``sdf - r_s - reach`` and, with ``check_self``, of the self model's
    ``distance - (0.15 + radius + margin)``.  Negative: invalid."""
    x, _, t, radii, _ = fp.sphere_centres(q)
    N, S = x.shape[:2]
    m = torch.full((N,), float("inf"), dtype=torch.float64)
    if scene_b is not None and scene_b["cub_dims"].shape[1] + scene_b["cyl_radii"].shape[1] > 0:
        best, _, _ = fp.sdf_min_grad(x.reshape(1, N * S, 3), scene_b)
        m = torch.minimum(m, (best.reshape(N, S) - radii - reach).amin(-1))
    if check_self:
        for link, radius in ((7, 0.1), (9, 0.01), (12, 0.01), (13, 0.01)):
            c = t[:, link]
            dz = c[:, 2] - torch.clamp(c[:, 2], -0.3, 0.333)
            m = torch.minimum(m, torch.sqrt(c[:, 0] ** 2 + c[:, 1] ** 2 + dz ** 2) - (0.15 + radius + self_margin))
    return m.numpy()


def graph_verdicts(nodes, edge_state, scene_b, resolution=fr.DEFAULTS["resolution"], reach=1e-4, check_self=True,
                   self_margin=1e-4, band=SDF_BAR):
    """The float64 verdict on the diagonal and on every TESTED edge of a given ``edge_state`` [V,V] over float32 ``nodes``
    [V,7] (a device's, or the restatement's own) -> (expected uint8 [V,V] on those entries, 0 elsewhere; in_band bool: some
    configuration that decides one of them lies within ``band`` of its threshold, so float32 may decide it the other way)."""
    nodes = np.asarray(nodes, np.float32)
    V = nodes.shape[0]
    W32 = fr.lengths(nodes, np.float32)
    want = np.zeros((V, V), np.uint8)
    edges = list(zip(*np.nonzero(np.triu(edge_state != fr.UNTESTED, 1))))
    configs = [fr.edge_configs(nodes[a], nodes[b], fr.pieces(W32[a, b], np.float32(resolution), np.float32), np.float32)
               for a, b in edges]
    m = margins(torch.from_numpy(np.concatenate([nodes] + configs, 0).astype(np.float64)), scene_b, reach, check_self,
                self_margin)  # (one call per problem: the nodes, then every tested edge's pieces)
    mv, at = m[:V], V
    want[np.arange(V), np.arange(V)] = np.where(mv > 0, fr.FREE, fr.BLOCKED)
    in_band = bool((np.abs(mv) <= band).any())
    for (a, b), q in zip(edges, configs):
        me, at = m[at:at + len(q)], at + len(q)
        want[a, b] = want[b, a] = fr.FREE if (me > 0).all() else fr.BLOCKED
        if not (me < -band).any() and (np.abs(me) <= band).any():  # (a definite hit decides the edge whatever else is close)
            in_band = True
    return want, in_band


# ---- refusals ------------------------------------------------------------------------------------------------------------------
GOOD = dict(nodes=64, resolution=0.05, connect_radius=float("inf"), max_rounds=8, smooth_passes=4, check_margin=1e-4,
            clearance=0.0, check_self=1)


def _roadmap(lib, B=4, T=50, S=0, M1=0, opts=None, env_offset=0, traj=256, status=256, path=256, hops=256, qs=256, lim=256):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731  (any non-NULL "device pointer": refused before it is touched)
    sph, cub = p(256 if S else 0), p(256 if M1 else 0)
    return lib.mpx_franka_roadmap(p(qs), p(256), B, T, 0.025, p(lim), sph, sph, sph, S, cub, cub, M1, None, None, None, 0,
                                  None if opts is None else ctypes.byref(opts), 0, env_offset, p(traj), p(status), p(path),
                                  p(hops), None, None, None, None)


def test_roadmap_refuses_bad_arguments_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    opt = lambda **kw: _lib.RoadmapOptions(**dict(GOOD, **kw))  # noqa: E731
    # what mpx_franka_plan refuses
    for T in (1, 65):
        assert _roadmap(lib, T=T) != 0 and b"waypoints" in lib.mpx_last_error()
    assert _roadmap(lib, B=-1) != 0 and b"negative size" in lib.mpx_last_error()
    assert _roadmap(lib, S=65) != 0 and b"65" in lib.mpx_last_error()
    assert _roadmap(lib, M1=65, S=56) != 0 and b"64 cuboids" in lib.mpx_last_error()
    assert _roadmap(lib, M1=4, S=0) != 0 and b"without collision spheres" in lib.mpx_last_error()
    assert _roadmap(lib, env_offset=-1) != 0 and b"env_offset" in lib.mpx_last_error()
    assert _roadmap(lib, env_offset=(1 << 32)) != 0 and b"env_offset" in lib.mpx_last_error()
    assert _roadmap(lib, opts=opt(check_margin=-1e-4)) != 0 and b"check_margin" in lib.mpx_last_error()
    assert _roadmap(lib, opts=opt(clearance=float("nan"))) != 0 and b"clearance" in lib.mpx_last_error()
    assert _roadmap(lib, qs=0) != 0 and b"NULL operand" in lib.mpx_last_error()
    assert _roadmap(lib, lim=0) != 0 and b"NULL operand" in lib.mpx_last_error()
    # its own
    for V in (-1, 0, 1, 257):
        assert _roadmap(lib, opts=opt(nodes=V)) != 0 and b"nodes" in lib.mpx_last_error()
    for res in (0.0, -0.05, float("nan")):
        assert _roadmap(lib, opts=opt(resolution=res)) != 0 and b"resolution" in lib.mpx_last_error()
    assert _roadmap(lib, opts=opt(connect_radius=float("nan"))) != 0 and b"connect_radius" in lib.mpx_last_error()
    assert _roadmap(lib, opts=opt(max_rounds=0)) != 0 and b"max_rounds" in lib.mpx_last_error()
    assert _roadmap(lib, opts=opt(smooth_passes=-1)) != 0 and b"smooth_passes" in lib.mpx_last_error()
    for out in ("traj", "status", "path", "hops"):
        assert _roadmap(lib, **{out: 0}) != 0 and b"NULL output" in lib.mpx_last_error()
    # nothing to do, nothing touched; a bad option is refused even then
    assert _roadmap(lib, B=0, traj=0, status=0, path=0, hops=0, qs=0, lim=0) == 0
    assert _roadmap(lib, B=0, opts=opt(nodes=1)) != 0


def _seeded(lib, B=4, T=50, opts=None, seeds=256, Ks=1, traj=256, status=256, env_offset=0):
    p = lambda v: ctypes.c_void_p(v) if v else None  # noqa: E731
    return lib.mpx_franka_plan_seeded(p(256), p(256), B, T, 0.025, p(256), None, None, None, 0, None, None, 0, None, None,
                                      None, 0, None if opts is None else ctypes.byref(opts), 0, env_offset, p(seeds), Ks,
                                      p(traj), p(status), None, None, None, None)


def test_seeded_planner_refuses_bad_arguments_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    good = dict(candidates=8, iterations=10, step=1e-3, smooth_weight=1.0, epsilon=0.05, spread=0.5, substeps=4,
                check_margin=1e-4, clearance=0.0, max_jerk=0.15, check_self=1)
    assert _seeded(lib, Ks=9) != 0 and b"candidates + seeds" in lib.mpx_last_error()  # 8 + 9 > 16
    assert _seeded(lib, Ks=1, opts=_lib.PlanOptions(**dict(good, candidates=16))) != 0 and b"candidates + seeds" in lib.mpx_last_error()
    assert _seeded(lib, Ks=-1) != 0 and b"negative size" in lib.mpx_last_error()
    assert _seeded(lib, Ks=2, seeds=0) != 0 and b"seeds" in lib.mpx_last_error()
    # mpx_franka_plan's own refusals, under this entry's name
    assert _seeded(lib, T=65) != 0 and b"mpx_franka_plan_seeded" in lib.mpx_last_error()
    assert _seeded(lib, traj=0) != 0 and b"NULL output" in lib.mpx_last_error()
    assert _seeded(lib, opts=_lib.PlanOptions(**dict(good, step=0.0))) != 0 and b"step" in lib.mpx_last_error()
    assert _seeded(lib, env_offset=-1) != 0 and b"env_offset" in lib.mpx_last_error()
    assert _seeded(lib, B=0, traj=0, status=0, seeds=0, Ks=3) == 0


def test_python_entry_points_and_defaults_are_one_set():
    import inspect

    from mpinets_amd import _lib, robot

    q = torch.zeros(2, 7)
    for fn in (robot.franka_roadmap, robot.franka_plan_global):
        with pytest.raises(_lib.MpxError):
            fn(q, q)
        assert inspect.signature(fn).parameters["T"].default == 50
    with pytest.raises(TypeError):
        robot._roadmap_options("franka_roadmap", {"node": 3})
    assert inspect.signature(robot.franka_plan).parameters["seeds"].default is None
    assert inspect.signature(scenes.make_problem_batch).parameters["expert_from"].default == "primitives"
    assert robot.ROADMAP_DEFAULTS == fr.DEFAULTS
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    for key in ("nodes", "resolution", "max_rounds", "smooth_passes"):
        m = re.search(r"#define MPX_ROADMAP_DEFAULT_%s\s+([0-9.e+-]+)f?" % key.upper(), text)
        assert m and float(m.group(1)) == pytest.approx(float(fr.DEFAULTS[key]), rel=1e-6), key
    assert int(re.search(r"#define MPX_ROADMAP_MAX_NODES\s+(\d+)", text).group(1)) == fr.MAX_NODES
    assert fr.DEFAULTS["check_margin"] == fp.DEFAULTS["check_margin"]


def test_roadmap_kernel_uses_no_scratch():
    """Four waves per workgroup leave a wave the registers of the planner's <= 8-candidate form."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "franka_roadmap_kernel" in n}
    assert len(hits) == 1
    (f,) = hits.values()
    print({k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0


# ---- the restatement's own properties ------------------------------------------------------------------------------------------
def test_nodes_are_keyed_by_the_global_problem_id():
    qs, qg = scenes.random_configurations(40, 0), scenes.random_configurations(40, 1)
    a = fr.draw_nodes(qs, qg, V=64, seed=3)
    b = fr.draw_nodes(qs[15:], qg[15:], V=64, seed=3, env_offset=15)
    assert a.dtype == np.float32 and np.array_equal(a[15:], b)
    assert np.array_equal(a[:, 0], qs) and np.array_equal(a[:, 1], qg)
    other = fr.draw_nodes(qs, qg, V=64, seed=4)
    assert np.array_equal(a[:, :2], other[:, :2]) and not np.array_equal(a[:, 2:], other[:, 2:])
    assert np.array_equal(fr.draw_nodes(qs, qg, V=16, seed=3), a[:, :16])  # (a node's draw does not depend on V)
    lim = fp.limits32(ft.JOINT_LIMITS_REAL)
    assert ((a[:, 2:] >= lim[:, 0]) & (a[:, 2:] <= lim[:, 1])).all()
    assert len(np.unique(a[:, 2:].reshape(-1))) > 0.99 * a[:, 2:].size  # (seven different words per node)


def _toy(seed, V=48):
    """A planar toy in the first two joints: start and goal left and right of a disc, V - 2 uniform nodes."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros((V, 7), np.float32)
    nodes[:, :2] = rng.uniform(-1, 1, size=(V, 2))
    nodes[0, :2], nodes[1, :2] = (-0.9, 0.05 * seed), (0.9, -0.03 * seed)
    centre, radius = np.float64([0.05, 0.0]), 0.45

    def is_valid(q):
        return np.linalg.norm(np.asarray(q, np.float64)[:, :2] - centre, axis=-1) > radius
    return nodes, is_valid


@pytest.mark.parametrize("seed", range(6))
def test_lazy_search_ends_with_the_shortest_path_among_edges_not_blocked(seed):
    nodes, is_valid = _toy(seed)
    st, path, state, rounds = fr.search(nodes, is_valid, resolution=0.02, max_rounds=200)
    assert st == 0 and path[0] == 0 and path[-1] == 1 and len(path) >= 3 and rounds >= 2  # (the disc blocks the direct edge)
    assert state[0, 1] == fr.BLOCKED and np.array_equal(state, state.T)
    assert all(state[u, v] == fr.FREE for u, v in zip(path[:-1], path[1:]))
    assert len(set(path)) == len(path) and all(is_valid(nodes[path]))
    # every tested verdict is right, by a finer test than the search's
    for a, b in zip(*np.nonzero(np.triu(state != fr.UNTESTED, 1))):
        fine = fr.edge_configs(nodes[a], nodes[b], 4000)
        assert bool(is_valid(fine).all()) == (state[a, b] == fr.FREE) or state[a, b] == fr.FREE  # (0.02 pieces can miss a graze)
    # shortest over "valid nodes, edges not blocked": an independent routine gives the same cost
    assert fr.path_cost(nodes, path) == pytest.approx(fr.dijkstra_cost(nodes, state), rel=1e-12)
    # one round less is not enough, and a radius that cuts every way round leaves status 1
    assert fr.search(nodes, is_valid, resolution=0.02, max_rounds=rounds - 1)[0] == 1
    assert fr.search(nodes, is_valid, resolution=0.02, connect_radius=0.05)[0] == 1
    bad = nodes.copy()
    bad[1, :2] = (0.05, 0.0)  # the goal inside the disc
    assert fr.search(bad, is_valid)[0] == 2


def test_one_edge_path_is_the_planners_line_and_resampling_keeps_the_endpoints():
    B, T = 24, 50
    qs, qg = scenes.random_configurations(B, 5), scenes.random_configurations(B, 6)
    traj, status, path, hops, nodes, state, rounds = fr.solve(qs, qg, None, T=T, seed=1, nodes=16)
    planned = status != 2  # (a uniform draw can itself be a self collision)
    assert planned.sum() >= B // 2
    L = fp.line(qs, qg, T)
    one = planned & (hops == 1)
    assert one.sum() >= 4 and np.array_equal(traj[one], L[one].astype(np.float64))
    assert (rounds[one] == 1).all() and (path[one][:, :2] == [0, 1]).all() and (path[one][:, 2:] == -1).all()
    assert np.isnan(traj[status != 0]).all() and (hops[status != 0] == 0).all() and (path[status != 0] == -1).all()
    # a bent polyline: endpoints exact in both precisions, every waypoint on the polyline, equal steps of arc length
    rng = np.random.default_rng(2)
    for H in (2, 3, 7):
        pts = rng.uniform(-2, 2, size=(H + 1, 7)).astype(np.float32)
        for dt in (np.float64, np.float32):
            r = fr.resample(pts, T, dt)
            assert np.array_equal(r[0], pts[0].astype(dt)) and np.array_equal(r[-1], pts[-1].astype(dt))
            s = fr.smooth(r, 5, dt)
            assert np.array_equal(s[0], r[0]) and np.array_equal(s[-1], r[-1])
        r = fr.resample(pts, 4 * T)
        total = fr.path_cost(pts, range(H + 1))
        step = np.linalg.norm(r[1:] - r[:-1], axis=-1)
        assert step.max() <= total / (4 * T - 1) * (1 + 1e-9)  # (a chord across a corner is shorter than the arc)
        seg = pts[1:].astype(np.float64) - pts[:-1]
        rel = r[:, None] - pts[None, :-1]
        u = np.clip((rel * seg).sum(-1) / (seg * seg).sum(-1), 0, 1)
        assert np.abs(rel - u[..., None] * seg).max(-1).min(-1).max() < 1e-12
    assert np.array_equal(fr.seed_trajectory(pts, [0, 1], T, 8), fp.line(pts[:1], pts[1:2], T)[0])


# ---- the restatement as a planner on the forced-detour problems ----------------------------------------------------------------
# recorded by test_restatement_solves_more_detour_problems (float64, the default options)
DETOUR_PLANNED, DETOUR_PLAIN_SOLVED = 162, 111  # tests/test_gpu_plan.py::test_forced_detour records the same two
DETOUR_GLOBAL_SOLVED = 157                      # ... with the roadmap's seed as a ninth candidate


@pytest.fixture(scope="module")
def detour():
    qs, qg, lim, scn = detour_problems()
    scene = fp.scene_from_arrays(scn)
    t0 = time.time()
    road = fr.solve(qs, qg, scene, limits=lim, seed=DETOUR_PLAN_SEED)
    t1 = time.time()
    seeded = fr.solve_seeded(qs, qg, road[0][:, None], scene, limits=lim, seed=DETOUR_PLAN_SEED)
    print(f"detour restatement: roadmap {t1 - t0:.0f} s, seeded optimiser {time.time() - t1:.0f} s")
    return qs, qg, lim, scene, road, seeded


def test_restatement_solves_more_detour_problems(detour):
    """The restatement as a planner (roadmap, then the seeded optimiser, float64, default options) on the 256 forced-detour
    problems.  Candidates 0 .. 7 are the plain planner's, so it solves at least every problem the plain restatement
    solves; the defaults are right only if it solves strictly more.  Measured (14 s for the roadmap, 73 s for the optimiser
    on 16 threads): 162 planned, the roadmap finds a path for 160 (143 of two edges, 17 of three; 2 run out of their 64
    rounds), the plain candidates solve 111, with the seed 157: of the 51 the plain planner leaves, the seed is valid on 46
    and hits the cube after its 20 iterations on 5."""
    qs, qg, lim, scene, (seed_traj, rst, path, hops, nodes, state, rounds), (traj, st, choice, all_traj, bits) = detour
    K = fp.DEFAULTS["candidates"]
    plain_ok = (bits[:, :K] == 0).any(1) & (st != 2)
    ok = st == 0
    found = rst == 0
    print(f"forced detour, float64 restatement: planned {int((st != 2).sum())}, plain solves {int(plain_ok.sum())}, with the "
          f"roadmap seed {int(ok.sum())}; roadmap status 0 / 1 / 2: {np.bincount(rst, minlength=3).tolist()}, hops histogram "
          f"{np.bincount(hops[found]).tolist()}, rounds histogram {np.bincount(rounds).tolist()}, seed bits histogram "
          f"{np.bincount(bits[found, K], minlength=8).tolist()}, choice histogram {np.bincount(choice[ok], minlength=K + 1).tolist()}")
    assert int((st != 2).sum()) == DETOUR_PLANNED and int(plain_ok.sum()) == DETOUR_PLAIN_SOLVED
    assert np.array_equal(rst == 2, st == 2)  # one rule for the endpoints
    assert bool(ok[plain_ok].all())
    first = np.where((bits[:, :K] == 0).any(1), (bits[:, :K] == 0).argmax(1), -1)
    assert np.array_equal(choice[plain_ok], first[plain_ok])  # ... and returns the plain planner's own row there
    assert int(ok.sum()) > int(plain_ok.sum()) and int(ok.sum()) == DETOUR_GLOBAL_SOLVED
    assert (bits[(st != 2) & ~found, K] == 7).all() and np.isnan(all_traj[(st != 2) & ~found, K]).all()
    assert (hops[found] >= 2).all()  # (the cube sits on the line: no one-edge path)
    won = ok & ~plain_ok
    assert (choice[won] == K).all()
    assert np.array_equal(traj[won][:, 0], qs[won].astype(np.float64)) and np.array_equal(traj[won][:, -1], qg[won].astype(np.float64))


def test_left_out_share_of_the_edge_state_comparison(detour):
    """The GPU test leaves out the problems where a configuration that decides a tested verdict lies within SDF_BAR
    (tests/float64_collision.py) of its threshold.  On the restatement's own graphs of the detour problems at seed
    DETOUR_PLAN_SEED the share is printed and stays below LEFT_OUT_CAP; the restatement's graph agrees with the verdicts
    recomputed from the float32 pieces everywhere else."""
    qs, qg, lim, scene, (seed_traj, rst, path, hops, nodes, state, rounds), _ = detour
    rows = np.flatnonzero(rst != 2)[:96]
    left, wrong = 0, 0
    for b in rows:
        want, in_band = graph_verdicts(nodes[b], state[b], {k: v[b:b + 1] for k, v in scene.items()})
        left += in_band
        tested = want != 0
        wrong += (not in_band) and not np.array_equal(want[tested], state[b][tested])
    print(f"edge-state comparison on {len(rows)} detour problems: {left} left out ({left / len(rows):.4f}), {wrong} disagree")
    assert left / len(rows) <= LEFT_OUT_CAP and wrong == 0


# what the bar of tests/test_gpu_roadmap.py's seed-trajectory test is 4x of (recorded on the CPU)
SEED_REFERENCE = 7.7e-7


def seed_reference_difference(nodes, path, hops, T, passes):
    """The restatement's resample-and-smooth in float32 against float64 from the same float32 nodes and paths, over the
    rows with more than one edge -> the largest |q| difference."""
    worst = 0.0
    for b in np.flatnonzero(hops >= 2):
        p = path[b, :hops[b] + 1]
        a64 = fr.seed_trajectory(nodes[b], list(p), T, passes, np.float64)
        a32 = fr.seed_trajectory(nodes[b], list(p), T, passes, np.float32)
        worst = max(worst, float(np.abs(a64 - a32.astype(np.float64)).max()))
    return worst


def test_seed_trajectory_bar_can_be_derived_again(detour):
    """Reference against reference on the paths of the detour problems (float32 nodes, T = 50, the default passes): the
    float32 run of resample-and-smooth differs from the float64 run by 7.69e-7 rad at most over 160 paths (joint angles up
    to 2.9 rad: an ulp is 2.4e-7; the arc length, the division and eight filter passes each add theirs).  The GPU test's bar is 4x the recorded figure; here the measurement is repeated and must land
    within a factor 2 of it."""
    _, _, _, _, (seed_traj, rst, path, hops, nodes, state, rounds), _ = detour
    worst = seed_reference_difference(nodes, path, hops, 50, fr.DEFAULTS["smooth_passes"])
    print(f"seed trajectory, float32 vs float64 restatement over {int((hops >= 2).sum())} paths: max {worst:.3e}")
    assert SEED_REFERENCE / 2 <= worst <= SEED_REFERENCE * 2
