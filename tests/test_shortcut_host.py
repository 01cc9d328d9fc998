"""CPU: ``mpx_franka_shortcut`` and ``mpx_franka_shortcut_cloud`` refuse bad arguments on the host, before any launch; their
kernels use no scratch; the Python defaults are the header's; the restatement (tests/float64_shortcut.py) keeps its
invariants on the forced-detour problems of tests/test_roadmap_host.py -- the length never grows, the end points are kept, a
free straight line gives one hop, no passes give the input back.  The bars of tests/test_gpu_shortcut.py are derived here:
the float32 run of the restatement against its float64 run, and the share of rows left out because a configuration that
decides a chord lies within the band of its threshold.  Last, the restatement as a planner: the detour problems solved with
TWO seeds, the shortcut trajectory in front of the roadmap's."""
import ctypes
import inspect
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
import float64_roadmap_cloud as frc  # noqa: E402
import float64_shortcut as fs  # noqa: E402
from float64_collision import SDF_BAR  # noqa: E402
from test_roadmap_cloud_host import BAND as FIELD_BAND, POINT_RADIUS, detour_field  # noqa: E402
from test_roadmap_cloud_host import DETOUR_PLAN_SEED as CLOUD_PLAN_SEED  # noqa: E402
from test_roadmap_host import DETOUR_GLOBAL_SOLVED, DETOUR_PLAN_SEED, DETOUR_PLANNED, LEFT_OUT_CAP, detour_problems, margins  # noqa: E402

from mpinets_amd import _lib, capture, robot, scenes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_ROWS = 64                     # the detour rows tests/test_gpu_shortcut.py compares decisions on
CLOUD_ROWS = 24                      # float64_cloud_plan.DETOUR_B: the rows of the cloud form's comparison
REACH, SELF_MARGIN = 1e-4, 1e-4      # clearance + check_margin and check_margin at the defaults

# recorded by test_float32_run_against_float64_run: the largest |difference| of points_out and of traj [rad] between the
# restatement's float32 and float64 runs over the rows on which both take the same decisions.  Joint angles reach 2.9 rad
# (an ulp is 2.4e-7); a kept vertex is a dense point (one division, one fma) of a polyline whose vertices are dense points of
# the pass before, and traj adds the arc length, a division and eight filter passes, as SEED_REFERENCE does.
POINTS_REFERENCE = 2.1e-7  # (39 rows, none with different decisions)
TRAJ_REFERENCE = 4.8e-7
# recorded by test_two_seeds_solve_no_fewer_detour_problems (float64 optimiser, the float32-geometry shortcut's seeds)
DETOUR_SHORTCUT_SOLVED = 157


def prim_rule(scene, b):
    """-> is_valid, margins of detour problem ``b`` at the default options."""
    sc = {k: v[b:b + 1] for k, v in scene.items()}
    valid = fr.franka_validity(sc, REACH, True, SELF_MARGIN)
    return valid, lambda q: margins(torch.from_numpy(np.ascontiguousarray(q, np.float64)), sc, REACH, True, SELF_MARGIN)


def field_rule(field_b, grid, point_radius=POINT_RADIUS):
    """-> is_valid, margins of one environment's field at the default options (``float64_roadmap_cloud.margins``' two)."""
    valid = frc.field_validity(field_b, grid, point_radius=point_radius)

    def m(q):
        env, own = frc.margins(torch.from_numpy(np.ascontiguousarray(q, np.float64)), field_b, grid, point_radius=point_radius)
        return np.minimum(env, own)
    return valid, m


# ---- refusals ------------------------------------------------------------------------------------------------------------------
GOOD = dict(points=64, passes=2, fanout=4, resolution=0.05, smooth_passes=8, check_margin=1e-4, clearance=0.0, check_self=1)


def _p(v):  # any non-NULL "device pointer": refused before it is touched
    return ctypes.c_void_p(v) if v else None


def _shortcut(lib, B=4, Pin=64, T=50, S=0, M1=0, opts=None, pts=256, count=256, traj=256, status=256, points_out=256,
              count_out=256, length=256):
    sph, cub = _p(256 if S else 0), _p(256 if M1 else 0)
    return lib.mpx_franka_shortcut(_p(pts), _p(count), B, Pin, T, 0.025, sph, sph, sph, S, cub, cub, M1, None, None, None, 0,
                                   None if opts is None else ctypes.byref(opts), _p(traj), _p(status), _p(points_out),
                                   _p(count_out), _p(length), None, None, None)


def _shortcut_cloud(lib, B=4, Pin=64, T=50, S=56, field=256, trunc=0.2, point_radius=0.02, field_slack=0.0, opts=None,
                    pts=256, traj=256, table=256, grid=True):
    g = _lib.FieldGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), 0.05, 8, 8, 8, trunc)
    return lib.mpx_franka_shortcut_cloud(_p(pts), _p(256), B, Pin, T, 0.025, _p(table), _p(table), _p(table), S, _p(field),
                                         ctypes.byref(g) if grid else None, point_radius, field_slack,
                                         None if opts is None else ctypes.byref(opts), _p(traj), _p(256), _p(256), _p(256),
                                         _p(256), None, None, None)


def test_shortcut_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    err = lib.mpx_last_error
    opt = lambda **kw: _lib.ShortcutOptions(**dict(GOOD, **kw))  # noqa: E731
    for call in (_shortcut, _shortcut_cloud):
        # the roadmap's set
        for T in (1, 65):
            assert call(lib, T=T) != 0 and b"waypoints" in err()
        assert call(lib, B=-1) != 0 and b"negative size" in err()
        assert call(lib, S=65) != 0 and b"65" in err()
        assert call(lib, opts=opt(check_margin=-1e-4)) != 0 and b"check_margin" in err()
        assert call(lib, opts=opt(clearance=float("nan"))) != 0 and b"clearance" in err()
        for res in (0.0, -0.05, float("nan")):
            assert call(lib, opts=opt(resolution=res)) != 0 and b"resolution" in err()
        assert call(lib, opts=opt(smooth_passes=-1)) != 0 and b"smooth_passes" in err()
        # its own
        for Pin in (-1, 0, 1, 257):
            assert call(lib, Pin=Pin, opts=opt(points=256)) != 0 and b"Pin" in err()
        for P in (63, 257, 0, -1):
            assert call(lib, opts=opt(points=P)) != 0 and b"points" in err()
        assert call(lib, opts=opt(passes=-1)) != 0 and b"passes" in err()
        for K in (0, -1, 257):
            assert call(lib, opts=opt(fanout=K)) != 0 and b"fanout" in err()
        assert call(lib, pts=0) != 0 and b"NULL operand" in err()
        assert call(lib, traj=0) != 0 and b"NULL output" in err()
        # nothing to do, nothing touched; a bad option is refused even then
        assert call(lib, B=0, pts=0, traj=0) == 0
        assert call(lib, B=0, opts=opt(fanout=0)) != 0
    assert _shortcut(lib, M1=65, S=56) != 0 and b"64 cuboids" in err()
    assert _shortcut(lib, M1=4, S=0) != 0 and b"without collision spheres" in err()
    for out in ("status", "points_out", "count_out", "length"):
        assert _shortcut(lib, **{out: 0}) != 0 and b"NULL output" in err()
    assert _shortcut(lib, count=0) != 0 and b"NULL operand" in err()
    # the field's, in mpx_franka_roadmap_cloud's words
    assert _shortcut_cloud(lib, point_radius=-0.01) != 0 and b"point_radius" in err()
    assert _shortcut_cloud(lib, field_slack=float("inf")) != 0 and b"field_slack" in err()
    assert _shortcut_cloud(lib, S=0) != 0 and b"without collision spheres" in err()
    assert _shortcut_cloud(lib, trunc=0.1) != 0 and b"trunc" in err()  # 0.08 + 0.02 + 1e-4 > 0.1
    assert _shortcut_cloud(lib, grid=False) != 0 and b"grid" in err()


def test_python_entry_points_and_defaults_are_one_set():
    q, n = torch.zeros(2, 3, 7), torch.full((2,), 3, dtype=torch.int32)
    for fn, args in ((robot.franka_shortcut, (q, n)), (robot.franka_shortcut_cloud, (q, n, None))):
        with pytest.raises(_lib.MpxError):
            fn(*args)
        assert inspect.signature(fn).parameters["T"].default == 50
        assert inspect.signature(fn).parameters["return_trace"].default is False
    with pytest.raises(TypeError):
        robot._shortcut_options("franka_shortcut", {"point": 3})
    assert robot.SHORTCUT_DEFAULTS == fs.DEFAULTS
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    for key in ("points", "passes", "fanout"):
        m = re.search(r"#define MPX_SHORTCUT_DEFAULT_%s\s+(\d+)" % key.upper(), text)
        assert m and int(m.group(1)) == fs.DEFAULTS[key], key
    assert int(re.search(r"#define MPX_SHORTCUT_MAX_FANOUT\s+(\d+)", text).group(1)) == fs.MAX_FANOUT
    assert fs.MAX_POINTS == fr.MAX_NODES
    for key in ("resolution", "smooth_passes", "check_margin", "clearance", "check_self"):  # the roadmap's
        assert fs.DEFAULTS[key] == fr.DEFAULTS[key], key
    assert [n for n, _ in _lib.ShortcutOptions._fields_] == list(fs.DEFAULTS)
    # the flag of the callers above: off by default, and refused where there is no roadmap to shortcut
    for fn in (robot.franka_plan_global, robot.franka_plan_global_cloud):
        assert inspect.signature(fn).parameters["shortcut"].default is None
    assert inspect.signature(scenes.make_problem_batch).parameters["expert_shortcut"].default is False
    assert inspect.signature(capture.plan_to_poses).parameters["shortcut"].default is False
    with pytest.raises(ValueError):
        scenes.make_problem_batch(2, device="cpu", collision_free=True, expert=True, expert_shortcut=True)
    with pytest.raises(ValueError):
        capture.plan_to_poses(q, q[:, 0], torch.zeros(2, 4, 4), shortcut=True)


def test_shortcut_kernels_use_no_scratch():
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "franka_shortcut" in n}
    assert len(hits) == 2
    for n, f in hits.items():
        print(n[:40], {k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0


# ---- the restatement on planar toys ----------------------------------------------------------------------------------------------
def _disc(centre=(0.0, 0.0), radius=0.45):
    c = np.float64(centre)
    return lambda q: np.linalg.norm(np.asarray(q, np.float64)[:, :2] - c, axis=-1) > radius


def _dogleg():
    p = np.zeros((3, 7), np.float32)
    p[:, :2] = [(-0.9, 0.0), (0.0, 1.5), (0.9, 0.0)]
    return p


def test_probes_and_densification():
    assert fs.probes(3, 11, 4) == [5, 7, 9, 11] and fs.probes(3, 4, 4) == [4] and fs.probes(3, 6, 4) == [4, 5, 6]
    assert fs.probes(3, 11, 1) == [11] and fs.probes(3, 11, 256) == list(range(4, 12))
    for dt in (np.float64, np.float32):
        D, at = fs.densify(_dogleg(), 64, dt)
        assert len(D) <= 64 and len(D) >= 62 and at[0] == 0 and at[-1] == len(D) - 1
        assert np.array_equal(D[at], _dogleg().astype(dt))  # the vertices are copied
        same = np.zeros((4, 7), np.float32)  # L = 0: nothing is added
        assert len(fs.densify(same, 64, dt)[0]) == 4
        assert len(fs.densify(_dogleg(), 3, dt)[0]) == 3  # P = n: nothing is added


@pytest.mark.parametrize("K", [1, 2, 4, 256])
def test_planar_dogleg_is_cut_and_a_free_line_gives_one_hop(K):
    p = _dogleg()
    before = fs.polyline_length(p)
    out = fs.shortcut(p, _disc(), fanout=K, resolution=0.01)
    assert out["length"][0] == before and out["length"][1] < 0.8 * before and len(out["points_out"]) >= 3
    assert np.array_equal(out["points_out"][0], p[0]) and np.array_equal(out["points_out"][-1], p[-1])
    for a, e in out["free"]:  # every chord found free is free by a finer test
        assert _disc(radius=0.449)(fr.edge_configs(a, e, 2000)).all()
    free = fs.shortcut(p, _disc(centre=(0.0, -2.0)), fanout=K)
    first_level = len(fs.probes(1, len(fs.densify(p, 64)[0]) - 1, K))  # (one level: its last chord reaches the far end)
    assert len(free["points_out"]) == 2 and free["chords"] == first_level
    assert np.array_equal(free["traj"], fp.line(p[:1], p[2:], 50)[0])
    kept = fs.shortcut(p, _disc(), passes=0, fanout=K)
    assert np.array_equal(kept["points_out"], p.astype(np.float64)) and kept["chords"] == 0
    assert np.array_equal(kept["traj"], fr.seed_trajectory(p, [0, 1, 2], 50, 8))
    walled = fs.shortcut(p, lambda q: np.zeros(len(q), bool), fanout=K)  # nothing is free: the input's own pieces remain
    assert walled["length"][1] <= before * (1 + 1e-12) and np.array_equal(walled["points_out"][[0, -1]], p[[0, 2]].astype(np.float64))


# ---- the restatement on the forced-detour problems -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detour():
    qs, qg, lim, scn = detour_problems()
    scene = fp.scene_from_arrays(scn)
    t0 = time.time()
    road = fr.solve(qs, qg, scene, limits=lim, seed=DETOUR_PLAN_SEED)
    pts, cnt = fs.path_polylines(road[4], road[2], road[3])
    runs = {}
    for b in np.flatnonzero(cnt >= 2):
        valid, m = prim_rule(scene, b)
        runs[b] = {np.float32: fs.shortcut(pts[b, :cnt[b]], valid, dtype=np.float32, margins=m, band=SDF_BAR)}
        if b < PARITY_ROWS:
            runs[b][np.float64] = fs.shortcut(pts[b, :cnt[b]], valid, dtype=np.float64)
    print(f"detour restatement: roadmap and {len(runs)} shortcuts {time.time() - t0:.0f} s")
    return qs, qg, lim, scene, road, pts, cnt, runs


def test_invariants_on_the_detour_paths(detour):
    """Over the roadmap's paths of the 256 detour problems (all of two or three edges): the returned polyline is never longer
    than the input, keeps its end points bit for bit, has at least three vertices (the cube sits on the straight line) and
    ``passes=0`` gives the input back.  The lengths are printed: they are what DESIGN.md quotes.  Measured on 160 paths: mean
    length 6.97 -> 5.47 rad (the straight line is 4.57), ratio 0.47 .. 1.00, median 0.80; 30 chords and 1 607 interior
    configurations per path on average (49 and 2 394 at most)."""
    qs, qg, lim, scene, road, pts, cnt, runs = detour
    ratio, n_chords, n_configs = [], [], []
    for b, r in runs.items():
        out = r[np.float32]
        before, after = out["length"]
        assert after <= before * (1 + 1e-6) and len(out["points_out"]) >= 3
        assert np.array_equal(out["points_out"][0], qs[b]) and np.array_equal(out["points_out"][-1], qg[b])
        assert np.array_equal(out["traj"][0], qs[b]) and np.array_equal(out["traj"][-1], qg[b])
        ratio.append(after / before), n_chords.append(out["chords"]), n_configs.append(out["configs"])
    lens = np.float64([[r[np.float32]["length"][0], r[np.float32]["length"][1]] for r in runs.values()])
    line = np.float64([np.linalg.norm(qg[b].astype(np.float64) - qs[b]) for b in runs])
    print(f"shortcut on {len(runs)} detour paths: mean length {lens[:, 0].mean():.3f} -> {lens[:, 1].mean():.3f} rad (straight line "
          f"{line.mean():.3f}), ratio min / median / max {min(ratio):.3f} / {np.median(ratio):.3f} / {max(ratio):.3f}, chords "
          f"mean {np.mean(n_chords):.1f} max {max(n_chords)}, configurations mean {np.mean(n_configs):.0f} max {max(n_configs)}")
    assert np.median(ratio) < 1.0
    b = next(iter(runs))
    kept = fs.shortcut(pts[b, :cnt[b]], lambda q: np.ones(len(q), bool), passes=0)
    assert np.array_equal(kept["points_out"], pts[b, :cnt[b]].astype(np.float64)) and kept["chords"] == 0
    assert np.array_equal(kept["traj"], np.asarray(road[0][b]))  # ... and the roadmap's own seed trajectory
    free = fs.shortcut(pts[b, :cnt[b]], lambda q: np.ones(len(q), bool))
    assert len(free["points_out"]) == 2 and free["chords"] == fs.DEFAULTS["fanout"]  # (one level)


def test_left_out_share_of_the_decision_comparison(detour):
    """tests/test_gpu_shortcut.py leaves out the rows where a configuration that decides a chord lies within SDF_BAR of its
    threshold.  On the first PARITY_ROWS detour rows the restatement's own float32-geometry run stays under LEFT_OUT_CAP."""
    qs, qg, lim, scene, road, pts, cnt, runs = detour
    rows = [b for b in runs if b < PARITY_ROWS]
    left = sum(runs[b][np.float32]["in_band"] for b in rows)
    print(f"decision comparison on {len(rows)} detour rows with a path (of {PARITY_ROWS}): {left} left out")
    assert len(rows) >= PARITY_ROWS // 2 and left / len(rows) <= LEFT_OUT_CAP


def test_float32_run_against_float64_run(detour):
    """Reference against reference: the restatement with float32 geometry against the one with float64 geometry, both
    judged in float64, over the first PARITY_ROWS detour rows.  Where both take the same decisions (the same chords,
    configurations and vertex count) ``points_out`` and ``traj`` differ by POINTS_REFERENCE / TRAJ_REFERENCE at most; the
    GPU test's bars are 4x the recorded figures, tests/test_gpu_roadmap.py's convention, and the measurement must land within
    a factor 2 of them here."""
    qs, qg, lim, scene, road, pts, cnt, runs = detour
    worst_p, worst_t, same, differ = 0.0, 0.0, 0, 0
    for b, r in runs.items():
        if np.float64 not in r:
            continue
        a32, a64 = r[np.float32], r[np.float64]
        if (a32["chords"], a32["configs"], len(a32["points_out"])) != (a64["chords"], a64["configs"], len(a64["points_out"])):
            differ += 1
            continue
        same += 1
        worst_p = max(worst_p, float(np.abs(a32["points_out"].astype(np.float64) - a64["points_out"]).max()))
        worst_t = max(worst_t, float(np.abs(a32["traj"].astype(np.float64) - a64["traj"]).max()))
    print(f"float32 vs float64 restatement over {same} rows (decisions differ on {differ}): points_out max {worst_p:.3e}, "
          f"traj max {worst_t:.3e}")
    assert same >= PARITY_ROWS // 2 and differ <= LEFT_OUT_CAP * (same + differ)
    assert POINTS_REFERENCE / 2 <= worst_p <= POINTS_REFERENCE * 2
    assert TRAJ_REFERENCE / 2 <= worst_t <= TRAJ_REFERENCE * 2


def test_cloud_form_left_out_share_and_invariants():
    """The cloud form's rows (float64_cloud_plan.DETOUR_B = 24, the detour drawn as a cloud, the host-built field): the same
    invariants with ``float64_roadmap_cloud``'s validity test, and the left-out share at the cloud roadmap test's band."""
    qs, qg, lim, cloud, grid, field = detour_field(CLOUD_ROWS)
    road = frc.solve(qs, qg, field, grid, POINT_RADIUS, limits=lim, seed=CLOUD_PLAN_SEED)
    pts, cnt = fs.path_polylines(road[4], road[2], road[3])
    rows = np.flatnonzero(cnt >= 2)
    left = 0
    for b in rows:
        valid, m = field_rule(field[b], grid)
        out = fs.shortcut(pts[b, :cnt[b]], valid, dtype=np.float32, margins=m, band=FIELD_BAND)
        left += out["in_band"]
        assert out["length"][1] <= out["length"][0] * (1 + 1e-6)
        assert np.array_equal(out["points_out"][0], qs[b]) and np.array_equal(out["points_out"][-1], qg[b])
    print(f"cloud form: {len(rows)} of {CLOUD_ROWS} rows with a path, {left} left out")
    assert len(rows) >= 6 and left / len(rows) <= LEFT_OUT_CAP


def test_two_seeds_solve_no_fewer_detour_problems(detour):
    """The restatement as a planner on the 256 forced-detour problems (162 planned): ``float64_roadmap.solve_seeded`` with the
    shortcut's trajectory as candidate 8 and the roadmap's as candidate 9.  Candidates 0 .. 7 and the roadmap's seed are
    what tests/test_roadmap_host.py solves DETOUR_GLOBAL_SOLVED = 157 with, and the lowest valid candidate wins, so no fewer
    are solved; the count, and the mean joint-space length of the returned trajectories where the shortcut's seed won
    against what the roadmap's seed gives on the same rows, are printed for DESIGN.md.  Measured (62 s for the optimiser on
    16 threads): 162 planned, 157 solved with and without the shortcut's seed; that seed is valid on 144 rows and is the
    choice on 38 (the roadmap's own on 8), where the returned trajectory is 5.49 rad long against 6.71 rad from the
    roadmap's seed on the same rows."""
    qs, qg, lim, scene, road, pts, cnt, runs = detour
    T = 50
    seeds = np.full((len(qs), 2, T, 7), np.nan, np.float32)
    seeds[:, 1] = road[0]
    for b, r in runs.items():
        seeds[b, 0] = r[np.float32]["traj"]
    t0 = time.time()
    traj, st, choice, all_traj, bits = fr.solve_seeded(qs, qg, seeds, scene, limits=lim, seed=DETOUR_PLAN_SEED)
    K = fp.DEFAULTS["candidates"]
    ok = st == 0
    old = (bits[:, list(range(K)) + [K + 1]] == 0).any(1) & (st != 2)  # what candidates 0 .. 7 and the roadmap's seed solve
    both = ok & (bits[:, K] == 0) & (bits[:, K + 1] == 0) & (choice == K)

    def mean_len(t):
        return float(np.linalg.norm(np.diff(t, axis=1), axis=-1).sum(-1).mean()) if len(t) else float("nan")
    print(f"two seeds on the detour, float64 ({time.time() - t0:.0f} s): planned {int((st != 2).sum())}, solved {int(ok.sum())} "
          f"(without the shortcut's seed {int(old.sum())}), choice histogram {np.bincount(choice[ok], minlength=K + 2).tolist()}, "
          f"shortcut seed valid on {int(((bits[:, K] == 0) & (st != 2)).sum())}; on the {int(both.sum())} rows it won and the "
          f"roadmap's seed is valid too: mean trajectory length {mean_len(all_traj[both, K + 1]):.3f} -> {mean_len(all_traj[both, K]):.3f} rad")
    assert int((st != 2).sum()) == DETOUR_PLANNED and int(old.sum()) == DETOUR_GLOBAL_SOLVED
    assert bool(ok[old].all()) and int(ok.sum()) >= DETOUR_GLOBAL_SOLVED
    assert int(ok.sum()) == DETOUR_SHORTCUT_SOLVED
