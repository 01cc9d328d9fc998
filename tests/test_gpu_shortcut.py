"""GPU: ``mpx_franka_shortcut`` (csrc/shortcut_kernel.inc in roadmap.hip) and ``robot.franka_plan_global(shortcut=True)``
against the restatement (tests/float64_shortcut.py: the device's float32 geometry, every configuration judged in float64),
against properties of the device's own output, at the edges of the shape space and through the callers above it.  One
module-scoped fixture: the roadmap and the default shortcut run once on 64 forced-detour rows."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_plan as fp  # noqa: E402
import float64_roadmap as fr  # noqa: E402
import float64_shortcut as fs  # noqa: E402
from float64_collision import SDF_BAR  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_cloud_plan import same  # noqa: E402
from test_gpu_plan import dev, device_scene, prims_of, take  # noqa: E402
from test_plan_host import MIXED  # noqa: E402
from test_roadmap_host import DETOUR_PLAN_SEED, LEFT_OUT_CAP, detour_problems  # noqa: E402
from test_shortcut_host import PARITY_ROWS, POINTS_REFERENCE, TRAJ_REFERENCE, prim_rule  # noqa: E402

pytestmark = pytest.mark.gpu

T = 50
NAMES = ("traj", "status", "points_out", "count_out", "length", "chords", "configs")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(out):
    return tuple(x.cpu().numpy() for x in out)


@pytest.fixture(scope="module")
def detour():
    """The first PARITY_ROWS forced-detour problems: the roadmap with its graph at the planner's seed, the polylines
    ``nodes[path]`` the global planner hands on, and the shortcut at its defaults with the trace."""
    from mpinets_amd import robot, solvers

    torch.cuda.set_device(0)
    qs, qg, lim, scn = detour_problems()
    n = PARITY_ROWS
    qs, qg, scn = qs[:n], qg[:n], {k: v[:n] for k, v in scn.items()}
    cub, cyl = prims_of(scn)
    a, b = _t(qs), _t(qg)
    road = robot.franka_roadmap(a, b, cub, cyl, return_graph=True, seed=DETOUR_PLAN_SEED, limits=lim)
    pts, cnt = solvers._path_vertices(road[4], road[2], road[3])
    out = robot.franka_shortcut(pts, cnt, cub, cyl, return_trace=True)
    return dict(qs=qs, qg=qg, lim=lim, a=a, b=b, cub=cub, cyl=cyl, road=road, pts=pts, cnt=cnt, out=out, host=host(out),
                scene=device_scene(cub, cyl), pts_h=pts.cpu().numpy(), cnt_h=cnt.cpu().numpy())


def test_decisions_and_outputs_against_float64(detour):
    """Row by row against the restatement run on the device's own float32 polylines: where no configuration that decides a
    chord lies within SDF_BAR of its threshold, ``count_out``, ``chords`` and ``configs`` are equal, ``points_out`` is within
    4 x POINTS_REFERENCE and ``traj`` within 4 x TRAJ_REFERENCE (tests/test_shortcut_host.py derives both).  Rows left out
    are capped at LEFT_OUT_CAP; rows without a path are bad rows: status 2, NaN, zero counts."""
    traj, st, po, co, ln, ch, cf = detour["host"]
    cnt = detour["cnt_h"]
    assert np.array_equal(st == 0, cnt >= 2) and np.array_equal(st == 2, cnt == 0)
    bad = st == 2
    assert np.isnan(traj[bad]).all() and np.isnan(po[bad]).all() and np.isnan(ln[bad]).all()
    assert (co[bad] == 0).all() and (ch[bad] == 0).all() and (cf[bad] == 0).all()
    rows = np.flatnonzero(st == 0)
    left, worst_p, worst_t, wrong = 0, 0.0, 0.0, []
    for b in rows:
        valid, m = prim_rule(detour["scene"], b)
        want = fs.shortcut(detour["pts_h"][b, :cnt[b]], valid, T=T, dtype=np.float32, margins=m, band=SDF_BAR)
        if want["in_band"]:
            left += 1
            continue
        n = len(want["points_out"])
        if (co[b], ch[b], cf[b]) != (n, want["chords"], want["configs"]):
            wrong.append((int(b), (int(co[b]), int(ch[b]), int(cf[b])), (n, want["chords"], want["configs"])))
            continue
        assert np.isnan(po[b, n:]).all()
        worst_p = max(worst_p, float(np.abs(po[b, :n].astype(np.float64) - want["points_out"]).max()))
        worst_t = max(worst_t, float(np.abs(traj[b].astype(np.float64) - want["traj"]).max()))
        assert abs(ln[b, 0] - want["length"][0]) <= 1e-6 * want["length"][0] and abs(ln[b, 1] - want["length"][1]) <= 1e-6 * want["length"][1]
    print(f"shortcut against float64 on {len(rows)} rows with a path: {left} left out, disagreeing {wrong}; points_out max "
          f"{worst_p:.3e} (bar {4 * POINTS_REFERENCE:.2e}), traj max {worst_t:.3e} (bar {4 * TRAJ_REFERENCE:.2e}); chords mean "
          f"{ch[rows].mean():.1f}, configurations mean {cf[rows].mean():.0f}, length {ln[rows, 0].mean():.3f} -> {ln[rows, 1].mean():.3f}")
    assert len(rows) >= PARITY_ROWS // 2 and left / len(rows) <= LEFT_OUT_CAP
    assert not wrong
    assert worst_p <= 4 * POINTS_REFERENCE and worst_t <= 4 * TRAJ_REFERENCE


def test_properties_of_the_devices_own_output(detour):
    """The length does not grow; the end points are bit-equal to the input's, in ``points_out`` and in ``traj``; something
    was cut.  After ONE pass every returned vertex is bit-equal to a point of the restated dense polyline, and every returned
    edge that skips a dense point is a chord the kernel must have tested: re-tested here at the stated float32
    configurations and judged in float64 it is free (rows with a configuration within SDF_BAR of its threshold are left
    out, capped at LEFT_OUT_CAP).  An edge between neighbouring dense points is a piece of the input, which is not tested.
    (One pass: a later pass may keep a PIECE of an earlier pass's chord, which no chord test covers as such.)"""
    from mpinets_amd import robot

    traj, st, po, co, ln, ch, cf = detour["host"]
    ok = st == 0
    assert (ln[ok, 1] <= ln[ok, 0] * (1 + 1e-6)).all() and (ln[ok, 1] < 0.99 * ln[ok, 0]).sum() > ok.sum() // 2
    last = np.take_along_axis(po[ok], (co[ok] - 1)[:, None, None].astype(np.int64), 1)[:, 0]
    assert np.array_equal(po[ok][:, 0], detour["qs"][ok]) and np.array_equal(last, detour["qg"][ok])
    assert np.array_equal(traj[ok][:, 0], detour["qs"][ok]) and np.array_equal(traj[ok][:, -1], detour["qg"][ok])
    assert (co[ok] >= 3).all()  # (the cube sits on the straight line)
    _, st1, po1, co1, _ = host(robot.franka_shortcut(detour["pts"], detour["cnt"], detour["cub"], detour["cyl"], passes=1))
    left, tested, blocked = 0, 0, []
    for b in np.flatnonzero(st1 == 0):
        D, _ = fs.densify(detour["pts_h"][b, :detour["cnt_h"][b]], fs.DEFAULTS["points"], np.float32)
        idx = [int(np.flatnonzero((D == v).all(-1))[0]) for v in po1[b, :co1[b]]]  # (fails if a vertex is no dense point)
        assert idx[0] == 0 and idx[-1] == len(D) - 1 and all(j > i for i, j in zip(idx[:-1], idx[1:]))
        _, m = prim_rule(detour["scene"], b)
        for i, j in zip(idx[:-1], idx[1:]):
            if j == i + 1:
                continue
            q = fr.edge_configs(D[i], D[j], fr.pieces(fs.length(D[i], D[j], np.float32), np.float32(0.05), np.float32), np.float32)
            if not len(q):
                continue
            mm = m(q.astype(np.float64))
            tested += 1
            if (np.abs(mm) <= SDF_BAR).any():
                left += 1
            elif (mm < 0).any():
                blocked.append((int(b), i, j))
    print(f"one pass: {tested} returned chords re-tested, {left} in the band, blocked {blocked}")
    assert tested >= 16 and left <= LEFT_OUT_CAP * tested and not blocked


def test_free_line_no_passes_and_halves(detour):
    """Without primitives only the self test can block a chord: most rows come back as one edge, and such a row's ``traj`` is
    the planner's line bit for bit.  ``passes=0`` with a roadmap's ``nodes[path]`` gives that roadmap's ``traj`` bit for bit
    and the input back.  A batch equals its two halves run separately, every output."""
    from mpinets_amd import robot

    pts, cnt = detour["pts"], detour["cnt"]
    tr, st, po, co, ln, ch, cf = host(robot.franka_shortcut(pts, cnt, return_trace=True))
    ok = st == 0
    one = ok & (co == 2)
    assert one.sum() > ok.sum() // 2
    assert np.array_equal(tr[one], fp.line(detour["qs"], detour["qg"], T)[one])
    assert np.array_equal(po[one][:, 0], detour["qs"][one]) and np.array_equal(po[one][:, 1], detour["qg"][one])
    assert (ch[one] == fs.DEFAULTS["fanout"]).all()  # (one level from the first anchor: its last chord reaches the far end)
    kept = robot.franka_shortcut(pts, cnt, detour["cub"], detour["cyl"], return_trace=True, passes=0)
    assert same(kept[0], detour["road"][0])
    found = cnt >= 2
    assert torch.equal(kept[3][found], cnt[found]) and bool((kept[5] == 0).all()) and bool((kept[6] == 0).all())
    V = pts.size(1)
    live = torch.arange(V, device=dev())[None, :] < cnt[:, None]
    assert torch.equal(kept[2][:, :V][live], pts[live]) and bool(torch.isnan(kept[2][:, :V][~live]).all())
    assert torch.equal(kept[4][found][:, 0], kept[4][found][:, 1])
    h = PARITY_ROWS // 2
    for name, whole, lo, hi in zip(NAMES, detour["out"],
                                   robot.franka_shortcut(pts[:h], cnt[:h], *take((detour["cub"], detour["cyl"]), slice(0, h)), return_trace=True),
                                   robot.franka_shortcut(pts[h:], cnt[h:], *take((detour["cub"], detour["cyl"]), slice(h, None)), return_trace=True)):
        assert same(whole, torch.cat([lo, hi])), name


def _guarded(shape, dtype, fill):
    """A tensor with a guard row in front and behind: -> (whole, view)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev())
    return whole, whole[1:-1]


CASES = {
    "B1": dict(B=1), "count2": dict(count=2), "Pin2": dict(Pin=2, P=2), "P=Pin": dict(P=4), "P256": dict(P=256),
    "P100": dict(P=100), "T2": dict(T=2), "T64": dict(T=64), "K1": dict(K=1), "K256": dict(K=256), "passes3": dict(passes=3),
    "duplicates": dict(duplicates=True), "bad_rows": dict(bad=True), "no_primitives": dict(prims=False), "B0": dict(B=0),
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_edges_of_the_shape_space(detour, case):
    """Four detour rows with a path (fewer where the case says so) through the C entry with guard rows around every output:
    the guards keep their fill, and status, ``count_out``, ``chords`` and ``configs`` are the restatement's (rows in the band
    left out), ``points_out`` NaN behind the polyline, the end points bit-equal.  Pin = 2 and count = 2: one edge, nothing
    tested, the planner's line.  Duplicate vertices (one w_i = 0; every vertex equal, L = 0): no division by zero, the row
    comes back as a polyline.  NaN vertex, count 1, count 0, count > Pin: status 2 and NaN outputs, the neighbours untouched."""
    from mpinets_amd import _lib, robot

    c = CASES[case]
    found = np.flatnonzero(detour["cnt_h"] >= 3)[:4]
    B = c.get("B", 4)
    rows = found[:B]
    Pin = c.get("Pin", 4)
    P, T_, K, passes = c.get("P", 64), c.get("T", T), c.get("K", 4), c.get("passes", 2)
    pts = torch.zeros((B, Pin, 7), device=dev())
    cnt = torch.zeros(B, dtype=torch.int32, device=dev())
    for i, b in enumerate(rows):
        n = min(int(detour["cnt_h"][b]), Pin, c.get("count", Pin))
        src = detour["pts"][b, :int(detour["cnt_h"][b])]
        pts[i, :n] = torch.cat([src[:n - 1], src[-1:]])  # (the first n - 1 vertices and the goal)
        cnt[i] = n
    if c.get("duplicates"):
        pts[0, 2] = pts[0, 1]                   # w_1 = 0
        pts[1, :] = pts[1, 0]                   # L = 0
        cnt[0], cnt[1] = min(4, Pin), Pin
        pts[0, 3] = detour["pts"][rows[0], int(detour["cnt_h"][rows[0]]) - 1]
    if c.get("bad"):
        pts[0, 1, 3] = float("nan")
        cnt[1], cnt[2] = 1, Pin + 1
    with_prims = c.get("prims", True)
    cub, cyl = take((detour["cub"], detour["cyl"]), _t(rows)) if B else (detour["cub"], detour["cyl"])
    sc, sr, sl = robot._ik_sphere_table(dev(), False) if with_prims else (None, None, None)
    (wt, traj), (wp, po), (wl, ln) = _guarded((B, T_, 7), torch.float32, 7.0), _guarded((B, P, 7), torch.float32, 7.0), \
        _guarded((B, 2), torch.float32, 7.0)
    (ws, st), (wc, co), (wh, ch), (wf, cf) = (_guarded((B,), torch.int32, -9) for _ in range(4))
    opt = _lib.ShortcutOptions(P, passes, K, 0.05, 8, 1e-4, 0.0, 1)
    p = _lib.ptr
    _lib.call("mpx_franka_shortcut", p(pts), p(cnt), B, Pin, T_, ft.FINGER_OPENING, p(sc), p(sr), p(sl),
              int(sc.size(0)) if with_prims else 0, p(cub.inv_frames) if with_prims else None, p(cub.dims) if with_prims else None,
              cub.dims.size(1) if with_prims else 0, p(cyl.inv_frames) if with_prims else None,
              p(cyl.radii) if with_prims else None, p(cyl.heights) if with_prims else None,
              cyl.radii.size(1) if with_prims else 0, ctypes.byref(opt), p(traj), p(st), p(po), p(co), p(ln), p(ch), p(cf))
    torch.cuda.synchronize()
    for whole, fill in ((wt, 7.0), (wp, 7.0), (wl, 7.0), (ws, -9), (wc, -9), (wh, -9), (wf, -9)):
        assert bool((whole[0] == fill).all()) and bool((whole[-1] == fill).all())
    if B == 0:
        return
    traj, st, po, co, ln, ch, cf = host((traj, st, po, co, ln, ch, cf))
    pts_h, cnt_h = pts.cpu().numpy(), cnt.cpu().numpy()
    want_bad = (cnt_h < 2) | (cnt_h > Pin) | ~np.isfinite(np.where((np.arange(Pin)[None, :] < cnt_h[:, None])[:, :, None], pts_h, 0)).all((1, 2))
    assert np.array_equal(st == 2, want_bad) and np.array_equal(st == 0, ~want_bad)
    assert np.isnan(traj[want_bad]).all() and np.isnan(po[want_bad]).all() and np.isnan(ln[want_bad]).all()
    assert (co[want_bad] == 0).all() and (ch[want_bad] == 0).all() and (cf[want_bad] == 0).all()
    if c.get("bad"):
        assert want_bad.tolist() == [True, True, True, False]
    scene = device_scene(cub, cyl)
    for i in np.flatnonzero(~want_bad):
        n = int(co[i])
        assert 2 <= n <= P
        assert not np.isnan(po[i, :n]).any() and np.isnan(po[i, n:]).all() and not np.isnan(traj[i]).any()
        assert np.array_equal(po[i, 0], pts_h[i, 0]) and np.array_equal(po[i, n - 1], pts_h[i, cnt_h[i] - 1])
        assert np.array_equal(traj[i, 0], pts_h[i, 0]) and np.array_equal(traj[i, -1], pts_h[i, cnt_h[i] - 1])
        assert ln[i, 1] <= ln[i, 0] * (1 + 1e-6)
        if with_prims:
            valid, m = prim_rule(scene, i)
        else:
            valid = fr.franka_validity(None, 1e-4, True, 1e-4)
            m = None
        want = fs.shortcut(pts_h[i, :cnt_h[i]], valid, T=T_, dtype=np.float32, margins=m, band=SDF_BAR, points=P, passes=passes,
                           fanout=K)
        if want["in_band"]:
            print(f"{case}: row {i} left out (a configuration in the band)")
            continue
        assert (n, int(ch[i]), int(cf[i])) == (len(want["points_out"]), want["chords"], want["configs"]), (case, i)
        assert np.abs(po[i, :n].astype(np.float64) - want["points_out"]).max() <= 4 * POINTS_REFERENCE
        if n == 2:
            assert np.array_equal(traj[i], fp.line(pts_h[i, :1], pts_h[i, cnt_h[i] - 1:cnt_h[i]], T_)[0])
    if c.get("Pin") == 2 or c.get("count") == 2:
        assert (co == 2).all() and (ch == 0).all() and (ln[:, 0] == ln[:, 1]).all()
    if T_ == 2:
        ok = ~want_bad
        assert np.array_equal(traj[ok][:, 0], pts_h[ok][:, 0])
    if c.get("duplicates"):
        assert st.tolist() == [0, 0, 0, 0] and ln[1, 0] == 0 and ln[1, 1] == 0 and co[1] >= 2


def test_global_planner_with_the_shortcut(detour):
    """``franka_plan_global(shortcut=True)`` on the 64 detour rows: candidates 0 .. 7 and the roadmap's seed (now candidate 9)
    are bit-equal to ``franka_plan_global()``'s 0 .. 8; a row solved by a candidate below 8 comes back identical; the solved
    set is a superset; a row whose choice is 9 returns what ``franka_plan_global()`` returns with choice 8; the shortcut's
    seed is what ``franka_shortcut`` gives on the roadmap's ``nodes[path]`` (a dict of options reaches it)."""
    from mpinets_amd import robot

    kw = dict(seed=DETOUR_PLAN_SEED, limits=detour["lim"], return_all=True)
    a, b, cub, cyl = detour["a"], detour["b"], detour["cub"], detour["cyl"]
    old = robot.franka_plan_global(a, b, cub, cyl, **kw)
    new = robot.franka_plan_global(a, b, cub, cyl, shortcut=True, **kw)
    K = old[3].shape[1] - 1
    assert new[3].shape[1] == K + 2 and torch.equal(new[5], old[5])
    assert same(new[3][:, :K], old[3][:, :K]) and torch.equal(new[4][:, :K], old[4][:, :K])
    assert same(new[3][:, K + 1], old[3][:, K]) and torch.equal(new[4][:, K + 1], old[4][:, K])
    low = (old[1] == 0) & (old[2] < K)
    assert same(new[0][low], old[0][low]) and torch.equal(new[2][low], old[2][low]) and bool((new[1][low] == 0).all())
    assert bool((new[1][old[1] == 0] == 0).all()) and torch.equal(new[1] == 2, old[1] == 2)
    by_old_seed = (new[1] == 0) & (new[2] == K + 1)
    assert bool((old[2][by_old_seed] == K).all()) and same(new[0][by_old_seed], old[0][by_old_seed])
    won = (new[1] == 0) & (new[2] == K)
    print(f"franka_plan_global on {len(a)} detour rows: solved {int((old[1] == 0).sum())}, with shortcut {int((new[1] == 0).sum())}; "
          f"choice histogram {torch.bincount(new[2][new[1] == 0], minlength=K + 2).tolist()} (was "
          f"{torch.bincount(old[2][old[1] == 0], minlength=K + 1).tolist()})")
    assert int(won.sum()) > 0  # (the shorter seed does survive the optimiser and the judge on some rows)
    ln = detour["out"][4]
    assert bool((ln[won][:, 1] <= ln[won][:, 0]).all())
    one = robot.franka_plan_global(a, b, cub, cyl, shortcut=dict(passes=0), **kw)  # no passes: the roadmap's seed, twice
    assert same(one[3][:, K], one[3][:, K + 1]) and same(one[0], old[0])


def test_problem_batches_can_ask_for_the_shortcut():
    """``make_problem_batch(expert_from="roadmap", expert_shortcut=True)``: opt-in; the flag off is the call without it;
    everything but the demonstrations is unchanged, every row solved without it is solved with it."""
    from mpinets_amd import scenes

    torch.cuda.set_device(0)
    kw = dict(seed=4, kinds=MIXED, M1=40, M2=16, device_clouds=True, collision_free=True, expert=True, expert_from="roadmap")
    base = scenes.make_problem_batch(16, **kw)
    off = scenes.make_problem_batch(16, expert_shortcut=False, **kw)
    on = scenes.make_problem_batch(16, expert_shortcut=True, **kw)
    assert set(base) == set(off) == set(on)
    for k in base:
        if torch.is_tensor(base[k]):
            assert same(base[k], off[k]), k
            if k not in ("global_solutions", "expert_valid"):
                assert same(base[k], on[k]), k
    assert bool(on["expert_valid"][base["expert_valid"]].all())
    assert bool(torch.isnan(on["global_solutions"][~on["expert_valid"]]).all())
