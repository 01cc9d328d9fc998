"""GPU: ``mpx_gripper_shortcut`` (csrc/gripper_shortcut.hip: shortcut_kernel.inc over the gripper's metric, edge pose and
validity, then gripper_poses.inc), ``robot.gripper_plan`` and ``make_problem_batch(..., hybrid_shortcut=True)`` against the
restatement (tests/float64_gripper_shortcut.py: the device's float32 geometry, every pose judged in float64), against
properties of the device's own output, at the edges of the shape space and through the callers above it.  One module-scoped
fixture: the device's own gripper roadmap with its graph on the 64 wall and the 64 cylinder problems at ROADMAP_SEED, the
polylines ``nodes[path]`` and the default shortcut with the trace.

The checks are functions of a ``form`` (how the entry is called and how a pose is judged), so that
tests/test_gpu_gripper_shortcut_cloud.py runs the same ones on the cloud form."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_gripper_roadmap as fg  # noqa: E402
import float64_gripper_shortcut as fgs  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_gripper_roadmap import prims, same  # noqa: E402
from test_gripper_roadmap_host import GRIPPER_BAND, LEFT_OUT_CAP  # noqa: E402
from test_gripper_shortcut_host import POINTS_REFERENCE, POSES_REFERENCE  # noqa: E402

pytestmark = pytest.mark.gpu

B, W = 64, 8
SEED = fg.ROADMAP_SEED
KINDS = ("wall", "cylinder")
NAMES = ("poses", "status", "points_out", "count_out", "length", "chords", "configs")
POINTS_BAR, POSES_BAR = 4 * POINTS_REFERENCE, 4 * POSES_REFERENCE
F32 = np.float32


def dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(out):
    return tuple(x.cpu().numpy() for x in out)


class PrimitiveForm:
    """``mpx_gripper_shortcut`` on one scenario: the device call and the restatement's rule of a row."""
    band = GRIPPER_BAND

    def __init__(self, kind):
        self.kind = kind
        self.cub, self.cyl, self.scene = prims(kind)

    def roadmap(self, sp, gp, **kw):
        from mpinets_amd import robot

        return robot.gripper_roadmap(sp, gp, self.cub, self.cyl, W=W, seed=SEED, return_graph=True, **kw)

    def _rows(self, rows):
        from mpinets_amd.geometry import TorchCuboids, TorchCylinders

        cub = None if self.cub is None else TorchCuboids(self.cub.centers[rows], self.cub.dims[rows], self.cub.quats[rows])
        cyl = None if self.cyl is None else TorchCylinders(self.cyl.centers[rows], self.cyl.radii[rows], self.cyl.heights[rows],
                                                           self.cyl.quats[rows])
        return cub, cyl

    def shortcut(self, pts, cnt, rows=slice(None), **kw):
        from mpinets_amd import robot

        cub, cyl = self._rows(rows)
        return robot.gripper_shortcut(pts, cnt, cub, cyl, W=kw.pop("W", W), **kw)

    def rule(self, b, clearance=0.0):
        return fgs.prim_rule(None if self.scene is None else {k: v[b:b + 1] for k, v in self.scene.items()}, clearance)

    def c_call(self, rows, with_env, pts, cnt, Bn, Pin, Wn, goal, opt, outs):
        """The C entry on the scenario's rows ``rows`` (``with_env`` False: S = 0, no primitives)."""
        from mpinets_amd import _lib, robot

        p = _lib.ptr
        cub, cyl = self._rows(rows) if with_env else (None, None)
        sc, sr, sl = robot._ik_sphere_table(dev(), False) if with_env else (None, None, None)
        _lib.call("mpx_gripper_shortcut", p(pts), p(cnt), Bn, Pin, Wn, p(goal), ft.FINGER_OPENING, p(sc), p(sr), p(sl),
                  int(sc.size(0)) if with_env else 0, p(cub.inv_frames) if cub is not None else None,
                  p(cub.dims) if cub is not None else None, cub.dims.size(1) if cub is not None else 0,
                  p(cyl.inv_frames) if cyl is not None else None, p(cyl.radii) if cyl is not None else None,
                  p(cyl.heights) if cyl is not None else None, cyl.radii.size(1) if cyl is not None else 0, ctypes.byref(opt),
                  *[p(o) for o in outs])

    def rule_without_env(self):
        return fgs.prim_rule(None)


def run_form(form, sp, gp):
    """-> dict: the roadmap with its graph, the polylines, the default shortcut with the trace (tensors and numpy)."""
    from mpinets_amd import solvers

    a, b = _t(sp), _t(gp)
    road = form.roadmap(a, b)
    pts, cnt = solvers._path_vertices(road[4], road[2], road[3])
    out = form.shortcut(pts, cnt, goal_pose=b, return_trace=True)
    return dict(form=form, sp=sp, gp=gp, a=a, b=b, road=road, pts=pts, cnt=cnt, out=out, host=host(out), pts_h=pts.cpu().numpy(),
                cnt_h=cnt.cpu().numpy())


@pytest.fixture(scope="module")
def runs():
    torch.cuda.set_device(0)
    sp, gp = fg.problems(B)
    return {kind: run_form(PrimitiveForm(kind), sp, gp) for kind in KINDS}


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def points_differ(got, want):
    """Largest difference of two polylines [n,7]: positions, and quaternions up to their sign."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return max(float(np.abs(got[:, :3] - want[:, :3]).max()), float(fgs.same_rotation(got[:, 3:], want[:, 3:]).max()))


def check_row(rule, band, polyline, goal, got, Wn=W, **options):
    po_, pt_, co_, ln_, ch_, cf_ = got
    valid, m = rule
    want = fgs.shortcut(polyline, valid, W=Wn, goal_pose=goal, dtype=F32, margins=m, band=band, **options)
    if want["in_band"]:
        return "left"
    n = len(want["points_out"])
    if (int(co_), int(ch_), int(cf_)) != (n, want["chords"], want["configs"]):
        return (int(co_), int(ch_), int(cf_)), (n, want["chords"], want["configs"])
    assert not np.isnan(pt_[:n]).any() and np.isnan(pt_[n:]).all()
    for k in (0, 1):
        assert abs(float(ln_[k]) - float(want["length"][k])) <= 1e-6 * float(want["length"][k]) + 1e-30
    return points_differ(pt_[:n], want["points_out"]), float(np.abs(po_.astype(np.float64) - want["poses"]).max())


def check_against_restatement(run, clearance=0.0):
    """Row by row against the restatement run on the device's own float32 polylines: where no pose that decides a chord lies
    within the band of its threshold (and no chord's piece count is fragile), ``count_out``, ``chords`` and ``configs`` are
    equal, ``points_out`` is within 4 x POINTS_REFERENCE up to the sign of q, ``poses`` within 4 x POSES_REFERENCE and
    ``length`` within 1e-6 relative.  Rows left out are capped at LEFT_OUT_CAP; rows without a path are bad rows: status 2,
    NaN, zero counts."""
    form = run["form"]
    po, st, pt, co, ln, ch, cf = run["host"]
    cnt = run["cnt_h"]
    assert np.array_equal(st == 0, cnt >= 2) and np.array_equal(st == 2, cnt == 0)
    bad = st == 2
    assert np.isnan(po[bad]).all() and np.isnan(pt[bad]).all() and np.isnan(ln[bad]).all()
    assert (co[bad] == 0).all() and (ch[bad] == 0).all() and (cf[bad] == 0).all()
    rows = np.flatnonzero(st == 0)
    left, worst_p, worst_t, wrong = 0, 0.0, 0.0, []
    for b in rows:
        res = check_row(form.rule(b), form.band, run["pts_h"][b, :cnt[b]], run["gp"][b], (po[b], pt[b], co[b], ln[b], ch[b], cf[b]))
        if res == "left":
            left += 1
        elif isinstance(res[0], tuple):
            wrong.append((int(b),) + res)
        else:
            worst_p, worst_t = max(worst_p, res[0]), max(worst_t, res[1])
    print(f"{form.kind}: gripper shortcut against float64 on {len(rows)} rows with a path: {left} left out, disagreeing {wrong}; "
          f"points_out max {worst_p:.3e} (bar {POINTS_BAR:.2e}), poses max {worst_t:.3e} (bar {POSES_BAR:.2e}); chords mean "
          f"{ch[rows].mean():.1f}, interior poses mean {cf[rows].mean():.0f}, length {ln[rows, 0].mean():.3f} -> {ln[rows, 1].mean():.3f}")
    assert len(rows) >= 0.9 * B and left / len(rows) <= LEFT_OUT_CAP
    assert not wrong
    assert worst_p <= POINTS_BAR and worst_t <= POSES_BAR


def check_properties(run):
    """The length does not grow and most rows get shorter; the end vertices are bit-equal to the input's; rows 0-2 of the last
    pose are ``goal_pose``'s bit for bit and row 3 of every pose is (0, 0, 0, 1).  After ONE pass every returned vertex is
    within the bar of a point of the restated dense polyline, in rising order, and every returned edge that skips a dense point
    is a chord the kernel must have tested: re-tested here at the stated float32 poses and judged in float64 it is free (chords
    with a pose in the band, or a fragile piece count, are left out, capped at LEFT_OUT_CAP).  The guide poses themselves are
    NOT asserted valid: a pose between two tested poses may graze; poses guide, the follower's judge decides."""
    form = run["form"]
    po, st, pt, co, ln, ch, cf = run["host"]
    ok = st == 0
    assert (ln[ok, 1] <= ln[ok, 0] * (1 + 1e-6)).all() and (ln[ok, 1] < 0.99 * ln[ok, 0]).sum() >= 0.9 * ok.sum()
    first = run["pts_h"][ok][:, 0]
    last_in = np.take_along_axis(run["pts_h"][ok], (run["cnt_h"][ok] - 1)[:, None, None].astype(np.int64), 1)[:, 0]
    last = np.take_along_axis(pt[ok], (co[ok] - 1)[:, None, None].astype(np.int64), 1)[:, 0]
    assert np.array_equal(pt[ok][:, 0], first) and np.array_equal(last, last_in)
    assert np.array_equal(po[ok][:, -1, :3], run["gp"][ok][:, :3])
    assert np.array_equal(po[ok][:, :, 3], np.broadcast_to(F32([0, 0, 0, 1]), po[ok][:, :, 3].shape))
    assert (co[ok] >= 3).all()  # (the obstacle sits between every start and its goal)
    _, st1, pt1, co1, _ = host(form.shortcut(run["pts"], run["cnt"], goal_pose=run["b"], passes=1))
    left, tested, blocked = 0, 0, []
    for b in np.flatnonzero(st1 == 0):
        D, _ = fgs.densify(run["pts_h"][b, :run["cnt_h"][b]], fgs.DEFAULTS["points"], dtype=F32)
        idx, at = [], 0
        for v in pt1[b, :co1[b]]:
            d = np.maximum(np.abs(D[at:, :3].astype(np.float64) - v[:3]).max(-1), fgs.same_rotation(D[at:, 3:], v[None, 3:]))
            j = at + int(np.argmin(d))
            assert d[j - at] <= POINTS_BAR, (b, len(idx))
            idx.append(j)
            at = j + 1
        assert idx[0] == 0 and idx[-1] == len(D) - 1
        _, m = form.rule(b)
        for i, j in zip(idx[:-1], idx[1:]):
            if j == i + 1:
                continue
            n, fragile = fgs.chord_pieces(fgs.length(D[i], D[j], dtype=F32), fgs.DEFAULTS["resolution"], F32)
            q = fg.edge_poses(D[i], D[j], n, F32)
            if not len(q):
                continue
            mm = m(q.astype(np.float64))
            tested += 1
            if fragile or (np.abs(mm) <= form.band).any():
                left += 1
            elif (mm < 0).any():
                blocked.append((int(b), i, j))
    print(f"{form.kind}: one pass: {tested} returned chords re-tested, {left} in the band, blocked {blocked}")
    assert tested >= 16 and left <= LEFT_OUT_CAP * tested and not blocked


def check_identities(run):
    """``passes=0`` on ``nodes[path]`` with the roadmap's goal gives the roadmap's ``poses`` bit for bit and the input back; a
    batch equals its two halves run separately, every output; negating every input quaternion of the rows leaves
    ``count_out`` / ``chords`` / ``configs`` equal and ``poses`` within the bar."""
    form, pts, cnt, goal = run["form"], run["pts"], run["cnt"], run["b"]
    kept = form.shortcut(pts, cnt, goal_pose=goal, return_trace=True, passes=0)
    assert same(kept[0], run["road"][0])
    found = cnt >= 2
    assert torch.equal(kept[3][found], cnt[found]) and bool((kept[5] == 0).all()) and bool((kept[6] == 0).all())
    V = pts.size(1)
    live = torch.arange(V, device=dev())[None, :] < cnt[:, None]
    assert torch.equal(kept[2][:, :V][live], pts[live]) and bool(torch.isnan(kept[2][:, :V][~live]).all())
    assert torch.equal(kept[4][found][:, 0], kept[4][found][:, 1])
    h = B // 2
    lo = form.shortcut(pts[:h], cnt[:h], rows=slice(0, h), goal_pose=goal[:h], return_trace=True)
    hi = form.shortcut(pts[h:], cnt[h:], rows=slice(h, None), goal_pose=goal[h:], return_trace=True)
    for name, whole, a, b in zip(NAMES, run["out"], lo, hi):
        assert same(whole, torch.cat([a, b])), name
    flipped = pts.clone()
    flipped[:, :, 3:] = -flipped[:, :, 3:]
    neg = form.shortcut(flipped, cnt, goal_pose=goal, return_trace=True)
    for i in (1, 3, 5, 6):
        assert torch.equal(neg[i], run["out"][i]), NAMES[i]
    ok = run["out"][1] == 0
    assert float((neg[0][ok] - run["out"][0][ok]).abs().max()) <= POSES_BAR
    assert float((neg[4][ok] - run["out"][4][ok]).abs().max()) <= 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_decisions_and_outputs_against_float64(runs, kind):
    check_against_restatement(runs[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_properties_of_the_devices_own_output(runs, kind):
    check_properties(runs[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_no_passes_halves_and_negated_quaternions(runs, kind):
    check_identities(runs[kind])


def test_gripper_plan_composes_the_two(runs):
    """``gripper_plan(shortcut=None)`` is ``gripper_roadmap``; with the default ``shortcut=True`` its poses are
    ``gripper_shortcut``'s on the roadmap's ``nodes[path]`` at max(64, nodes) points, its status the roadmap's, rows without
    a path NaN; a dict of options reaches the shortcut."""
    from mpinets_amd import robot

    run = runs["wall"]
    form, a, b = run["form"], run["a"], run["b"]
    off = robot.gripper_plan(a, b, form.cub, form.cyl, W=W, seed=SEED, shortcut=None)
    assert len(off) == 2 and same(off[0], run["road"][0]) and torch.equal(off[1], run["road"][1])
    on = robot.gripper_plan(a, b, form.cub, form.cyl, W=W, seed=SEED, return_length=True)
    assert same(on[0], run["out"][0]) and torch.equal(on[1], run["road"][1]) and same(on[2], run["out"][4])
    assert bool(torch.isnan(on[0][on[1] != 0]).all()) and not bool(torch.isnan(on[0][on[1] == 0]).any())
    none = robot.gripper_plan(a, b, form.cub, form.cyl, W=W, seed=SEED, shortcut=dict(passes=0))
    assert same(none[0], run["road"][0])


# ---- the edges of the shape space ------------------------------------------------------------------------------------------------
def _guarded(shape, dtype, fill):
    """A tensor with a guard row in front and behind: -> (whole, view)."""
    whole = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device=dev())
    return whole, whole[1:-1]


CASES = {
    "B1": dict(B=1), "B0": dict(B=0), "count2": dict(count=2), "Pin2": dict(Pin=2, P=2), "P=Pin": dict(P=4), "P100": dict(P=100),
    "P256": dict(P=256), "W1": dict(W=1), "W64": dict(W=64), "K1": dict(K=1), "K256": dict(K=256), "passes3": dict(passes=3),
    "duplicates": dict(duplicates=True), "negative_dot": dict(negative_dot=True), "bad_nan_count1": dict(bad="a"),
    "bad_count_norm": dict(bad="b"), "no_environment": dict(env=False), "goal_NULL": dict(goal=False),
}


def check_edge_case(run, case, c=None):
    """Four rows with a path (fewer where the case says so) through the C entry with guard rows around every output: the
    guards keep their fill, and status, ``count_out``, ``chords`` and ``configs`` are the restatement's (rows in the band left
    out), ``points_out`` NaN behind the polyline and within the bar, ``poses`` within the bar, the end vertices bit-equal, the
    last pose the goal's rows (``goal_pose`` NULL: the last vertex's own frame).  Pin = 2 and count = 2: one edge, nothing
    tested.  Duplicate vertices (one w_i = 0; every vertex equal, L = 0): no division by zero.  A NaN vertex, count 1, count >
    Pin, a quaternion of norm 1.1: status 2 and NaN outputs, the neighbours untouched."""
    from mpinets_amd import _lib

    form = run["form"]
    c = CASES[case] if c is None else c
    found = np.flatnonzero(run["cnt_h"] >= 3)[:4]
    Bn = c.get("B", 4)
    rows = found[:Bn]
    Pin = c.get("Pin", 4)
    P, Wn, K, passes = c.get("P", 64), c.get("W", W), c.get("K", 4), c.get("passes", 2)
    pts = torch.zeros((Bn, Pin, 7), device=dev())
    pts[:, :, 6] = 1.0  # (rows behind count are not read; a unit quaternion anyway)
    cnt = torch.zeros(Bn, dtype=torch.int32, device=dev())
    for i, b in enumerate(rows):
        full = int(run["cnt_h"][b])
        n = min(full, Pin, c.get("count", Pin))
        src = run["pts"][b, :full]
        pts[i, :n] = torch.cat([src[:n - 1], src[-1:]])  # (the first n - 1 vertices and the goal)
        cnt[i] = n
    if c.get("duplicates"):
        pts[0, 3] = pts[0, int(cnt[0]) - 1]
        pts[0, 2] = pts[0, 1]                   # w_1 = 0
        pts[1, :] = pts[1, 0]                   # L = 0
        cnt[0], cnt[1] = 4, Pin
    if c.get("negative_dot"):
        for i in range(Bn):
            pts[i, int(cnt[i]) - 1, 3:] = -pts[i, int(cnt[i]) - 1, 3:]  # dot(q_before, q_goal) < 0: the sigma = -1 nlerp
        assert float((pts[0, 0, 3:] * pts[0, int(cnt[0]) - 1, 3:]).sum()) < 0
    if c.get("bad") == "a":
        pts[0, 1, 4] = float("nan")
        cnt[1] = 1
    if c.get("bad") == "b":
        cnt[0] = Pin + 1
        pts[1, 1, 3:] = pts[1, 1, 3:] * 1.1
    with_env, with_goal = c.get("env", True), c.get("goal", True)
    goal = run["b"][_t(rows)].contiguous() if with_goal and Bn else None
    (wq, po), (wp, pt), (wl, ln) = _guarded((Bn, Wn, 4, 4), torch.float32, 7.0), _guarded((Bn, P, 7), torch.float32, 7.0), \
        _guarded((Bn, 2), torch.float32, 7.0)
    (ws, st), (wc, co), (wh, ch), (wf, cf) = (_guarded((Bn,), torch.int32, -9) for _ in range(4))
    opt = _lib.GripperShortcutOptions(P, passes, K, 0.01, 0.12, 1e-4, 0.0, 1)
    form.c_call(_t(rows), with_env, pts, cnt, Bn, Pin, Wn, goal, opt, (po, st, pt, co, ln, ch, cf))
    torch.cuda.synchronize()
    for whole, fill in ((wq, 7.0), (wp, 7.0), (wl, 7.0), (ws, -9), (wc, -9), (wh, -9), (wf, -9)):
        assert bool((whole[0] == fill).all()) and bool((whole[-1] == fill).all())
    if Bn == 0:
        return
    po, st, pt, co, ln, ch, cf = host((po, st, pt, co, ln, ch, cf))
    pts_h, cnt_h = pts.cpu().numpy(), cnt.cpu().numpy()
    want_bad = np.array([fgs.bad_row(pts_h[i], int(cnt_h[i])) for i in range(Bn)])
    assert np.array_equal(st == 2, want_bad) and np.array_equal(st == 0, ~want_bad)
    assert np.isnan(po[want_bad]).all() and np.isnan(pt[want_bad]).all() and np.isnan(ln[want_bad]).all()
    assert (co[want_bad] == 0).all() and (ch[want_bad] == 0).all() and (cf[want_bad] == 0).all()
    if c.get("bad"):
        assert want_bad.tolist() == [True, True, False, False]
    goal_h = None if goal is None else goal.cpu().numpy()
    for i in np.flatnonzero(~want_bad):
        n = int(co[i])
        assert 2 <= n <= P
        assert not np.isnan(pt[i, :n]).any() and np.isnan(pt[i, n:]).all() and not np.isnan(po[i]).any()
        assert np.array_equal(pt[i, 0], pts_h[i, 0]) and np.array_equal(pt[i, n - 1], pts_h[i, cnt_h[i] - 1])
        assert np.array_equal(po[i, :, 3], np.tile(F32([0, 0, 0, 1]), (Wn, 1)))
        if with_goal:
            assert np.array_equal(po[i, -1, :3], goal_h[i, :3])
        else:  # the last vertex's own frame: the header's R, every product and sum rounded on its own
            assert np.array_equal(po[i, -1], fg.pose_matrix(pts_h[i, cnt_h[i] - 1:cnt_h[i]])[0])
        rule = form.rule(int(rows[i])) if with_env else form.rule_without_env()
        res = check_row(rule, form.band, pts_h[i, :cnt_h[i]], None if goal_h is None else goal_h[i],
                        (po[i], pt[i], co[i], ln[i], ch[i], cf[i]), Wn, points=P, passes=passes, fanout=K)
        if res == "left":
            print(f"{case}: row {i} left out (a pose in the band)")
            continue
        assert not isinstance(res[0], tuple), (case, i, res)
        assert res[0] <= POINTS_BAR and res[1] <= POSES_BAR, (case, i, res)
    if c.get("Pin") == 2 or c.get("count") == 2:
        assert (co == 2).all() and (ch == 0).all() and (cf == 0).all() and (ln[:, 0] == ln[:, 1]).all()
    if c.get("duplicates"):
        assert st.tolist() == [0, 0, 0, 0] and ln[1, 0] == 0 and ln[1, 1] == 0 and co[1] >= 2
        assert np.array_equal(pt[1, :co[1]], np.repeat(pts_h[1, :1], co[1], 0))


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_edges_of_the_shape_space(runs, case):
    check_edge_case(runs["wall"], case)


# ---- the callers -----------------------------------------------------------------------------------------------------------------
def test_make_problem_batch_with_the_shortcut_guide():
    """``make_problem_batch(hybrid_guide="gripper", hybrid_shortcut=True)`` at B = 16: opt-in; the flag off is the call without
    it; only ``hybrid_guide_poses``, ``hybrid_solutions``, ``hybrid_valid`` and ``hybrid_target_pose`` may differ; rows that
    are not ``hybrid_valid`` are NaN; the guide is NaN exactly where the roadmap found no path.  ``hybrid_valid`` under both
    guides is printed, not asserted (profiles/gripper_shortcut_timing.md)."""
    from mpinets_amd import scenes

    torch.cuda.set_device(0)
    kw = dict(seed=3, collision_free=True, expert=True, hybrid=True, hybrid_guide="gripper")
    base = scenes.make_problem_batch(16, **kw)
    off = scenes.make_problem_batch(16, hybrid_shortcut=False, **kw)
    on = scenes.make_problem_batch(16, hybrid_shortcut=True, **kw)
    some = scenes.make_problem_batch(16, hybrid_shortcut=dict(passes=0), **kw)
    assert set(base) == set(off) == set(on)
    for k in base:
        assert same(base[k], off[k]), k
        if k not in ("hybrid_guide_poses", "hybrid_solutions", "hybrid_valid", "hybrid_target_pose"):
            assert same(base[k], on[k]), k
        assert same(base[k], some[k]), k  # no passes: the roadmap's own poses, so the same batch
    gst = on["hybrid_guide_status"]
    assert bool(torch.isnan(on["hybrid_guide_poses"][gst != 0]).all()) and not bool(torch.isnan(on["hybrid_guide_poses"][gst == 0]).any())
    assert bool(torch.isnan(on["hybrid_solutions"][~on["hybrid_valid"]]).all())
    assert not bool((on["hybrid_valid"] & ((gst != 0) | ~on["expert_valid"])).any())
    found = gst == 0
    assert torch.equal(on["hybrid_guide_poses"][found][:, -1], base["hybrid_guide_poses"][found][:, -1])  # the goal, bit for bit
    moved = int((on["hybrid_guide_poses"][found] != base["hybrid_guide_poses"][found]).flatten(1).any(1).sum())
    print(f"hybrid_valid of 16 (expert_valid {int(on['expert_valid'].sum())}, gripper paths {int(found.sum())}, guides the shortcut "
          f"changed {moved}: a one-edge path has nothing to cut): roadmap guide {int(base['hybrid_valid'].sum())}, shortcut guide "
          f"{int(on['hybrid_valid'].sum())}")
