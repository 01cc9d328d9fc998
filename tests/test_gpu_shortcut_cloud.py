"""GPU: ``mpx_franka_shortcut_cloud`` (csrc/shortcut_kernel.inc in roadmap_cloud.hip), ``robot.franka_plan_global_cloud(
shortcut=True)`` and the callers above it.  The restatement (tests/float64_shortcut.py) judges by
tests/float64_roadmap_cloud.py's rule on the field the DEVICE built, copied to the host, so these tests judge the shortcut
kernel and not the field build.  One module-scoped fixture: the 24 forced-detour rows drawn as a cloud."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_plan as fcp  # noqa: E402
import float64_plan as fp  # noqa: E402
import float64_shortcut as fs  # noqa: E402
from test_gpu_cloud_plan import build_field, dev, grid_dict, same, up  # noqa: E402
from test_roadmap_cloud_host import BAND, DETOUR_PLAN_SEED, LEFT_OUT_CAP, POINT_RADIUS  # noqa: E402
from test_shortcut_host import CLOUD_ROWS, POINTS_REFERENCE, TRAJ_REFERENCE, field_rule  # noqa: E402

pytestmark = pytest.mark.gpu

T = 50
NAMES = ("traj", "status", "points_out", "count_out", "length", "chords", "configs")


def host(out):
    return tuple(x.cpu().numpy() for x in out)


@pytest.fixture(scope="module")
def detour():
    from mpinets_amd import robot, solvers

    torch.cuda.set_device(0)
    qs, qg, lim, cloud, _ = fcp.detour_problems(CLOUD_ROWS)
    a, b, c = up(qs), up(qg), up(cloud)
    field = build_field(c, POINT_RADIUS)
    kw = dict(field=field, point_radius=POINT_RADIUS)
    road = robot.franka_roadmap_cloud(a, b, c, return_graph=True, seed=DETOUR_PLAN_SEED, limits=lim, **kw)
    pts, cnt = solvers._path_vertices(road[4], road[2], road[3])
    out = robot.franka_shortcut_cloud(pts, cnt, c, return_trace=True, **kw)
    return dict(qs=qs, qg=qg, lim=lim, a=a, b=b, c=c, field=field, kw=kw, road=road, pts=pts, cnt=cnt, out=out, host=host(out),
                values=field.values.cpu().numpy(), grid=grid_dict(field.grid), pts_h=pts.cpu().numpy(), cnt_h=cnt.cpu().numpy())


def test_decisions_and_outputs_against_float64(detour):
    """Row by row against the restatement on the device's own polylines and field: where no configuration that decides a
    chord has a sphere, or a self distance, within BAND of its threshold (tests/test_roadmap_cloud_host.py: 4.4e-7 m),
    ``count_out``, ``chords`` and ``configs`` are equal, ``points_out`` within 4 x POINTS_REFERENCE and ``traj`` within 4 x
    TRAJ_REFERENCE.  Rows left out are capped at LEFT_OUT_CAP.  The properties of the output hold on every row."""
    traj, st, po, co, ln, ch, cf = detour["host"]
    cnt = detour["cnt_h"]
    assert np.array_equal(st == 0, cnt >= 2) and np.array_equal(st == 2, cnt == 0)
    bad = st == 2
    assert np.isnan(traj[bad]).all() and np.isnan(po[bad]).all() and (co[bad] == 0).all() and (ch[bad] == 0).all()
    rows = np.flatnonzero(st == 0)
    left, worst_p, worst_t, wrong = 0, 0.0, 0.0, []
    for b in rows:
        valid, m = field_rule(detour["values"][b], detour["grid"])
        want = fs.shortcut(detour["pts_h"][b, :cnt[b]], valid, T=T, dtype=np.float32, margins=m, band=BAND)
        n = int(co[b])
        assert ln[b, 1] <= ln[b, 0] * (1 + 1e-6) and np.isnan(po[b, n:]).all() and not np.isnan(po[b, :n]).any()
        assert np.array_equal(po[b, 0], detour["qs"][b]) and np.array_equal(po[b, n - 1], detour["qg"][b])
        assert np.array_equal(traj[b, 0], detour["qs"][b]) and np.array_equal(traj[b, -1], detour["qg"][b])
        if want["in_band"]:
            left += 1
            continue
        if (n, ch[b], cf[b]) != (len(want["points_out"]), want["chords"], want["configs"]):
            wrong.append((int(b), (n, int(ch[b]), int(cf[b])), (len(want["points_out"]), want["chords"], want["configs"])))
            continue
        worst_p = max(worst_p, float(np.abs(po[b, :n].astype(np.float64) - want["points_out"]).max()))
        worst_t = max(worst_t, float(np.abs(traj[b].astype(np.float64) - want["traj"]).max()))
    print(f"cloud shortcut against float64 on {len(rows)} of {CLOUD_ROWS} rows with a path: {left} left out, disagreeing {wrong}; "
          f"points_out max {worst_p:.3e}, traj max {worst_t:.3e}; chords mean {ch[rows].mean():.1f}, configurations mean "
          f"{cf[rows].mean():.0f}, length {ln[rows, 0].mean():.3f} -> {ln[rows, 1].mean():.3f}")
    assert len(rows) >= 6 and left / len(rows) <= LEFT_OUT_CAP
    assert not wrong
    assert worst_p <= 4 * POINTS_REFERENCE and worst_t <= 4 * TRAJ_REFERENCE


def test_no_cloud_no_passes_and_halves(detour):
    """Without a cloud and without a field only the self test can block a chord, and the output equals ``franka_shortcut``'s
    without primitives, every output; a one-edge row's ``traj`` is the planner's line bit for bit.  ``passes=0`` gives
    ``franka_roadmap_cloud``'s ``traj`` bit for bit.  A batch equals its two halves run separately."""
    from mpinets_amd import robot
    from mpinets_amd.field import CloudField

    pts, cnt = detour["pts"], detour["cnt"]
    free = robot.franka_shortcut_cloud(pts, cnt, None, return_trace=True)
    for name, g, w in zip(NAMES, free, robot.franka_shortcut(pts, cnt, return_trace=True)):
        assert same(g, w), name
    tr, st, po, co, _, _, _ = host(free)
    one = (st == 0) & (co == 2)
    assert one.sum() > 0 and np.array_equal(tr[one], fp.line(detour["qs"], detour["qg"], T)[one])
    kept = robot.franka_shortcut_cloud(pts, cnt, detour["c"], passes=0, **detour["kw"])
    assert same(kept[0], detour["road"][0])
    h = CLOUD_ROWS // 2
    f = detour["field"]
    lo = robot.franka_shortcut_cloud(pts[:h], cnt[:h], detour["c"][:h], field=CloudField(f.values[:h].contiguous(), f.grid),
                                     point_radius=POINT_RADIUS, return_trace=True)
    hi = robot.franka_shortcut_cloud(pts[h:], cnt[h:], detour["c"][h:], field=CloudField(f.values[h:].contiguous(), f.grid),
                                     point_radius=POINT_RADIUS, return_trace=True)
    for name, whole, x, y in zip(NAMES, detour["out"], lo, hi):
        assert same(whole, torch.cat([x, y])), name


def test_global_cloud_planner_with_the_shortcut(detour):
    """``franka_plan_global_cloud(shortcut=True)`` on the 24 rows: candidates 0 .. 7 and the roadmap's seed (now candidate 9)
    are bit-equal to the call without the flag; a row solved by a candidate below 8 comes back identical; the solved set is a
    superset; a row whose choice is 9 returns what the call without the flag returns with choice 8."""
    from mpinets_amd import robot

    kw = dict(detour["kw"], seed=DETOUR_PLAN_SEED, limits=detour["lim"], return_all=True)
    a, b, c = detour["a"], detour["b"], detour["c"]
    old = robot.franka_plan_global_cloud(a, b, c, **kw)
    new = robot.franka_plan_global_cloud(a, b, c, shortcut=True, **kw)
    K = old[3].shape[1] - 1
    assert new[3].shape[1] == K + 2 and torch.equal(new[5], old[5])
    assert same(new[3][:, :K], old[3][:, :K]) and torch.equal(new[4][:, :K], old[4][:, :K])
    assert same(new[3][:, K + 1], old[3][:, K]) and torch.equal(new[4][:, K + 1], old[4][:, K])
    low = (old[1] == 0) & (old[2] < K)
    assert same(new[0][low], old[0][low]) and torch.equal(new[2][low], old[2][low]) and bool((new[1][low] == 0).all())
    assert bool((new[1][old[1] == 0] == 0).all()) and torch.equal(new[1] == 2, old[1] == 2)
    by_old_seed = (new[1] == 0) & (new[2] == K + 1)
    assert bool((old[2][by_old_seed] == K).all()) and same(new[0][by_old_seed], old[0][by_old_seed])
    print(f"franka_plan_global_cloud on {CLOUD_ROWS} rows: solved {int((old[1] == 0).sum())}, with shortcut {int((new[1] == 0).sum())}; "
          f"choice histogram {torch.bincount(new[2][new[1] == 0], minlength=K + 2).tolist()}")
    # the shortcut's seed is franka_shortcut_cloud's trajectory on the roadmap's nodes[path]: the planner keeps its end points
    found = detour["cnt"] >= 2
    assert bool(torch.isnan(new[3][~found & (new[1] != 2), K]).all())


def test_plan_to_poses_and_the_expert_with_the_shortcut():
    """``plan_to_poses(global_plan=True, shortcut=True)`` and ``make_problem_batch(expert_from="cloud_roadmap",
    expert_shortcut=True)`` on 8 rows: they run, the keys are those without the flag, the flag off is the call without it,
    and every row valid without the flag is valid with it."""
    from mpinets_amd import capture, scenes

    torch.cuda.set_device(0)
    B, pr = 8, scenes.EXPERT_CLOUD_POINT_RADIUS
    kw = dict(seed=4, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16, collision_free=True)
    prob = scenes.make_problem_batch(B, device=dev(), device_clouds=True, **kw)
    cloud = prob["xyz"][:, 2048:6144, :3]
    args = (cloud, prob["q"], prob["target_pose"])
    base = capture.plan_to_poses(*args, point_radius=pr, seed=4, global_plan=True)
    off = capture.plan_to_poses(*args, point_radius=pr, seed=4, global_plan=True, shortcut=False)
    on = capture.plan_to_poses(*args, point_radius=pr, seed=4, global_plan=True, shortcut=True)
    assert sorted(base) == sorted(off) == sorted(on)
    assert all(same(base[k], off[k]) for k in base)
    assert all(same(base[k], on[k]) for k in ("q_goal", "ik_status", "roadmap_status"))
    assert bool(on["valid"][base["valid"]].all())
    plain = scenes.make_problem_batch(B, expert=True, expert_from="cloud_roadmap", **kw)
    short = scenes.make_problem_batch(B, expert=True, expert_from="cloud_roadmap", expert_shortcut=True, **kw)
    assert set(plain) == set(short)
    assert all(same(plain[k], short[k]) for k in plain if torch.is_tensor(plain[k]) and k not in ("global_solutions", "expert_valid"))
    assert bool(short["expert_valid"][plain["expert_valid"]].all())
    assert bool(torch.isnan(short["global_solutions"][~short["expert_valid"]]).all())
