"""CPU: ``mpx_gripper_shortcut`` and ``mpx_gripper_shortcut_cloud`` refuse bad arguments on the host, before any launch; their
kernels use no scratch and the LDS their header comment states; the Python defaults are the header's; the wrappers and their
callers (``gripper_plan[_cloud]``, ``scenes.make_problem_batch(hybrid_shortcut=...)``, ``capture.plan_to_poses(
follow_shortcut=...)``) hand to C what they should; and the restatement (tests/float64_gripper_shortcut.py) keeps its
invariants on planar toys and on the gripper roadmap tests' four scenarios (wall and cylinder, as primitives and as a cloud's
field).  The bars of tests/test_gpu_gripper_shortcut.py and tests/test_gpu_gripper_shortcut_cloud.py are derived here: the
float32-geometry run of the restatement against its float64-geometry run, and the share of rows left out because a pose that
decides a chord lies within the band of its threshold.

Recorded at ROADMAP_SEED = 5 on the 64 problems of ``float64_gripper_roadmap.problems()``, the restatement's own float32
roadmaps, the default options (64 points, 2 passes, fan-out 4, resolution 0.01 m), float32 geometry judged in float64:
  wall, primitives       metric length 1.004 -> 0.841, 0 of 64 rows in the band, 39 chords / 1290 interior poses per row (48 / 1618 at most)
  cylinder, primitives   metric length 0.835 -> 0.719, 0 of 64 rows in the band, 31 chords / 1040 interior poses per row (56 / 1507 at most)
  wall, cloud field      metric length 1.035 -> 0.880, 0 of 64 rows in the band, 42 chords / 1382 interior poses per row (66 / 2036 at most)
  cylinder, cloud field  metric length 0.867 -> 0.738, 0 of 64 rows in the band, 36 chords / 1141 interior poses per row (49 / 1557 at most)
63 or 64 of the 64 rows get shorter by more than 1 % in every scenario."""
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
import float64_gripper_roadmap as fg  # noqa: E402
import float64_gripper_roadmap_cloud as fgc  # noqa: E402
import float64_gripper_shortcut as fgs  # noqa: E402
import float64_shortcut as fs  # noqa: E402
import solver_call_grid as grid_calls  # noqa: E402
from test_gripper_roadmap_cloud_host import CLOUD_BAND  # noqa: E402
from test_gripper_roadmap_host import GRIPPER_BAND, LEFT_OUT_CAP  # noqa: E402  (the cap: a condition, not a measurement)

from mpinets_amd import _lib, capture, robot, scenes, solvers  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 64
SHORTER_SHARE = 0.90  # share of the rows that must get shorter by more than 1 %

# recorded by test_float32_run_against_float64_run: the largest |difference| of points_out (positions [m] and quaternion
# entries, up to the sign of q) and of poses (rows 0-2: rotation entries and positions [m]) between the restatement's float32
# and float64 geometry over the primitive scenarios' rows on which both take the same decisions.  Positions are below 0.7 m and
# quaternion entries below 1 (an ulp is 6e-8): a kept vertex is a dense point -- one division, three fmas, an nlerp with a
# square root and four divisions -- of a polyline whose vertices are dense points of the pass before; a pose adds the metric
# lengths, a division, one more nlerp and the products of the rotation matrix.
POINTS_REFERENCE = 8.4e-8  # (128 rows, none with different decisions)
POSES_REFERENCE = 4.5e-7


# ---- refusals ------------------------------------------------------------------------------------------------------------------
GOOD = dict(points=64, passes=2, fanout=4, resolution=0.01, rot_weight=0.12, check_margin=1e-4, clearance=0.0, check_self=1)


def _p(v):  # any non-NULL "device pointer": refused before it is touched
    return ctypes.c_void_p(v) if v else None


def _grid(trunc=0.2, n=(8, 8, 8), h=0.05):
    return _lib.FieldGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), h, n[0], n[1], n[2], trunc)


def _shortcut(lib, B=4, Pin=64, W=8, S=0, M1=0, M2=0, opts=None, pts=256, count=256, goal=256, poses=256, status=256,
              points_out=256, count_out=256, length=256, table=256):
    sph, cub, cyl = _p(table if S else 0), _p(256 if M1 else 0), _p(256 if M2 else 0)
    return lib.mpx_gripper_shortcut(_p(pts), _p(count), B, Pin, W, _p(goal), 0.025, sph, sph, sph, S, cub, cub, M1, cyl, cyl, cyl,
                                    M2, None if opts is None else ctypes.byref(opts), _p(poses), _p(status), _p(points_out),
                                    _p(count_out), _p(length), None, None, None)


def _shortcut_cloud(lib, B=4, Pin=64, W=8, S=56, field=256, grid="good", point_radius=0.02, field_slack=0.0, opts=None, pts=256,
                    count=256, goal=256, poses=256, status=256, points_out=256, count_out=256, length=256, table=256):
    g = _grid() if grid == "good" else grid
    return lib.mpx_gripper_shortcut_cloud(_p(pts), _p(count), B, Pin, W, _p(goal), 0.025, _p(table), _p(table), _p(table), S,
                                          _p(field), None if g is None else ctypes.byref(g), point_radius, field_slack,
                                          None if opts is None else ctypes.byref(opts), _p(poses), _p(status), _p(points_out),
                                          _p(count_out), _p(length), None, None, None)


def test_gripper_shortcut_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    err = lib.mpx_last_error
    opt = lambda **kw: _lib.GripperShortcutOptions(**dict(GOOD, **kw))  # noqa: E731
    for call, name in ((_shortcut, b"mpx_gripper_shortcut"), (_shortcut_cloud, b"mpx_gripper_shortcut_cloud")):
        # what mpx_franka_shortcut refuses
        for Pin in (-1, 0, 1, 257):
            assert call(lib, Pin=Pin, opts=opt(points=256)) != 0 and b"Pin" in err()
        for P in (63, 257, 0, -1):
            assert call(lib, opts=opt(points=P)) != 0 and b"points" in err()
        assert call(lib, opts=opt(passes=-1)) != 0 and b"passes" in err()
        for K in (0, -1, 257):
            assert call(lib, opts=opt(fanout=K)) != 0 and b"fanout" in err()
        for res in (0.0, -0.01, float("nan")):
            assert call(lib, opts=opt(resolution=res)) != 0 and b"resolution" in err()
        assert call(lib, opts=opt(check_margin=-1e-4)) != 0 and b"check_margin" in err()
        assert call(lib, opts=opt(clearance=float("nan"))) != 0 and b"clearance" in err()
        for operand in ("pts", "count"):
            assert call(lib, **{operand: 0}) != 0 and b"NULL operand" in err()
        for out in ("poses", "status", "points_out", "count_out", "length"):
            assert call(lib, **{out: 0}) != 0 and b"NULL output" in err()
        # what mpx_gripper_roadmap refuses
        for W in (-1, 0, 65):
            assert call(lib, W=W) != 0 and b"guide poses" in err()
        for rw in (0.0, -0.12, float("nan"), float("inf")):
            assert call(lib, opts=opt(rot_weight=rw)) != 0 and b"rot_weight" in err()
        assert call(lib, B=-1) != 0 and b"negative size" in err()
        assert call(lib, S=-1) != 0 and b"negative size" in err()
        assert call(lib, S=65) != 0 and b"65" in err()
        assert call(lib, S=56, table=0) != 0 and b"sphere table" in err()
        # its own: the two products indexed in int32
        assert call(lib, B=1 << 25, W=64) != 0 and b"B x W x 16" in err()
        assert call(lib, B=1 << 21, opts=opt(points=256)) != 0 and b"B x P x 7" in err()  # 2^21 x 1792 entries
        assert name in err()
        # a NULL goal_pose and NULL options are operands like the others
        assert call(lib, B=0, goal=0) == 0 and call(lib, B=0, opts=None) == 0
        # nothing to do, nothing touched; a bad option is refused even then
        assert call(lib, B=0, pts=0, count=0, poses=0, status=0, points_out=0, count_out=0, length=0) == 0
        assert call(lib, B=0, opts=opt(fanout=0)) != 0 and call(lib, B=0, opts=opt(rot_weight=0.0)) != 0
    assert _shortcut(lib, M1=65, S=56) != 0 and b"64 cuboids" in err()
    assert _shortcut(lib, M2=65, S=56) != 0 and b"64 cuboids" in err()
    assert _shortcut(lib, M1=-1) != 0 and b"negative size" in err()
    assert _shortcut(lib, M1=4, S=0) != 0 and b"without collision spheres" in err()
    # the cloud form: what mpx_gripper_roadmap_cloud refuses about the field, in its words
    assert _shortcut_cloud(lib, grid=None) != 0 and b"NULL grid" in err()
    assert _shortcut_cloud(lib, grid=_grid(n=(1, 8, 8))) != 0 and b"nodes" in err()
    assert _shortcut_cloud(lib, grid=_grid(h=0.0)) != 0 and b"spacing" in err()
    assert _shortcut_cloud(lib, grid=_grid(trunc=float("inf"))) != 0 and b"trunc" in err()
    for bad in (-0.01, float("nan"), float("inf")):
        assert _shortcut_cloud(lib, field_slack=bad) != 0 and b"field_slack" in err()
        assert _shortcut_cloud(lib, point_radius=bad) != 0 and b"point_radius" in err()
    assert _shortcut_cloud(lib, S=0, table=0) != 0 and b"without collision spheres" in err()
    assert _shortcut_cloud(lib, grid=_grid(trunc=0.1)) != 0 and b"trunc" in err()  # 0.08 + 0.02 + 1e-4 > 0.1
    assert _shortcut_cloud(lib, B=0, grid=_grid(trunc=0.1002)) == 0
    assert _shortcut_cloud(lib, B=0, grid=_grid(trunc=0.15), opts=opt(clearance=0.05)) != 0 and b"trunc" in err()
    assert _shortcut_cloud(lib, B=0, field=0, grid=None, S=0, table=0) == 0  # without a field no grid is read and S may be 0
    assert _shortcut_cloud(lib, B=0, field_slack=-1.0) != 0


def test_python_entry_points_and_defaults_are_one_set():
    p, n = torch.zeros(2, 3, 7), torch.full((2,), 3, dtype=torch.int32)
    for fn, args in ((robot.gripper_shortcut, (p, n)), (robot.gripper_shortcut_cloud, (p, n, None))):
        with pytest.raises(_lib.MpxError):
            fn(*args)  # (CPU tensors)
        sig = inspect.signature(fn).parameters
        assert sig["W"].default == 8 and sig["goal_pose"].default is None and sig["return_trace"].default is False
        assert sig["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert robot.gripper_shortcut is solvers.gripper_shortcut and robot.gripper_plan_cloud is solvers.gripper_plan_cloud
    sig = inspect.signature(robot.gripper_shortcut_cloud).parameters
    assert list(sig)[:9] == ["polylines", "count", "cloud", "counts", "field", "point_radius", "field_slack", "W", "goal_pose"]
    with grid_calls.recording():
        with pytest.raises(TypeError):
            robot.gripper_shortcut(p, n, point=3)
    with pytest.raises(TypeError):
        robot._gripper_shortcut_options("gripper_shortcut", {"smooth_passes": 3})  # (the joint-space shortcut's, not this one's)
    assert robot.GRIPPER_SHORTCUT_DEFAULTS == fgs.DEFAULTS
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    for key in ("points", "passes", "fanout"):
        m = re.search(r"#define MPX_SHORTCUT_DEFAULT_%s\s+(\d+)" % key.upper(), text)
        assert m and int(m.group(1)) == fgs.DEFAULTS[key], key
    for key in ("resolution", "rot_weight"):
        m = re.search(r"#define MPX_GRIPPER_ROADMAP_DEFAULT_%s\s+([0-9.]+)f" % key.upper(), text)
        assert m and float(m.group(1)) == fgs.DEFAULTS[key], key
    for key in ("resolution", "rot_weight", "check_margin", "clearance", "check_self"):  # the gripper roadmap's
        assert fgs.DEFAULTS[key] == fg.DEFAULTS[key], key
    assert (fgs.MAX_POINTS, fgs.MAX_FANOUT) == (fs.MAX_POINTS, fs.MAX_FANOUT)
    assert int(re.search(r"#define MPX_FOLLOW_MAX_POSES\s+(\d+)", text).group(1)) == fgs.MAX_POSES
    assert [n for n, _ in _lib.GripperShortcutOptions._fields_] == list(fgs.DEFAULTS)
    assert _lib.load().mpx_version() == 341
    # composition and the callers' flags: the roadmaps keep their signatures, the flags are off by default
    for fn in (robot.gripper_plan, robot.gripper_plan_cloud):
        sig = inspect.signature(fn).parameters
        assert sig["shortcut"].default is True and sig["roadmap"].default is None and sig["W"].default == 8
    for fn in (robot.gripper_roadmap, robot.gripper_roadmap_cloud):
        assert "shortcut" not in inspect.signature(fn).parameters
    assert inspect.signature(scenes.make_problem_batch).parameters["hybrid_shortcut"].default is False
    sig = inspect.signature(capture.plan_to_poses).parameters["follow_shortcut"]
    assert sig.default is False and sig.kind is inspect.Parameter.KEYWORD_ONLY
    for helper in (scenes._hybrid_trajectories, scenes._hybrid_trajectories_cloud):
        assert list(inspect.signature(helper).parameters)[-1] == "shortcut"


def test_new_value_errors():
    kw = dict(device="cpu", collision_free=True, expert=True)
    for bad in (dict(), dict(hybrid=True), dict(hybrid=True, hybrid_guide="global")):
        with pytest.raises(ValueError, match="hybrid_shortcut needs"):
            scenes.make_problem_batch(1, hybrid_shortcut=True, **kw, **bad)
    with pytest.raises(ValueError, match="hybrid_shortcut needs"):
        scenes.make_problem_batch(1, hybrid_shortcut=dict(passes=1), **kw)
    q0, poses, cloud = torch.zeros(2, 7), torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="follow_shortcut.*needs follow_guide='gripper'"):
        capture.plan_to_poses(cloud, q0, poses, follow_shortcut=True)
    with pytest.raises(ValueError, match="follow_shortcut.*needs follow_guide='gripper'"):
        capture.plan_to_poses(cloud, q0, poses, follow=True, follow_shortcut=dict(passes=1))


def test_what_the_wrappers_hand_to_c():
    B = 3
    pts, cnt = torch.zeros(B, 5, 7), torch.full((B,), 5, dtype=torch.int32)
    goal = torch.eye(4).repeat(B, 1, 1)
    cloud = torch.zeros(B, 9, 4)[:, 2:7, :3]
    with grid_calls.recording() as calls:
        out = robot.gripper_shortcut(pts, cnt, W=6, goal_pose=goal, points=32, rot_weight=0.2)
    assert [c[0] for c in calls] == ["mpx_gripper_shortcut"] and len(out) == 5
    a = calls[0][1]
    assert a[0] == pts.data_ptr() and a[1] == cnt.data_ptr() and a[2:5] == (B, 5, 6) and a[5] == goal.data_ptr()
    assert a[18]._obj.points == 32 and a[18]._obj.rot_weight == pytest.approx(0.2) and a[18]._obj.resolution == pytest.approx(0.01)
    assert None not in a[19:24] and a[24:26] == (None, None)
    assert out[0].shape == (B, 6, 4, 4) and out[2].shape == (B, 32, 7) and out[4].shape == (B, 2)
    with grid_calls.recording() as calls:
        out = robot.gripper_shortcut(pts, cnt, return_trace=True)
    a = calls[0][1]
    assert a[5] is None and len(out) == 7 and None not in a[19:26] and a[18]._obj.points == 64
    # the cloud form: no cloud and no field: NULL field and grid; a cloud: one build; a given field: none
    with grid_calls.recording() as calls:
        robot.gripper_shortcut_cloud(pts, cnt, None)
    assert [c[0] for c in calls] == ["mpx_gripper_shortcut_cloud"] and calls[0][1][11:15] == (None, None, 0.0, 0.0)
    with grid_calls.recording() as calls:
        out = robot.gripper_shortcut_cloud(pts, cnt, cloud, point_radius=0.01, field_slack=0.02, W=4, goal_pose=goal, clearance=0.03)
    assert [c[0] for c in calls] == ["mpx_cloud_field_build", "mpx_gripper_shortcut_cloud"] and len(out) == 5
    built, a = calls[0][1], calls[1][1]
    assert built[6]._obj.trunc == pytest.approx(robot.plan_cloud_truncation(0.01, 0.03, robot.FOLLOW_DEFAULTS["epsilon"]), rel=1e-6)
    assert a[11] == built[7] and a[12]._obj is built[6]._obj and a[13] == 0.01 and a[14] == 0.02 and a[2:5] == (B, 5, 4)
    assert a[15]._obj.clearance == pytest.approx(0.03) and a[10] == 56
    # composition: the roadmap with its graph, then the shortcut over nodes[path] with the roadmap's goal and options
    M = torch.eye(4).repeat(B, 1, 1)
    with grid_calls.recording() as calls:
        out = robot.gripper_plan(M, M, W=5, seed=7, env_offset=2, roadmap=dict(nodes=80, resolution=0.02, clearance=0.01),
                                 shortcut=dict(passes=1), return_length=True)
    assert [c[0] for c in calls] == ["mpx_gripper_roadmap", "mpx_gripper_shortcut"] and len(out) == 3
    rm, sc = calls[0][1], calls[1][1]
    assert None not in rm[20:27] and rm[17]._obj.nodes == 80 and rm[18] == 7 and rm[19] == 2
    assert sc[2:5] == (B, 80, 5) and sc[5] == rm[1] and sc[18]._obj.points == 80 and sc[18]._obj.passes == 1
    assert sc[18]._obj.resolution == pytest.approx(0.02) and sc[18]._obj.clearance == pytest.approx(0.01)
    with grid_calls.recording() as calls:
        out = robot.gripper_plan(M, M, W=5, shortcut=None)
    assert [c[0] for c in calls] == ["mpx_gripper_roadmap"] and len(out) == 2 and calls[0][1][24:27] == (None, None, None)
    with grid_calls.recording() as calls:
        robot.gripper_plan_cloud(M, M, cloud, point_radius=0.01, field_slack=0.02)
    assert [c[0] for c in calls] == ["mpx_cloud_field_build", "mpx_gripper_roadmap_cloud", "mpx_gripper_shortcut_cloud"]
    built, rm, sc = (c[1] for c in calls)
    assert rm[10] == built[7] == sc[11] and rm[12:14] == sc[13:15] == (0.01, 0.02) and sc[15]._obj.points == 64


def test_callers_are_unchanged_without_the_flag_and_share_one_field_with_it():
    B = 2
    q0, q1, valid = torch.zeros(B, 7), torch.full((B, 7), 0.1), torch.ones(B, dtype=torch.bool)
    big, plan = torch.zeros(B, 5, 3), torch.zeros(B, scenes.EXPERT_LENGTH, 7)
    prims = {k: torch.zeros((B, 1) + s) for k, s in (("cuboid_centers", (3,)), ("cuboid_dims", (3,)), ("cuboid_quats", (4,)),
                                                       ("cylinder_centers", (3,)), ("cylinder_radii", (1,)),
                                                       ("cylinder_heights", (1,)), ("cylinder_quats", (4,)))}

    def names(calls):
        return [c[0] for c in calls if "fk" not in c[0] and "prim_frames" not in c[0]]

    # the primitive helper
    with grid_calls.recording() as calls:
        off = scenes._hybrid_trajectories(prims, q0, plan, valid, q1, 5, 2, True)
    with grid_calls.recording() as same:
        scenes._hybrid_trajectories(prims, q0, plan, valid, q1, 5, 2, True, shortcut=False)
    assert names(calls) == names(same) and names(calls)[-2:] == ["mpx_gripper_roadmap", "mpx_franka_follow"]
    with grid_calls.recording() as calls:
        on = scenes._hybrid_trajectories(prims, q0, plan, valid, q1, 5, 2, True, shortcut=dict(clearance=0.02))
    assert names(calls)[-3:] == ["mpx_gripper_roadmap", "mpx_gripper_shortcut", "mpx_franka_follow"] and sorted(on) == sorted(off)
    by = {c[0]: c[1] for c in calls}
    assert by["mpx_gripper_shortcut"][18]._obj.clearance == pytest.approx(0.02) and by["mpx_gripper_shortcut"][4] == scenes.HYBRID_GUIDE_POSES
    assert by["mpx_franka_follow"][1] == on["hybrid_guide_poses"].data_ptr()  # the follower is handed the shortcut's poses
    # the cloud helper: one field build, and the roadmap, the shortcut and the follower read it
    with grid_calls.recording() as calls:
        off = scenes._hybrid_trajectories_cloud(big, q0, plan, valid, 0.02, q1, 5, 2, gripper_guide=True)
    assert names(calls) == ["mpx_cloud_field_build", "mpx_gripper_roadmap_cloud", "mpx_franka_follow_cloud"]
    with grid_calls.recording() as calls:
        on = scenes._hybrid_trajectories_cloud(big, q0, plan, valid, 0.02, q1, 5, 2, gripper_guide=True, shortcut=True)
    assert names(calls) == ["mpx_cloud_field_build", "mpx_gripper_roadmap_cloud", "mpx_gripper_shortcut_cloud", "mpx_franka_follow_cloud"]
    by = {c[0]: c[1] for c in calls}
    build, rm, sc, fol = (by[n] for n in names(calls))
    assert rm[10] == build[7] == sc[11] == fol[11] and sc[13] == pytest.approx(0.02) and sorted(on) == sorted(off)
    assert fol[1] == on["hybrid_guide_poses"].data_ptr()
    # plan_to_poses
    B = 3
    q0, poses = torch.zeros(B, 7), torch.eye(4).repeat(B, 1, 1)
    cloud, counts = torch.zeros(B, 9, 4)[:, 2:7, :3], torch.full((B,), 4, dtype=torch.int32)
    kw = dict(counts=counts, T=grid_calls.T, seed=5, env_offset=2, follow=True, follow_poses=6, follow_guide="gripper",
              gripper_options=dict(nodes=16, field_slack=0.02))
    with grid_calls.recording() as calls:
        off = capture.plan_to_poses(cloud, q0, poses, **kw)
    assert names(calls) == ["mpx_cloud_field_build", "mpx_franka_ik_cloud", "mpx_franka_plan_cloud", "mpx_gripper_roadmap_cloud",
                            "mpx_franka_follow_cloud"]
    with grid_calls.recording() as calls:
        on = capture.plan_to_poses(cloud, q0, poses, follow_shortcut=True, **kw)
    assert names(calls) == ["mpx_cloud_field_build", "mpx_franka_ik_cloud", "mpx_franka_plan_cloud", "mpx_gripper_roadmap_cloud",
                            "mpx_gripper_shortcut_cloud", "mpx_franka_follow_cloud"]
    by = {c[0]: c[1] for c in calls}
    rm, sc = by["mpx_gripper_roadmap_cloud"], by["mpx_gripper_shortcut_cloud"]
    assert rm[10] == by["mpx_cloud_field_build"][7] == sc[11] == by["mpx_franka_follow_cloud"][11]  # ONE field
    assert rm[13] == sc[14] == pytest.approx(0.02) and rm[14]._obj.nodes == 16 and sc[4] == 6 and sc[15]._obj.points == 64
    assert sorted(on) == sorted(off) and on["follow_guide_poses"].shape == (B, 6, 4, 4)


def test_gripper_shortcut_kernel_metadata():
    """Exactly one kernel of each name; no scratch, no VGPR spills; LDS is dynamic, and the bytes the header comment states
    (32 796 B at 256 points, 24 604 B for the cloud form) are what the sources' layout gives."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    md = kernel_metadata(LIB)
    for name in ("gripper_shortcut_kernel", "gripper_shortcut_cloud_kernel"):
        hits = {n: f for n, f in md.items() if name + "PK" in n}
        assert len(hits) == 1, name
        (f,) = hits.values()
        print(name, {k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0

    def lds(P, rows):  # the layout of the sources, in bytes: rows | spheres | count | poly, dist, 5 int arrays, off, first, ctl
        return 4 * (rows + 64 * 4 + 1 + 2 * P * 7 + 2 * P + 5 * P + 2 * (P + 1) + 4)
    assert lds(256, 128 * 16) == 32796 and lds(256, 0) == 24604 and lds(256, 128 * 16) - lds(256, 0) == 8192
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    assert "32 796 B at 256" in text and "24 604 B for the cloud form" in text
    for src, stated in (("gripper_shortcut.hip", "32 796 B"), ("gripper_shortcut_cloud.hip", "24 604 B")):
        assert stated in open(os.path.join(ROOT, "motion-policy-networks_amd", "csrc", src)).read()


# ---- the restatement on planar toys ----------------------------------------------------------------------------------------------
def _quat_z(angle):
    return np.float32([0.0, 0.0, np.sin(angle / 2), np.cos(angle / 2)])


def _disc(centre=(0.0, 0.0), radius=0.45):
    c = np.float64(centre)
    return lambda q: np.linalg.norm(np.asarray(q, np.float64)[:, :2] - c, axis=-1) > radius


def _dogleg(turn=1.2):
    """Three vertices round the disc, the gripper turning by ``turn`` rad about z along the way."""
    p = np.zeros((3, 7), np.float32)
    p[:, :2] = [(-0.9, 0.0), (0.0, 1.5), (0.9, 0.0)]
    for i, a in enumerate((0.0, turn / 2, turn)):
        p[i, 3:] = _quat_z(a)
    return p


def test_row_rule_probes_and_densification():
    p = _dogleg()
    assert not fgs.bad_row(p, 3) and not fgs.bad_row(p, 2) and fgs.bad_row(p, 1) and fgs.bad_row(p, 4)
    for bad in (np.nan, np.inf):
        q = p.copy()
        q[1, 5] = bad
        assert fgs.bad_row(q, 3) and fgs.bad_row(q, 2)
    q = p.copy()
    q[2, 3:] *= np.float32(1.1)
    assert fgs.bad_row(q, 3) and not fgs.bad_row(q, 2)  # (a vertex behind count is not read)
    q[2, 3:] = p[2, 3:] * np.float32(1 + 2.0 ** -12)  # |q|^2 within 2^-10 of 1
    assert not fgs.bad_row(q, 3)
    for dt in (np.float64, np.float32):
        D, at = fgs.densify(p, 64, dtype=dt)
        assert 62 <= len(D) <= 64 and at[0] == 0 and at[-1] == len(D) - 1
        assert np.array_equal(D[at], p.astype(dt))  # the vertices are copied
        assert np.abs(np.linalg.norm(D[:, 3:].astype(np.float64), axis=-1) - 1).max() < 1e-6  # nlerp keeps unit length
        assert len(fgs.densify(np.repeat(p[:1], 4, 0), 64, dtype=dt)[0]) == 4  # L = 0: nothing is added
        assert len(fgs.densify(p, 3, dtype=dt)[0]) == 3  # P = n: nothing is added
    # a pure rotation has length 2 rot_weight |q_b - q_a| = 4 rot_weight sin(theta / 4)
    a, b = np.zeros(7), np.zeros(7)
    a[3:], b[3:] = _quat_z(0.0), _quat_z(0.8)
    assert fgs.length(a, b) == pytest.approx(4 * 0.12 * np.sin(0.2), rel=1e-6)
    b[3:] = -b[3:]
    assert fgs.length(a, b) == pytest.approx(4 * 0.12 * np.sin(0.2), rel=1e-6)  # the sign of q is free


@pytest.mark.parametrize("K", [1, 2, 4, 256])
def test_planar_dogleg_with_a_rotation_is_cut_and_a_free_line_gives_one_hop(K):
    p = _dogleg()
    before = fgs.polyline_length(p)
    out = fgs.shortcut(p, _disc(), fanout=K)
    assert out["length"][0] == before and out["length"][1] < 0.8 * before and len(out["points_out"]) >= 3
    assert np.array_equal(out["points_out"][0], p[0]) and np.array_equal(out["points_out"][-1], p[-1])
    assert not out["in_band"]
    for a, e in out["free"]:  # every chord found free is free by a finer test
        assert _disc(radius=0.449)(fg.edge_poses(a, e, 2000)).all()
    # rows 0-2 of the last pose: the goal's when one is given, else the last vertex's own frame
    assert np.array_equal(out["poses"][-1], fg.pose_matrix(p[2:].astype(np.float64))[0])
    goal = np.eye(4, dtype=np.float32)
    goal[:3, 3] = (0.9, 0.0, 0.001)
    with_goal = fgs.shortcut(p, _disc(), goal_pose=goal, fanout=K)
    assert np.array_equal(with_goal["poses"][-1, :3], goal[:3].astype(np.float64)) and np.array_equal(with_goal["poses"][:-1], out["poses"][:-1])
    assert np.array_equal(out["poses"][:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (8, 1)))
    free = fgs.shortcut(p, _disc(centre=(0.0, -2.0)), fanout=K)
    first_level = len(fs.probes(1, len(fgs.densify(p, 64)[0]) - 1, K))  # (one level: its last chord reaches the far end)
    assert len(free["points_out"]) == 2 and free["chords"] == first_level
    # the guide poses of one hop turn evenly from the start's rotation to the goal's
    yaw = np.arctan2(free["poses"][:, 1, 0], free["poses"][:, 0, 0])
    assert np.all(np.diff(yaw) > 0) and yaw[-1] == pytest.approx(1.2, abs=1e-6)
    kept = fgs.shortcut(p, _disc(), passes=0, fanout=K)
    assert np.array_equal(kept["points_out"], p.astype(np.float64)) and kept["chords"] == 0
    assert np.array_equal(kept["poses"][:-1], fg.resample(p, [0, 1, 2], 8)[:-1])  # ... and the roadmap's own resampling
    # nothing is free: the input's own pieces remain.  The metric takes the CHORD of a quaternion pair and an nlerp runs along
    # the arc, so the pieces of an edge sum to more than the edge: by at most arc / chord = phi / (2 sin(phi / 2)) <=
    # 1 + phi^2 / 24 on the rotation part, phi = 0.3 rad the quaternion angle of an edge here (half the turn of 0.6 rad).
    walled = fgs.shortcut(p, lambda q: np.zeros(len(q), bool), fanout=K)
    assert before <= walled["length"][1] <= before * (1 + 0.3 ** 2 / 24)
    assert np.array_equal(walled["points_out"][[0, -1]], p[[0, 2]].astype(np.float64))
    flipped = p.copy()
    flipped[1, 3:] = -flipped[1, 3:]  # the sign of an input quaternion is free
    other = fgs.shortcut(flipped, _disc(), fanout=K)
    assert (other["chords"], other["configs"], len(other["points_out"])) == (out["chords"], out["configs"], len(out["points_out"]))
    assert np.abs(other["poses"] - out["poses"]).max() < 1e-12


# ---- the restatement on the gripper roadmap tests' scenarios ---------------------------------------------------------------------
def scenario_rule(kind, form, b, scene=None, field=None, grid=None):
    """-> is_valid, margins, band of problem ``b`` of a scenario at the default options."""
    if form == "primitives":
        valid, m = fgs.prim_rule(None if scene is None else {k: v[b:b + 1] for k, v in scene.items()})
        return valid, m, GRIPPER_BAND
    valid, m = fgs.field_rule(field, grid, fgc.POINT_RADIUS)
    return valid, m, CLOUD_BAND


@pytest.fixture(scope="module")
def scenarios():
    sp, gp = fg.problems(ROWS)
    out = {}
    t0 = time.time()
    for kind in ("wall", "cylinder"):
        for form in ("primitives", "cloud"):
            scene = field = grid = None
            if form == "primitives":
                scene = fg.scene_of(fg.scene_arrays(ROWS, kind), ROWS)
                road = fg.solve(sp, gp, scene, seed=fg.ROADMAP_SEED, dtype=np.float32)
            else:
                _, grid, field = fgc.scenario_field(kind)
                road = fgc.solve(sp, gp, field, grid, fgc.POINT_RADIUS, seed=fgc.ROADMAP_SEED, dtype=np.float32)
            pts, cnt = fgs.path_polylines(road[4], road[2], road[3])
            runs = {}
            for b in np.flatnonzero(cnt >= 2):
                valid, m, band = scenario_rule(kind, form, b, scene, field, grid)
                runs[b] = {np.float32: fgs.shortcut(pts[b, :cnt[b]], valid, goal_pose=gp[b], dtype=np.float32, margins=m, band=band)}
                if form == "primitives":
                    runs[b][np.float64] = fgs.shortcut(pts[b, :cnt[b]], valid, goal_pose=gp[b], dtype=np.float64)
            out[kind, form] = (road, pts, cnt, runs)
    print(f"four scenarios: roadmaps and {sum(len(v[3]) for v in out.values())} shortcuts (128 of them twice) {time.time() - t0:.0f} s")
    return sp, gp, out


def test_left_out_share_and_what_the_shortcut_gains(scenarios):
    """On the four scenarios the restatement alone leaves out at most LEFT_OUT_CAP of the rows (a condition: the GPU tests
    compare decisions on the rest), at least SHORTER_SHARE of the rows get shorter by more than 1 %, no row grows, the end
    vertices are kept bit for bit, the last pose is the goal's.  The module docstring records the figures printed here."""
    sp, gp, out = scenarios
    for (kind, form), (road, pts, cnt, runs) in out.items():
        L = np.float64([r[np.float32]["length"] for r in runs.values()])
        left = sum(r[np.float32]["in_band"] for r in runs.values())
        chords, configs = [r[np.float32]["chords"] for r in runs.values()], [r[np.float32]["configs"] for r in runs.values()]
        shorter = int((L[:, 1] < 0.99 * L[:, 0]).sum())
        print(f"{kind} ({form}): {len(runs)} rows with a path, metric length {L[:, 0].mean():.3f} -> {L[:, 1].mean():.3f}, {left} in the "
              f"band, {shorter} shorter by more than 1 %, chords mean {np.mean(chords):.0f} max {max(chords)}, interior poses mean "
              f"{np.mean(configs):.0f} max {max(configs)}")
        assert len(runs) >= 0.9 * ROWS and left / len(runs) <= LEFT_OUT_CAP
        assert shorter >= SHORTER_SHARE * len(runs) and (L[:, 1] <= L[:, 0] * (1 + 1e-6)).all()
        for b, r in runs.items():
            o = r[np.float32]
            assert np.array_equal(o["points_out"][0], pts[b, 0]) and np.array_equal(o["points_out"][-1], pts[b, cnt[b] - 1])
            assert np.array_equal(o["poses"][-1, :3], gp[b, :3]) and np.array_equal(o["poses"][-1, 3], [0, 0, 0, 1])
            assert len(o["points_out"]) >= 3  # (the obstacle sits between every start and its goal)


def test_no_passes_give_the_input_and_the_roadmaps_poses_back(scenarios):
    sp, gp, out = scenarios
    for (kind, form), (road, pts, cnt, runs) in out.items():
        for b in list(runs)[:8]:
            kept = fgs.shortcut(pts[b, :cnt[b]], lambda q: np.ones(len(q), bool), goal_pose=gp[b], dtype=np.float32, passes=0)
            assert np.array_equal(kept["points_out"], pts[b, :cnt[b]]) and kept["chords"] == 0 and kept["configs"] == 0
            assert kept["length"][0] == kept["length"][1]
            assert np.array_equal(kept["poses"], road[0][b])  # the roadmap's own guide poses, bit for bit
            free = fgs.shortcut(pts[b, :cnt[b]], lambda q: np.ones(len(q), bool), dtype=np.float32)
            assert len(free["points_out"]) == 2 and free["chords"] == fgs.DEFAULTS["fanout"]  # (one level)


def test_float32_run_against_float64_run(scenarios):
    """Reference against reference: the restatement with float32 geometry against the one with float64 geometry, both judged
    in float64, over the two primitive scenarios (the geometry is the cloud form's too).  Where both take the same decisions
    (the same chords, interior poses and vertex count) ``points_out`` (up to the sign of q) and ``poses`` differ by
    POINTS_REFERENCE / POSES_REFERENCE at most; the GPU tests' bars are 4x the recorded figures, the roadmap tests' convention
    (the device's division and square root may differ from numpy's by the last bit), and the measurement must land within a
    factor 2 of them here."""
    sp, gp, out = scenarios
    worst_p, worst_t, same, differ = 0.0, 0.0, 0, 0
    for (kind, form), (road, pts, cnt, runs) in out.items():
        for b, r in runs.items():
            if np.float64 not in r:
                continue
            a32, a64 = r[np.float32], r[np.float64]
            if (a32["chords"], a32["configs"], len(a32["points_out"])) != (a64["chords"], a64["configs"], len(a64["points_out"])):
                differ += 1
                continue
            same += 1
            p32, p64 = a32["points_out"].astype(np.float64), a64["points_out"]
            worst_p = max(worst_p, float(np.abs(p32[:, :3] - p64[:, :3]).max()), float(fgs.same_rotation(p32[:, 3:], p64[:, 3:]).max()))
            worst_t = max(worst_t, float(np.abs(a32["poses"].astype(np.float64) - a64["poses"]).max()))
    print(f"float32 vs float64 restatement over {same} rows (decisions differ on {differ}): points_out max {worst_p:.3e}, "
          f"poses max {worst_t:.3e}")
    assert same >= ROWS and differ <= LEFT_OUT_CAP * (same + differ)
    assert POINTS_REFERENCE / 2 <= worst_p <= POINTS_REFERENCE * 2
    assert POSES_REFERENCE / 2 <= worst_t <= POSES_REFERENCE * 2
