"""CPU: the float64 restatement of the path follower (tests/float64_follow.py) stands on its own -- the fixed point, the
retiming on a polyline with known arc lengths, the chord bound, chunked rollouts -- the bars of the GPU tests
(tests/test_gpu_follow.py) are derived here from the float32 run of the restatement against its float64 run, and
``mpx_franka_follow`` / ``robot.franka_follow`` refuse bad arguments before any launch.  The follower is a stand-in for the
reference's Geometric Fabrics expert, not Lula."""
import ctypes
import functools
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_follow as ff  # noqa: E402
import float64_plan as fp  # noqa: E402
import solver_call_grid as grid  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 50
SAMPLE_EVERY = 16  # the one-step test starts from every 16th state of the float64 rollout


# ---- the inputs the GPU tests share, and the float64 / float32 runs of the restatement on them --------------------------------
@functools.lru_cache(maxsize=None)
def shared_problems():
    """-> q_start, q_goal, guide, scene arrays of ``float64_follow.problems`` (32 problems, seed ``PROBLEM_SEED``)."""
    return ff.problems(32, ff.PROBLEM_SEED)


@functools.lru_cache(maxsize=None)
def reference(kind, dtype=torch.float64):
    """The restatement's ``follow`` on the 32 ``kind`` = "free" / "cuboid" problems in ``dtype`` (computed once, never written)."""
    qs, _, guide, scn = shared_problems()
    scene = fp.scene_from_arrays(scn) if kind == "cuboid" else None
    return ff.follow(qs, guide, scene, T=T, dtype=dtype, record_states=dtype == torch.float64)


@functools.lru_cache(maxsize=None)
def one_step_states():
    """Every SAMPLE_EVERY-th state of the float64 rollout beside the cuboid, rounded to float32: -> row index [N], q, v
    float32 [N,7], progress int32 [N,3] (finished flag 0: the step decides for itself).  (A dense path may graze the cube:
    such states are kept, a continued rollout is not refused for them, and they reach the c'(d) = -1 branch.)"""
    r = reference("cuboid")
    rows, qq, vv, pg = [], [], [], []
    for b in range(len(r["steps"])):
        for i in range(0, int(r["steps"][b]) + 1, SAMPLE_EVERY):
            rows.append(b), qq.append(r["path"][b, i]), vv.append(r["states"]["v"][b, i])
            pg.append([r["states"]["w"][b, i], r["states"]["nw"][b, i], 0])
    return np.asarray(rows), np.asarray(qq, np.float32), np.asarray(vv, np.float32), np.asarray(pg, np.int32)


def one_step(dtype):
    """One step of the restatement from ``one_step_states`` in ``dtype`` -> q', v' (float64 numpy), progress int32 [N,3],
    fragile bool [N], |repel g| [N]."""
    rows, q, v, pg = one_step_states()
    qs, _, guide, scn = shared_problems()
    scene = {k: a[rows] for k, a in fp.scene_from_arrays(scn).items()}
    r = ff.rollout(q, guide[rows], scene, v_init=v, progress=pg, dtype=dtype, max_steps=1)
    assert not r["bad"].any()
    return (r["q_end"].astype(np.float64), r["v_end"].astype(np.float64), r["progress_end"], r["fragile"][:, 0], r["repel_g"])


# What the bars of tests/test_gpu_follow.py are 4x of: the float32 run of the restatement against its float64 run on the
# GPU tests' inputs, measured on the CPU by the two tests below (which repeat the measurement).
ONE_STEP_REFERENCE = {"q": 1.8e-7, "v": 7.2e-6}  # [rad], [rad/s]: q' = q + dt v is one rounding of q; v' carries dt a, a = 144 u
ROLLOUT_REFERENCE = 2.7e-5  # [rad] over the whole dense path
ONE_STEP_LEFT_OUT_CAP = 0.02
FREE_LEFT_OUT_CAP = 0.10
CUBOID_FRAGILE_SHARE = 6 / 32  # the cuboid rows with a fragile step in the float64 run, measured on the CPU
CUBOID_LEFT_OUT_CAP = CUBOID_FRAGILE_SHARE + 0.05  # (<= 0.25: the whole-rollout comparison of the obstacle rows is kept)


def test_one_step_bar_can_be_derived_again():
    """Reference against reference, one step from the sampled float32 states.  Measured: 919 states, max |dq'| 1.75e-7 rad,
    max |dv'| 7.17e-6 rad/s, 0.11 % of the states left out as fragile, progress equal on every kept state, largest
    |repel g| 104.8 rad/s^2.  The GPU test's bars are 4x the recorded figures, one for q' and one for v' (the larger alone
    would ask less of q'); here the measurement is repeated and must land within a factor 2 of them."""
    q64, v64, p64, fragile, repel = one_step(torch.float64)
    q32, v32, p32, _, _ = one_step(torch.float32)
    keep = ~fragile
    dq, dv = np.abs(q64 - q32).max(-1), np.abs(v64 - v32).max(-1)
    print(f"one step from {len(keep)} states, float32 vs float64 restatement: max |dq'| {dq[keep].max():.3e}, max |dv'| "
          f"{dv[keep].max():.3e} (all states: {dq.max():.3e}, {dv.max():.3e}), left out {fragile.mean():.4f}, progress differs on "
          f"{int((p64 != p32).any(-1)[keep].sum())} kept states, largest |repel g| {repel.max():.2f}")
    assert fragile.mean() <= ONE_STEP_LEFT_OUT_CAP
    assert np.array_equal(p64[keep], p32[keep])
    assert repel.max() > 1e-3  # (the obstacle term moves something on these inputs)
    assert ONE_STEP_REFERENCE["q"] / 2 <= dq[keep].max() <= ONE_STEP_REFERENCE["q"] * 2
    assert ONE_STEP_REFERENCE["v"] / 2 <= dv[keep].max() <= ONE_STEP_REFERENCE["v"] * 2


def test_rollout_bar_can_be_derived_again():
    """Reference against reference, whole rollouts (the damping makes the system contractive, so dense paths compare).
    Measured: free space, 142 .. 1024 steps, 2 of 32 rows have a fragile step (both at the stop test), the float32 dense
    path stays within 2.71e-5 rad of the float64 one over the kept rows, 29 valid in either arithmetic (3 miss); beside the
    cube 141 .. 1024 steps, 6 of 32 rows fragile (stop 4, gradient 2, clamp 2, switch 1), 2.00e-5 rad, 28 valid (2 hit the
    cube, 2 miss); the same rollouts judged in the cube's scene WITHOUT the obstacle term: see test_gpu_follow.py.  Step
    counts are equal on every kept row.  The largest retimed third difference is 0.103 rad against the bar of 0.15."""
    worst = {}
    for kind in ("free", "cuboid"):
        r64, r32 = reference(kind), reference(kind, torch.float32)
        fragile = r64["fragile"].any(1)
        same = r64["steps"] == r32["steps"]
        d = np.nanmax(np.abs(r64["path"] - r32["path"].astype(np.float64)).reshape(len(same), -1), 1)
        keep = ~fragile
        assert same[keep].all()  # (a row without a fragile step takes the same number of steps in float32)
        worst[kind] = float(d[keep].max())
        kinds = {k: int(v.sum()) for k, v in r64["fragile_kinds"].items()}
        print(f"{kind}: steps {r64['steps'].min()} .. {r64['steps'].max()}, rows with a fragile step {int(fragile.sum())} of "
              f"{len(fragile)} {kinds}, float32 vs float64 dense path max {worst[kind]:.3e} rad over the kept rows, valid "
              f"{int((r64['status'] == 0).sum())} (float64) / {int((r32['status'] == 0).sum())} (float32), bits "
              f"{np.bincount(r64['bits'], minlength=16).tolist()}, largest retimed third difference "
              f"{np.abs(np.diff(r64['traj_any'], 3, axis=1)).max():.4f}")
    f_free, f_cub = reference("free")["fragile"].any(1).mean(), reference("cuboid")["fragile"].any(1).mean()
    assert f_free <= FREE_LEFT_OUT_CAP
    assert f_cub == pytest.approx(CUBOID_FRAGILE_SHARE, abs=1e-9) and CUBOID_LEFT_OUT_CAP <= 0.25
    assert ROLLOUT_REFERENCE / 2 <= max(worst.values()) <= ROLLOUT_REFERENCE * 2


# ---- the restatement's own properties --------------------------------------------------------------------------------------------
def test_a_guide_that_is_the_start_pose_is_a_fixed_point():
    """Free space, one guide pose = the pose of q_start: the stop test holds on entry, no step is taken, the T waypoints
    are q_start and the verdict is clean."""
    qs, _, _, _ = shared_problems()
    from oracle import oracle as orc

    pose = orc.frames_to_4x4(orc.franka_fk(qs)[:, ff.RIGHT_GRIPPER]).reshape(-1, 1, 4, 4)
    r = ff.follow(qs, pose, None, T=T)
    assert (r["steps"] == 0).all() and (r["progress_end"] == [0, 0, 1]).all()
    assert np.array_equal(r["traj"], np.broadcast_to(qs.astype(np.float64)[:, None], r["traj"].shape))
    assert (r["status"] == 0).all() and np.array_equal(r["q_end"], qs.astype(np.float64))


def test_retiming_is_exact_on_a_polyline_with_known_arc_lengths():
    path = np.zeros((1, 5, 7))
    path[0, 1, 0], path[0, 2, :2], path[0, 3, :3] = 1.0, (1.0, 2.0), (1.0, 2.0, 1.0)  # edges of length 1, 2, 1
    path[0, 4] = 99.0  # (behind n: never read)
    arc = np.asarray([[0.0, 1.0, 3.0, 4.0, 99.0]])
    out = ff.retime(path, arc, np.asarray([3]), 9)  # s_t = t / 2
    want = np.zeros((9, 7))
    want[:, 0] = np.minimum(np.arange(9) / 2, 1.0)
    want[:, 1] = np.clip(np.arange(9) / 2 - 1.0, 0, 2.0)
    want[:, 2] = np.clip(np.arange(9) / 2 - 3.0, 0, 1.0)
    assert np.array_equal(out[0], want)
    # a zero-length edge is stepped over, n = 0 gives T copies of the start
    arc0 = np.asarray([[0.0, 1.0, 1.0, 2.0, 99.0]])
    path0 = path.copy()
    path0[0, 2], path0[0, 3] = path0[0, 1], (2.0, 0, 0, 0, 0, 0, 0)
    assert np.array_equal(ff.retime(path0, arc0, np.asarray([3]), 5)[0, :, 0], [0.0, 0.5, 1.0, 1.5, 2.0])
    assert np.array_equal(ff.retime(path, arc, np.asarray([0]), 4)[0], np.zeros((4, 7)))


def test_chords_of_the_retimed_trajectory_are_bounded_by_the_arc_step():
    """Constant speed: every retimed segment's chord is at most arc[n] / (T-1), and waypoints 0 and T-1 are path[0] and path[n]."""
    for kind in ("free", "cuboid"):
        r = reference(kind)
        n = r["steps"]
        total = r["arc"][np.arange(len(n)), n]
        chord = np.linalg.norm(np.diff(r["traj_any"], axis=1), axis=-1)
        assert (chord <= (total / (T - 1))[:, None] * (1 + 1e-12) + 1e-15).all()
        assert np.array_equal(r["traj_any"][:, 0], r["path"][:, 0])
        assert np.array_equal(r["traj_any"][:, -1], r["path"][np.arange(len(n)), n])
        assert (chord.sum(1) >= 0.9 * total).all()  # (and the polyline is not cut short)


def test_chunked_rollouts_equal_the_single_rollout():
    """Four calls of 256 steps with (q_end, v_end, progress_end) carried over walk the dense path of one call of 1024 steps
    exactly; a finished row takes no further step."""
    qs, _, guide, scn = shared_problems()
    scene = fp.scene_from_arrays(scn)
    # the restatement's interface takes float32 inputs, as the device's does: the float32 run carries its state exactly
    single = ff.rollout(qs, guide, scene, dtype=torch.float32)
    q, v, pg, at = qs, None, None, np.zeros(len(qs), np.int64)
    path = np.full_like(single["path"], np.nan)
    path[:, 0] = qs
    for _ in range(4):
        r = ff.rollout(q, guide, scene, v_init=v, progress=pg, dtype=torch.float32, max_steps=256)
        for b in range(len(qs)):
            n = int(r["steps"][b])
            path[b, at[b] + 1:at[b] + 1 + n] = r["path"][b, 1:n + 1]
            at[b] += n
        q, v, pg = r["q_end"], r["v_end"], r["progress_end"]
    assert np.array_equal(at, single["steps"])
    assert np.array_equal(path, single["path"], equal_nan=True)
    assert np.array_equal(pg, single["progress_end"])
    done = pg[:, 2] == 1
    assert done.any()
    again = ff.rollout(q, guide, scene, v_init=v, progress=pg, dtype=torch.float32, max_steps=8)
    assert (again["steps"][done] == 0).all() and np.array_equal(again["q_end"][done], q[done])


def test_bad_rows_take_no_steps():
    qs, _, guide, scn = shared_problems()
    qs, guide = qs[:4].copy(), guide[:4].copy()
    scene = {k: v[:4] for k, v in fp.scene_from_arrays(scn).items()}
    guide[0, 3, 1, 2] = np.nan
    qs[1, 3] = 3.0  # outside the limits
    c = scene["cub_frames"][2]  # put the start's hand inside the cube: move the cube onto right_gripper(q_start)
    from oracle import oracle as orc

    hand = orc.franka_fk(qs[2:3])[0, ff.RIGHT_GRIPPER, 9:]
    c[0, :3, 3] = -(c[0, :3, :3] @ hand)
    r = ff.follow(qs, guide, scene, T=T)
    assert r["status"].tolist() == [2, 2, 2, r["status"][3]] and r["status"][3] != 2
    assert (r["bits"][:3] == 15).all() and (r["steps"][:3] == 0).all() and np.isnan(r["traj_any"][:3]).all()


# ---- the C entry and the Python wrapper, without a GPU ------------------------------------------------------------------------------
def _call(lib, B=4, W=8, T=50, S=0, M1=0, opts=None, out=256, path=256):
    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched
    sph, cub = (one if S else None), (one if M1 else None)
    o = ctypes.c_void_p(out) if out else None
    return lib.mpx_franka_follow(one, one, B, W, T, 0.025, one, sph, sph, sph, S, cub, cub, M1, None, None, None, 0, None, None,
                                 None if opts is None else ctypes.byref(opts), ctypes.c_void_p(path) if path else None, o, o, o, o,
                                 o, None, None, None, None, None)


def _options(**given):
    from mpinets_amd import _lib, robot

    return robot._follow_options("test", dict(given))[0] if given else _lib.FollowOptions(*[
        robot.FOLLOW_DEFAULTS[n] for n, _ in _lib.FollowOptions._fields_])


def test_bad_arguments_are_refused_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert lib.mpx_version() == 341
    assert _call(lib, out=0) != 0 and b"NULL output" in lib.mpx_last_error()
    assert _call(lib, path=0) != 0 and b"NULL output" in lib.mpx_last_error()
    for T_ in (1, 65):
        assert _call(lib, T=T_) != 0 and b"waypoints" in lib.mpx_last_error()
    for W in (0, 65):
        assert _call(lib, W=W) != 0 and b"guide poses" in lib.mpx_last_error()
    for n in (0, 4097, -1):
        assert _call(lib, opts=_options(max_steps=n)) != 0 and b"max_steps" in lib.mpx_last_error()
    # (the largest accepted value, without a launch: sizes and options are checked before the B == 0 return)
    assert _call(lib, B=0, opts=_options(max_steps=4096), out=0, path=0) == 0
    assert _call(lib, B=0, opts=_options(max_steps=4097), out=0, path=0) != 0 and b"max_steps" in lib.mpx_last_error()
    assert _call(lib, S=65) != 0 and b"65" in lib.mpx_last_error()
    assert _call(lib, M1=65, S=56) != 0 and b"64 cuboids" in lib.mpx_last_error()
    assert _call(lib, M1=4, S=0) != 0  # primitives without spheres to test them with
    for key, value, word in (("dt", 0.0, b"dt"), ("dt", float("nan"), b"dt"), ("lambda_", 0.0, b"lambda"),
                             ("step_clip", 0.0, b"step_clip"), ("attract", -1.0, b"attract"), ("damping", float("nan"), b"damping"),
                             ("epsilon", 0.0, b"epsilon"), ("speed_limit", 0.0, b"speed_limit"), ("switch_radius", -1.0, b"switch_radius"),
                             ("miss_tol", float("nan"), b"miss_tol"), ("switch_steps", 0, b"switch_steps"),
                             ("final_steps", 0, b"final_steps"), ("substeps", 0, b"substeps"), ("substeps", 65, b"substeps"),
                             ("check_margin", -1.0, b"check_margin"), ("clearance", float("nan"), b"clearance")):
        assert _call(lib, opts=_options(**{key: value})) != 0 and word in lib.mpx_last_error(), key
    assert _call(lib, B=-1) != 0 and b"negative size" in lib.mpx_last_error()
    assert _call(lib, B=(1 << 31) // 1025 + 1) != 0 and b"overflows int32" in lib.mpx_last_error()
    assert _call(lib, B=0, out=0, path=0) == 0  # nothing to do, nothing touched


def test_python_entry_point_refuses_cpu_tensors_and_unknown_options():
    from mpinets_amd import _lib, robot, scenes, solvers

    q, poses = torch.zeros(2, 7), torch.eye(4).repeat(2, 3, 1, 1)
    with pytest.raises(_lib.MpxError):
        robot.franka_follow(q, poses)
    with grid.recording():
        with pytest.raises(TypeError, match=r"^franka_follow: unknown option\(s\) \['iterations'\]$"):
            robot.franka_follow(q, poses, iterations=3)
    sig = inspect.signature(robot.franka_follow).parameters
    assert sig["T"].default == 50 and sig["return_path"].default is False and sig["return_state"].default is False
    assert "seed" not in sig and "env_offset" not in sig  # no randomness
    assert inspect.signature(scenes.make_problem_batch).parameters["hybrid"].default is False
    assert inspect.signature(scenes.problems_to_dataset).parameters["trajectory_key"].default == "global_solutions"
    with pytest.raises(ValueError):
        scenes.problems_to_dataset({}, "fabric_solutions")
    with pytest.raises(AssertionError):
        scenes.problems_to_dataset({"expert_valid": torch.ones(1, dtype=torch.bool)}, "hybrid_solutions")
    for name in ("FOLLOW_DEFAULTS", "FOLLOW_VALID", "FOLLOW_INVALID", "FOLLOW_BAD_INPUT", "FOLLOW_BIT_MISS", "_follow_options",
                 "franka_follow"):
        assert getattr(robot, name) is getattr(solvers, name), name
    assert (robot.FOLLOW_VALID, robot.FOLLOW_INVALID, robot.FOLLOW_BAD_INPUT, robot.FOLLOW_BIT_MISS) == (0, 1, 2, 8)
    # the Python defaults, the restatement's and the header's are one set
    assert robot.FOLLOW_DEFAULTS == ff.DEFAULTS
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    shared = {"lambda_": "MPX_IK_DEFAULT_LAMBDA", "step_clip": "MPX_IK_DEFAULT_STEP_CLIP", "epsilon": "MPX_PLAN_DEFAULT_EPSILON",
              "substeps": "MPX_PLAN_DEFAULT_SUBSTEPS", "check_margin": "MPX_PLAN_DEFAULT_CHECK_MARGIN",
              "max_jerk": "MPX_PLAN_DEFAULT_MAX_JERK"}
    for key, value in robot.FOLLOW_DEFAULTS.items():
        if key in ("clearance", "check_self"):
            continue
        m = re.search(r"#define %s\s+([0-9.e+-]+)f?" % shared.get(key, "MPX_FOLLOW_DEFAULT_" + key.upper()), text)
        assert m and float(m.group(1)) == pytest.approx(float(value), rel=1e-6), key
    assert re.search(r"#define MPX_FOLLOW_MAX_STEPS\s+4096", text) and robot.FOLLOW_MAX_STEPS == 4096
    copt, o = robot._follow_options("franka_follow", {"lambda": 0.1, "damping": 3.0, "check_self": 2})
    assert (round(copt.lambda_, 6), copt.damping, copt.check_self, copt.max_steps) == (0.1, 3.0, 1, 1024)
    assert robot._follow_options("franka_follow", {})[1] is robot.FOLLOW_DEFAULTS


@pytest.mark.parametrize("B", [0, 1, 3])
def test_the_recorded_call_fits_its_prototype(B):
    """``robot.franka_follow`` on CPU tensors with the library call recorded: over cuboids / cylinders / both / neither,
    with and without ``v_init`` / ``progress``, ``return_path``, ``return_state`` and options."""
    from mpinets_amd import _lib, robot

    q, poses = torch.zeros(B, 7), torch.eye(4).repeat(B, 5, 1, 1)
    v, pg = torch.zeros(B, 7), torch.zeros(B, 3, dtype=torch.int32)
    argtypes = _lib.PROTOTYPES["mpx_franka_follow"]
    for with_cub, with_cyl, state, ret_path, ret_state, opts in __import__("itertools").product((False, True), repeat=6):
        cub, cyl = grid._cuboids(B) if with_cub else None, grid._cylinders(B) if with_cyl else None
        o = dict(max_steps=37, repel=10.0, check_self=False) if opts else {}
        with grid.recording() as calls:
            out = robot.franka_follow(q, poses, cub, cyl, T=grid.T, v_init=v if state else None, progress=pg if state else None,
                                      return_path=ret_path, return_state=ret_state, **o)
        assert [n for n, _ in calls] == ["mpx_franka_follow"]
        args = calls[0][1]
        assert len(args) == len(argtypes) - 1  # (``_lib.call`` appends the stream)
        for i, (a, ctype) in enumerate(zip(args, argtypes)):
            try:
                ctype.from_param(a)
            except (TypeError, ctypes.ArgumentError) as e:
                raise AssertionError(f"argument {i} of mpx_franka_follow is {a!r}, not a {ctype.__name__}") from e
        rows = (37 if opts else 1024) + 1
        assert len(out) == 4 + 3 * ret_path + 3 * ret_state
        assert out[0].shape == (B, grid.T, 7) and all(t.shape == (B,) and t.dtype == torch.int32 for t in out[1:4])
        if ret_path:
            assert out[4].shape == (B, grid.T, 7) and out[5].shape == (B, rows, 7) and out[6].shape == (B, rows)
        if ret_state:
            assert out[-3].shape == out[-2].shape == (B, 7) and out[-1].shape == (B, 3) and out[-1].dtype == torch.int32
        assert args[2:5] == (B, 5, grid.T) and args[20]._obj.max_steps == rows - 1
        assert not (state and B) or (args[18], args[19]) == (v.data_ptr(), pg.data_ptr())
        assert (args[18] is None) == (not state) and (args[19] is None) == (not state)
        assert args[0] == q.data_ptr() and args[1] == poses.data_ptr()  # passed in place
        assert (args[27] is None) == (not ret_path) and all((a is None) == (not ret_state) for a in args[28:31])
        # (the sphere table only where there is a primitive to test)
        assert args[10] == (ft.collision_sphere_table(False)[0].shape[0] if with_cub or with_cyl else 0)


def test_a_bounded_path_buffer_runs_the_batch_in_slabs():
    """12 problems under a bound of 5 problems' dense path: calls of 5, 5 and 2 problems, every per-problem pointer advanced
    by its row, the shared operands and the one path buffer the same; with ``return_path`` one call over the whole batch."""
    from mpinets_amd import robot, solvers

    B, W, rows = 12, 5, 37 + 1
    q, poses = torch.zeros(B, 7), torch.eye(4).repeat(B, W, 1, 1)
    v, pg = torch.zeros(B, 7), torch.zeros(B, 3, dtype=torch.int32)
    cub, cyl = grid._cuboids(B), grid._cylinders(B)
    saved = solvers.FOLLOW_PATH_BYTES
    solvers.FOLLOW_PATH_BYTES = 5 * 32 * rows + 31
    try:
        with grid.recording() as calls:
            out = robot.franka_follow(q, poses, cub, cyl, T=grid.T, v_init=v, progress=pg, return_state=True, max_steps=37)
        with grid.recording() as whole:
            robot.franka_follow(q, poses, cub, cyl, T=grid.T, return_path=True, max_steps=37)
    finally:
        solvers.FOLLOW_PATH_BYTES = saved
    assert [n for n, _ in calls] == 3 * ["mpx_franka_follow"] and len(whole) == 1 and whole[0][1][2] == B
    a, b, c = (args for _, args in calls)
    assert [x[2] for x in (a, b, c)] == [5, 5, 2]
    # argument index -> 4-byte elements per problem behind that pointer
    per = {0: 7, 1: W * 16, 11: 2 * 16, 12: 2 * 3, 14: 3 * 16, 15: 3, 16: 3, 18: 7, 19: 3, 23: 1, 24: 1, 25: 1, 26: grid.T * 7,
           28: 7, 29: 7, 30: 3}
    first = {0: q, 1: poses, 11: cub.inv_frames, 12: cub.dims, 14: cyl.inv_frames, 15: cyl.radii, 16: cyl.heights, 18: v, 19: pg,
             23: out[1], 24: out[2], 25: out[3], 26: out[0], 28: out[4], 29: out[5], 30: out[6]}
    for i, row in per.items():
        p0 = first[i].data_ptr()
        assert [x[i] for x in (a, b, c)] == [p0, p0 + 5 * row * 4, p0 + 10 * row * 4], i
    for i in (3, 4, 5, 6, 7, 8, 9, 10, 13, 17, 21, 22):  # W, T, finger, limits, the sphere table, M1, M2, path, arc: the same
        assert a[i] == b[i] == c[i], i
    assert a[27] is None and a[20]._obj is b[20]._obj is c[20]._obj


def test_hybrid_refuses_the_cloud_expert():
    from mpinets_amd import scenes

    with pytest.raises(ValueError, match="hybrid"):
        scenes.make_problem_batch(1, device="cpu", collision_free=True, expert=True, expert_from="cloud", hybrid=True)


def test_follow_kernel_metadata():
    """The follow kernel's registers: no scratch and no VGPR spills.  It does spill SGPRs, into lanes of two VGPRs (an SGPR
    spill is a v_writelane / v_readlane, not memory): 30 kernel arguments, 25 of them pointers, and the saved comparison
    masks of its branches do not fit 106 SGPRs.  The count is printed and recorded in profiles/follow_timing.md."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "franka_follow_kernel" in n}
    assert len(hits) == 1
    (f,) = hits.values()
    print({k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0
    assert int(f[".group_segment_fixed_size"]) == 4 * (128 * 16 + 64 * 7)
