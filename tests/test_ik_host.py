"""CPU: the float64 restatement of the inverse kinematics (tests/float64_ik.py) stands on its own -- its starts are the
Philox draws the kernel makes, its solutions reach their targets -- and ``mpx_franka_ik`` refuses bad arguments on the
host, before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik as f64  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd import scenes  # noqa: E402


def host_targets(oracle, B, seed=0):
    return oracle.frames_to_4x4(oracle.franka_fk(scenes.random_configurations(B, seed))[:, oracle.RIGHT_GRIPPER_FRAME])


def test_vectorised_philox_is_the_oracles(oracle):
    rng = np.random.default_rng(0)
    for _ in range(32):
        ctr = rng.integers(0, 2 ** 32, 4, dtype=np.uint64)
        key = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
        got = f64.philox4x32_np(*ctr, *key)
        assert [int(g) for g in got] == oracle.philox4x32(ctr, key).tolist()


def test_starts_are_keyed_by_the_global_problem_id():
    lim = ft.JOINT_LIMITS_REAL
    a = f64.starts(40, lim, seed=3)
    b = f64.starts(25, lim, seed=3, env_offset=15)
    assert np.array_equal(a[15:, 1:], b[:, 1:])
    l32 = f64.limits32(lim)
    assert (a[:, 0] == np.clip(ft.DEFAULT_Q.astype(np.float32), l32[:, 0], l32[:, 1])).all()
    assert ((a.astype(np.float64) >= lim[:, 0]) & (a.astype(np.float64) <= lim[:, 1])).all()
    assert not np.array_equal(a[:, 1:], f64.starts(40, lim, seed=4)[:, 1:])
    u = (a[:, 1:] - lim[:, 0]) / (lim[:, 1] - lim[:, 0])
    assert abs(u.mean() - 0.5) < 0.01  # 40 x 63 x 7 uniforms


def test_restatement_round_trip_and_share(oracle):
    """4096 reachable targets, 64 seeds x 64 iterations, float64: every solved row is within 1 mm / 0.5 degrees of its
    target and inside the limits; share solved 0.9995 (4094 of 4096; one seed converges in 0.427 of the cases, seed 0
    -- from the neutral pose -- in 0.707)."""
    tp = host_targets(oracle, 4096)
    q, st, aq, ast = f64.solve(tp)
    ok = st == 0
    share = ok.mean()
    print(f"float64 restatement: share solved {share:.4f} ({ok.sum()} of {len(ok)}), converged seeds {(ast & 1).mean():.4f}, "
          f"seed 0 {(ast[:, 0] & 1).mean():.4f}")
    T = torch.from_numpy(tp).double()
    perr, theta = f64.pose_error(torch.from_numpy(q[ok]), T[ok, :3, :3], T[ok, :3, 3])
    assert float(perr.max()) <= 1e-3 and float(theta.max()) <= np.radians(0.5)
    lim = ft.JOINT_LIMITS_REAL  # (float64, as passed: the restatement clamps to their inward float32 rounding)
    assert ((q[ok] >= lim[:, 0]) & (q[ok] <= lim[:, 1])).all()
    assert np.isnan(q[~ok]).all()
    assert share >= 0.99
    # the rule: the lowest converged seed
    first = (ast & 1).argmax(1)
    assert np.array_equal(q[ok], aq[np.arange(len(st)), first][ok])


def one_step_reference_difference(tp, q0):
    """The restatement's step in float32 against float64 from the same float32 numbers -> (largest |dq| difference over
    the starts whose Jacobian's smallest singular value is >= 1e-3, median over all starts, starts left out)."""
    lim = torch.from_numpy(f64.limits32(ft.JOINT_LIMITS_REAL))
    out = {}
    for dt in (torch.float64, torch.float32):
        T, lm = torch.from_numpy(tp).to(dt), lim.to(dt)
        out[dt] = f64.step(torch.from_numpy(q0).to(dt), T[:, :3, :3], T[:, :3, 3], lm[:, 0], lm[:, 1]).double()
    J, _, _ = f64.jacobian(torch.from_numpy(q0).double())
    keep = torch.linalg.svdvals(J)[:, -1] >= 1e-3
    d = (out[torch.float64] - out[torch.float32]).abs().amax(1)
    return float(d[keep].max()), float(d.median()), int((~keep).sum())


# what the bars of tests/test_gpu_ik.py's one-step tests are 4x of (recorded on the CPU; the same at 1, 4 and 16 threads)
ONE_STEP_REFERENCE = {"given_start": 5.37e-4, "all_lanes": 3.55e-5}


def test_one_step_bars_can_be_derived_again(oracle):
    """Reference against reference on the inputs of the GPU one-step tests (targets from the oracle's FK instead of the
    device's): the float32 run of the restatement differs from the float64 run by 5.37e-4 rad at most over the 4096
    given starts (median 5.9e-7, 5 starts left out as near singular) and by 3.55e-5 over the 64 x 64 Philox starts
    (median 5.5e-7, 6 left out).  The GPU tests' bars are 4x these recorded figures; here the measurement is repeated
    and must land within a factor 2 of each (another BLAS or thread count moves the largest of 4096 values)."""
    cases = {
        "given_start": (host_targets(oracle, 4096), scenes.random_configurations(4096, 1)),
        "all_lanes": (np.repeat(host_targets(oracle, 64, seed=17), 64, 0),
                      f64.starts(64, ft.JOINT_LIMITS_REAL, seed=5, env_offset=1000).reshape(-1, 7)),
    }
    for name, (tp, q0) in cases.items():
        worst, median, left_out = one_step_reference_difference(tp, q0)
        print(f"{name}: float32 vs float64 restatement, max {worst:.3e}, median {median:.3e}, left out {left_out} of {len(q0)}")
        assert left_out <= len(q0) // 100
        assert ONE_STEP_REFERENCE[name] / 2 <= worst <= ONE_STEP_REFERENCE[name] * 2, name


def test_float32_limits_are_rounded_inward():
    """The limits the kernel clamps to never lie outside the float64 limits (the plain cast does, on 9 of the 14 empirical
    ones), in the package and in the restatement alike."""
    for lim in (ft.JOINT_LIMITS_REAL, ft.JOINT_LIMITS_PUBLISHED):
        got = ft.limits_float32_inward(lim)
        assert got.dtype == np.float32 and got.tobytes() == f64.limits32(lim).tobytes()
        assert (got[:, 0].astype(np.float64) >= lim[:, 0]).all() and (got[:, 1].astype(np.float64) <= lim[:, 1]).all()
        assert (np.abs(got.astype(np.float64) - lim) <= np.spacing(np.abs(lim).astype(np.float32))).all()
    assert (ft.limits_float32_inward(ft.JOINT_LIMITS_REAL) != ft.JOINT_LIMITS_REAL.astype(np.float32)).sum() == 9


def test_pick_is_the_first_free_seed():
    aq = np.arange(3 * 64 * 7, dtype=np.float64).reshape(3, 64, 7)
    ast = np.zeros((3, 64), np.int32)
    ast[0, 2], ast[0, 5], ast[0, 9] = 1 | 2, 1, 1  # seed 2 collides, 5 is free
    ast[1, 7] = 1 | 4  # only a self-colliding one
    q, st = f64.pick(aq, ast)
    assert st.tolist() == [0, 1, 2] and np.array_equal(q[0], aq[0, 5]) and np.isnan(q[1:]).all()


def _call(lib, B=4, S=0, opts=None, q_out=256, status=256, M1=0):
    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched
    sph = one if S else None
    return lib.mpx_franka_ik(one, B, 0.025, one, None, sph, sph, sph, S, one if M1 else None, one if M1 else None, M1,
                             None, None, None, 0, None if opts is None else ctypes.byref(opts), 0, 0,
                             ctypes.c_void_p(q_out) if q_out else None, ctypes.c_void_p(status) if status else None,
                             None, None, None)


def test_bad_arguments_are_refused_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert lib.mpx_version() == 341
    good = dict(iterations=64, lambda_=0.05, step_clip=0.5, pos_tol=1e-3, rot_tol=8.7e-3, clearance=0.0, check_self=0)
    assert _call(lib, q_out=0) != 0 and b"NULL output" in lib.mpx_last_error()
    assert _call(lib, status=0) != 0 and b"NULL output" in lib.mpx_last_error()
    assert _call(lib, S=65) != 0 and b"65" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.IkOptions(**dict(good, iterations=0))) != 0 and b"iterations" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.IkOptions(**dict(good, lambda_=0.0))) != 0 and b"lambda" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.IkOptions(**dict(good, step_clip=0.0))) != 0
    assert _call(lib, M1=65, S=56) != 0 and b"64 cuboids" in lib.mpx_last_error()
    assert _call(lib, M1=4, S=0) != 0  # primitives without spheres to test them with
    assert lib.mpx_franka_ik(ctypes.c_void_p(256), 4, 0.025, ctypes.c_void_p(256), None, None, None, None, 0, None, None, 0,
                             None, None, None, 0, None, 0, -1, ctypes.c_void_p(256), ctypes.c_void_p(256), None, None, None) != 0
    assert b"env_offset" in lib.mpx_last_error()
    assert _call(lib, B=0, q_out=0, status=0) == 0  # nothing to do, nothing touched


def test_python_entry_points_refuse_cpu_tensors_and_unknown_options():
    from mpinets_amd import _lib, robot

    with pytest.raises(_lib.MpxError):
        robot.franka_ik(torch.eye(4)[None])
    assert robot.FrankaRealRobot.JOINT_LIMITS is ft.JOINT_LIMITS_REAL and hasattr(robot.FrankaRobot, "collision_free_ik")
    import inspect

    assert inspect.signature(scenes.make_problem_batch).parameters["collision_free"].default is False


def test_option_helpers_merge_over_the_defaults(monkeypatch):
    """``robot._ik_options`` / ``_plan_options``: the defaults, the ``lambda`` alias, the refusal of unknown names, and the
    ``check_self`` default each IK entry hands over (the entries run on CPU tensors with the library call recorded)."""
    from types import SimpleNamespace

    from mpinets_amd import _lib, robot

    def fields(c):
        return {n: getattr(c, n) for n, _ in c._fields_}

    f32 = lambda d: {k: (np.float32(v) if isinstance(v, float) else int(v)) for k, v in d.items()}  # noqa: E731
    ik = fields(robot._ik_options("franka_ik", {}, check_self=False))
    want = dict(robot.IK_DEFAULTS, check_self=False)
    want["lambda_"] = want.pop("damping")
    assert ik == f32(want)
    copt, o = robot._plan_options("franka_plan", {})
    assert o == robot.PLAN_DEFAULTS and fields(copt) == f32(robot.PLAN_DEFAULTS)
    assert robot._plan_options("franka_plan_cloud", dict(candidates=3, clearance=0.05))[1] == dict(robot.PLAN_DEFAULTS, candidates=3, clearance=0.05)
    assert robot._plan_options("franka_plan", {"check_self": False})[0].check_self == 0
    assert robot._ik_options("franka_ik", {"check_self": True}, False).check_self == 1
    assert robot._ik_options("franka_ik", {"lambda": 0.25}, False).lambda_ == 0.25
    assert robot._ik_options("franka_ik_cloud", {"damping": 0.5, "iterations": 7}, True).iterations == 7
    for helper, who, more in ((robot._ik_options, "franka_ik", (True,)), (robot._ik_options, "franka_ik_cloud", (True,)),
                              (robot._plan_options, "franka_plan", ()), (robot._plan_options, "franka_plan_cloud", ())):
        with pytest.raises(TypeError, match=rf"^{who}: unknown option\(s\) \['bogus', 'zeta'\]$"):
            helper(who, {"zeta": 1, "bogus": 2}, *more)
    assert robot._plan_options("franka_plan", {"iterations": 3})[1] is not robot.PLAN_DEFAULTS  # (the defaults are never written)

    seen = {}
    monkeypatch.setattr(_lib, "require_cuda", lambda *t: None)
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.update({name: [x._obj for x in a if hasattr(x, "_obj")][0]}))
    poses = torch.eye(4)[None]
    robot.franka_ik(poses)
    assert seen["mpx_franka_ik"].check_self == 0
    box = SimpleNamespace(centers=torch.zeros(1, 2, 3), inv_frames=torch.zeros(1, 2, 16), dims=torch.ones(1, 2, 3))
    robot.franka_ik(poses, box)
    assert seen["mpx_franka_ik"].check_self == 1
    robot.franka_ik(poses, box, check_self=False)
    assert seen["mpx_franka_ik"].check_self == 0
    robot.franka_ik_cloud(poses, torch.zeros(1, 5, 3))
    assert seen["mpx_franka_ik_cloud"].check_self == 1


def test_ik_kernel_uses_no_scratch():
    """The 6x6 solve and the seven joint frames live in registers: no private segment, no spills."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, demangle_head, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if demangle_head(n) == "franka_ik_kernel"}
    assert len(hits) == 1
    (f,) = hits.values()
    print({k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
    assert all(int(f[k]) == 0 for k in NO_SCRATCH_FIELDS)
