"""CPU: ``mpx_franka_cloud_collision_each`` and ``mpx_franka_ik_cloud`` refuse bad arguments on the host, before any
launch; the Python layer's signatures; the new kernels keep everything in registers; and the inputs of the GPU suites can
tell right from wrong, shown by the restatement (tests/float64_ik_cloud.py) alone."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik_cloud as f64  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402

ONE = 256  # any non-NULL "device pointer": validation fails before it is touched


def _p(v):
    return ctypes.c_void_p(v) if v else None


def _each(lib, B=4, T=50, S=56, N=64, stride=3, point_radius=0.0, clearance=0.0, q=ONE, cloud=ONE, hit=ONE, sph=ONE):
    s = _p(sph) if S else None
    return lib.mpx_franka_cloud_collision_each(_p(q), B, T, 0.025, s, s, s, S, _p(cloud), N * stride, stride, N, None,
                                               point_radius, clearance, None, _p(hit), None)


def _ik(lib, B=4, S=56, N=64, stride=3, point_radius=0.0, opts=None, q_out=ONE, status=ONE, poses=ONE, limits=ONE,
        cloud=ONE, sph=ONE, env_offset=0, scratch=4096, scratch_bytes=None):
    s = _p(sph) if S else None
    if scratch_bytes is None:
        scratch_bytes = max(int(lib.mpx_franka_ik_cloud_scratch(max(B, 0))), 0)
    return lib.mpx_franka_ik_cloud(_p(poses), B, 0.025, _p(limits), None, s, s, s, S, _p(cloud), N * stride, stride, N, None,
                                   point_radius, None if opts is None else ctypes.byref(opts), 0, env_offset, _p(q_out),
                                   _p(status), None, None, _p(scratch), scratch_bytes, None)


def test_scratch_size():
    from mpinets_amd import _lib

    f = _lib.load().mpx_franka_ik_cloud_scratch
    for B in (1, 5, 8192):
        assert f(B) == B * 64 * (7 + 3) * 4 and f(B) % 16 == 0
    assert f(0) == 0 and f(-1) == -1 and f(-7) == -1


def test_each_refuses_bad_arguments_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert lib.mpx_version() == 341
    err = lib.mpx_last_error
    for bad in (dict(B=-1), dict(T=-1), dict(S=-1), dict(N=-1)):
        assert _each(lib, **bad) != 0 and b"negative" in err(), bad
    assert _each(lib, S=65) != 0 and b"65" in err()
    assert _each(lib, point_radius=-0.01) != 0 and b"point_radius" in err()
    assert _each(lib, clearance=float("nan")) != 0 and b"NaN" in err()
    assert _each(lib, stride=2) != 0 and b"stride" in err()
    assert _each(lib, B=1 << 20, T=1 << 11) != 0 and b"overflows" in err()
    assert _each(lib, hit=0) != 0 and b"NULL output" in err()
    assert _each(lib, q=0) != 0 and b"NULL operand" in err()
    assert _each(lib, cloud=0) != 0 and b"NULL operand" in err()
    assert _each(lib, sph=0) != 0 and b"NULL operand" in err()
    # nothing to do, nothing touched
    assert _each(lib, B=0, q=0, cloud=0, hit=0) == 0
    assert _each(lib, T=0, q=0, cloud=0, hit=0) == 0
    assert _each(lib, B=0, S=65) != 0  # (refused even when there is nothing to do, as mpx_franka_cloud_collision does)


def test_ik_cloud_refuses_bad_arguments_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    err = lib.mpx_last_error
    good = dict(iterations=64, lambda_=0.05, step_clip=0.5, pos_tol=1e-3, rot_tol=8.7e-3, clearance=0.0, check_self=1)
    # inherited from mpx_franka_ik
    assert _ik(lib, q_out=0) != 0 and b"NULL output" in err()
    assert _ik(lib, status=0) != 0 and b"NULL output" in err()
    assert _ik(lib, poses=0) != 0 and b"NULL operand" in err()
    assert _ik(lib, limits=0) != 0 and b"NULL operand" in err()
    assert _ik(lib, S=65) != 0 and b"65" in err()
    assert _ik(lib, opts=_lib.IkOptions(**dict(good, iterations=0))) != 0 and b"iterations" in err()
    assert _ik(lib, opts=_lib.IkOptions(**dict(good, lambda_=0.0))) != 0 and b"lambda" in err()
    assert _ik(lib, opts=_lib.IkOptions(**dict(good, step_clip=0.0))) != 0 and b"step_clip" in err()
    assert _ik(lib, opts=_lib.IkOptions(**dict(good, pos_tol=-1.0))) != 0 and b"tolerance" in err()
    assert _ik(lib, opts=_lib.IkOptions(**dict(good, clearance=float("nan")))) != 0 and b"NaN" in err()
    assert _ik(lib, env_offset=-1) != 0 and b"env_offset" in err()
    assert _ik(lib, sph=0) != 0 and b"sphere table" in err()
    # inherited from the cloud check
    for bad in (dict(B=-1), dict(S=-1), dict(N=-1)):
        assert _ik(lib, **bad) != 0 and b"negative" in err(), bad
    assert _ik(lib, point_radius=-0.01) != 0 and b"point_radius" in err()
    assert _ik(lib, stride=2) != 0 and b"stride" in err()
    assert _ik(lib, B=1 << 25) != 0 and b"overflows" in err()
    # its own
    assert _ik(lib, S=0) != 0 and b"without collision spheres" in err()
    need = int(lib.mpx_franka_ik_cloud_scratch(4))
    assert _ik(lib, scratch_bytes=need - 1) != 0 and b"scratch" in err()
    assert _ik(lib, scratch=0) != 0 and b"scratch" in err()
    assert _ik(lib, scratch=4100) != 0 and b"aligned" in err()
    assert _ik(lib, B=0, q_out=0, status=0, poses=0, limits=0, cloud=0, scratch=0) == 0  # nothing to do, nothing touched
    assert _ik(lib, B=0, stride=2) != 0


def test_python_entry_points_refuse_cpu_tensors_and_unknown_options():
    from mpinets_amd import _lib, capture, robot

    pose, cloud, q = torch.eye(4)[None], torch.zeros(1, 8, 3), torch.zeros(1, 7)
    with pytest.raises(_lib.MpxError):
        robot.franka_ik_cloud(pose, cloud)
    with pytest.raises(TypeError, match="bogus"):
        robot.franka_ik_cloud(pose, cloud, bogus=1)
    with pytest.raises(_lib.MpxError):
        capture.plan_to_poses(cloud, q, pose)
    with pytest.raises(TypeError, match="bogus"):
        capture.plan_to_poses(cloud, q, pose, ik_options=dict(bogus=1))
    with pytest.raises(TypeError):
        capture.plan_to_poses(cloud, q, pose, bogus=1)
    with pytest.raises(_lib.MpxError):
        robot.FrankaCollisionSampler.check_cloud_each(object.__new__(robot.FrankaCollisionSampler), q, cloud)
    with pytest.raises(ValueError):
        robot.FrankaRealRobot.collision_free_ik(np.eye(4), cuboids=object(), cloud=np.zeros((8, 3), np.float32))
    with pytest.raises(ValueError):
        robot.FrankaRobot.collision_free_ik(np.eye(4), None, object(), cloud=np.zeros((8, 3), np.float32))

    def defaults(fn, **want):
        sig = inspect.signature(fn).parameters
        for k, v in want.items():
            assert sig[k].default == v and type(sig[k].default) is type(v), (fn.__name__, k, sig[k].default)
        return sig

    defaults(robot.FrankaCollisionSampler.check_cloud_each, counts=None, point_radius=0.0, clearance=0.0, active=None)
    sig = defaults(robot.franka_ik_cloud, counts=None, point_radius=0.0, q_init=None, seed=0, env_offset=0,
                   with_base_link=False, return_all=False, finger=ft.FINGER_OPENING)
    assert list(sig) == ["target_poses", "cloud", "counts", "point_radius", "q_init", "limits", "seed", "env_offset",
                         "with_base_link", "return_all", "finger", "options"]
    assert sig["limits"].default is ft.JOINT_LIMITS_REAL
    sig = defaults(capture.plan_to_poses, counts=None, point_radius=0.0, T=50, seed=0, env_offset=0, field=None,
                   ik_options=None, plan_options=None)
    assert list(sig)[:3] == ["cloud", "q_start", "target_poses"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.items() if n not in ("cloud", "q_start", "target_poses"))
    defaults(robot.FrankaRobot.collision_free_ik, cuboids=None, cylinders=None, cloud=None, counts=None, point_radius=0.0)
    assert "mpx_franka_ik_cloud" in _lib.PROTOTYPES and "mpx_franka_cloud_collision_each" in _lib.PROTOTYPES


def test_new_kernels_use_no_scratch():
    """The per-waypoint kernels (nine pairs-per-thread instantiations, with and without the cull), the select kernel and the
    two helpers keep everything in registers.  VGPRs of the per-waypoint kernels: 50 .. 117 without the cull, 51 .. 123 with
    it (the flag kernels: 50 .. 121 / 51 .. 120), LDS 32 B / 176 B static beside the dynamic tiles."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    meta = kernel_metadata(LIB)
    for key, count in (("franka_cloud_collision_each_kernel", 18), ("franka_ik_cloud_select_kernel", 1),
                       ("franka_ik_cloud_active_kernel", 1), ("cloud_each_zero_kernel", 1)):
        hits = {n: f for n, f in meta.items() if key in n}
        assert len(hits) == count, key
        for n, f in sorted(hits.items()):
            print(n, {k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
            assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, n
            assert all(int(f[k]) == 0 for k in NO_SCRATCH_FIELDS), n


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_collision_cases_decide_their_waypoints(case):
    """Every case of the GPU suite, at waypoint granularity: the restatement leaves at most 2 % of a case's waypoints
    undecided, by the oracle's sphere centres."""
    B, T, base, N, pr, cl = case
    q, cloud = f64.make_case(case)
    hit, und = f64.verdicts(f64.fcc.oracle_centres(q, base), cloud, ft.collision_sphere_table(base)[1], pr, cl)
    print(f"{f64.case_id(case)}: {int(hit.sum())} of {B * T} waypoints hit, {int(und.sum())} undecided")
    assert und.mean() <= f64.UNDECIDED_CAP


@pytest.mark.parametrize("N,point_radius", f64.IK_CASES)
def test_ik_inputs_can_tell_right_from_wrong(N, point_radius):
    """The two IK input cases by the restatement alone.  Recorded: 0.41 of the starts converge, no converged start has a
    self hit, 0 of 1536 starts undecided; N = 65, point_radius 0.02: status 0 / 1 / 2 = 22 / 2 / 0, 7 moved winners;
    N = 255, point_radius 0: 14 / 10 / 0, 9 moved."""
    tp, _ = f64.ik_targets()
    q, status, all_q, bits, und = f64.solve(tp, f64.ik_cloud(N), point_radius, seed=f64.IK_SEED, check_self=True)
    counts = np.bincount(status, minlength=3).tolist()
    moved = f64.moved_winners(bits, status)
    conv = (bits & 1) != 0
    print(f"N = {N}, point_radius {point_radius}: converged {conv.mean():.3f}, self hits among them "
          f"{int(((bits & 4) != 0).sum())}, status 0/1/2 = {counts}, moved winners {moved}, undecided {int(und.sum())} of {und.size}")
    assert counts[0] >= 3 and counts[1] >= 2 and moved >= 3
    assert und.mean() <= f64.UNDECIDED_CAP
    assert ((bits & 2) == 0)[~conv].all() and np.isnan(q[status != 0]).all() and np.isfinite(q[status == 0]).all()
