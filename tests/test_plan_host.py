"""CPU: the float64 restatement of the trajectory planner (tests/float64_plan.py) stands on its own -- the metric's closed
form, the SDF gradient against central differences of the oracle's SDFs, the fixed points, the Philox keying -- the bars of
the GPU one-step test are derived here, and ``mpx_franka_plan`` refuses bad arguments on the host, before any launch."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik as fik  # noqa: E402
import float64_plan as fp  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd import scenes  # noqa: E402

MIXED = ("tabletop", "cubby", "dresser")


def host_problems(oracle, N, seed, M1=40, M2=16):
    """Mixed scenes with a collision-free start and goal per scene, all on the CPU: the poses of two uniform draws, solved
    against the scene by the float64 restatement of the inverse kinematics; the scenes where both solve are kept.
    -> scene arrays, q_start, q_goal (float32)."""
    scn = scenes.make_scenes(N, seed, MIXED, M1, M2)

    def poses(s):
        return oracle.frames_to_4x4(oracle.franka_fk(scenes.random_configurations(N, s))[:, oracle.RIGHT_GRIPPER_FRAME])

    qs, ss, _, _ = fik.solve(poses(seed), scene=scn, seed=seed)
    qg, sg, _, _ = fik.solve(poses(seed + 7), scene=scn, seed=seed + 7)
    ok = (ss == 0) & (sg == 0)
    return {k: v[ok] for k, v in scn.items()}, qs[ok].astype(np.float32), qg[ok].astype(np.float32)


def test_metric_inverse_closed_form():
    for n in (1, 6, 48, 62):
        M, A = fp.metric_inverse(n), fp.metric(n)
        assert float((M @ A - torch.eye(n, dtype=torch.float64)).abs().max()) < 1e-12, n


def test_smoothness_gradient_in_the_metric_is_the_distance_to_the_line():
    """A^-1 grad(1/2 sum |q_{t+1} - q_t|^2) = q - L for fixed endpoints: the smoothness term needs no matrix product."""
    rng = np.random.default_rng(0)
    for T in (3, 8, 50, 64):
        n = T - 2
        q = torch.from_numpy(rng.normal(size=(T, 7)))
        L = q[0] + (torch.arange(T, dtype=torch.float64) / (T - 1))[:, None] * (q[-1] - q[0])
        grad = 2 * q[1:-1] - q[:-2] - q[2:]  # A q_inner - (boundary terms)
        assert float((fp.metric_inverse(n) @ grad - (q[1:-1] - L[1:-1])).abs().max()) < 1e-10, T


def _gradient_scene():
    """Two cuboids (one with a roll / pitch quaternion: the reference's inverse frame is not a rotation there), two
    cylinders (one tilted), one zero-volume row of each kind."""
    scn = {"cuboid_centers": [[[0.4, 0.1, 0.3], [0.1, -0.4, 0.5], [0.0, 0.0, 0.0]]],
           "cuboid_dims": [[[0.3, 0.2, 0.25], [0.2, 0.4, 0.1], [0.0, 0.0, 0.0]]],
           "cuboid_quats": [[[0.9, 0.3, 0.2, 0.1], [1.0, 0.0, 0.0, 0.3], [1.0, 0.0, 0.0, 0.0]]],
           "cylinder_centers": [[[-0.3, 0.3, 0.2], [0.3, 0.5, 0.6], [0.0, 0.0, 0.0]]],
           "cylinder_radii": [[[0.1], [0.15], [0.0]]], "cylinder_heights": [[[0.3], [0.2], [0.0]]],
           "cylinder_quats": [[[1.0, 0.0, 0.0, 0.0], [0.8, 0.5, -0.2, 0.1], [1.0, 0.0, 0.0, 0.0]]]}
    return {k: np.asarray(v, np.float32) for k, v in scn.items()}


def test_sdf_gradient_matches_central_differences_of_the_oracle(oracle):
    scn = _gradient_scene()
    scene = fp.scene_from_arrays(scn)
    rng = np.random.default_rng(1)
    x = rng.uniform(-0.6, 0.9, size=(1, 4096, 3))
    best, grad, fragile = fp.sdf_min_grad(torch.from_numpy(x), scene, want_fragile=True)

    def oracle_min(p):
        p32 = p.astype(np.float32)
        return np.minimum(oracle.cuboid_sdf(scn["cuboid_centers"], scn["cuboid_dims"], scn["cuboid_quats"], p32),
                          oracle.cylinder_sdf(scn["cylinder_centers"], scn["cylinder_radii"], scn["cylinder_heights"],
                                              scn["cylinder_quats"], p32))

    # the value is the oracle's (float32) to its rounding
    assert np.abs(best.numpy() - oracle_min(x)).max() < 2e-6
    h = 1e-2  # float32 SDFs: a 2e-7 rounding over 2h = 1e-5 per component; the field is piecewise smooth, so keep points
    num = np.stack([(oracle_min(x + h * e) - oracle_min(x - h * e)) / (2 * h) for e in np.eye(3)], -1).astype(np.float64)
    # whose +-h stencil stays on one smooth piece: the restatement's gradient at the six stencil points agrees with the centre's
    same = np.ones(x.shape[:2], bool)
    for e in np.eye(3):
        for sgn in (-1, 1):
            _, g2, _ = fp.sdf_min_grad(torch.from_numpy(x + sgn * h * e), scene)
            same &= (np.abs(g2.numpy() - grad.numpy()).max(-1) < 0.05)
    keep = same & ~fragile.numpy()
    assert keep.mean() > 0.3
    assert np.abs(num - grad.numpy())[keep].max() < 0.03  # (curvature of the outside norm over h = 1 cm, 1 / distance)
    # the rolled cuboid's frame is NOT orthonormal: its gradient is not a unit vector everywhere, and still matches
    norms = np.linalg.norm(grad.numpy()[keep], axis=-1)
    assert norms.max() > 1.0 + 1e-3 or norms.min() < 1.0 - 1e-3


def test_straight_line_in_free_space_is_a_fixed_point():
    qs, qg = scenes.random_configurations(8, 0), scenes.random_configurations(8, 1)
    L = fp.line(qs, qg, 50)
    lim = torch.from_numpy(fp.limits32(ft.JOINT_LIMITS_REAL)).double()
    traj = torch.from_numpy(L).double()[:, None]
    out = fp.step(traj, torch.from_numpy(L).double(), None, lim[:, 0], lim[:, 1])
    assert torch.equal(out, traj)
    # a bent candidate relaxes toward the line at the rate step * smooth_weight
    c = torch.from_numpy(fp.candidates(qs, qg, seed=3)).double()
    out = fp.step(c, torch.from_numpy(L).double(), None, lim[:, 0], lim[:, 1])
    rate = fp.DEFAULTS["step"] * fp.DEFAULTS["smooth_weight"]
    assert 0 < rate < 1
    np.testing.assert_allclose((out - traj).numpy(), ((c - traj) * (1 - rate)).numpy(), atol=1e-12)


def test_candidates_are_keyed_by_the_global_problem_id():
    qs, qg = scenes.random_configurations(40, 0), scenes.random_configurations(40, 1)
    a = fp.candidates(qs, qg, seed=3)
    b = fp.candidates(qs[15:], qg[15:], seed=3, env_offset=15)
    assert np.array_equal(a[15:], b)
    assert np.array_equal(a[:, 0], fp.line(qs, qg, 50))  # candidate 0 is the line
    assert np.array_equal(a[:, :, 0], np.broadcast_to(qs[:, None], a[:, :, 0].shape))  # endpoints bit-equal
    assert np.array_equal(a[:, :, -1], np.broadcast_to(qg[:, None], a[:, :, -1].shape))
    other = fp.candidates(qs, qg, seed=4)
    assert np.array_equal(a[:, 0], other[:, 0]) and not np.array_equal(a[:, 1:], other[:, 1:])
    lim = ft.JOINT_LIMITS_REAL
    assert ((a.astype(np.float64) >= lim[:, 0]) & (a.astype(np.float64) <= lim[:, 1])).all()


def one_step_inputs(oracle):
    """The inputs of tests/test_gpu_plan.py's one-step test: 64 mixed scenes (seed 11), the endpoints solved on the CPU,
    all 8 candidates drawn at seed 5, env_offset 1000."""
    scn, qs, qg = host_problems(oracle, 64, 11)
    return scn, qs, qg, fp.candidates(qs, qg, seed=5, env_offset=1000)


def one_step_reference_difference(scn, qs, qg, start):
    """The restatement's step in float32 against float64 from the same float32 numbers -> (largest |q| difference over the
    interior waypoints that the leave-out rule keeps, median, share left out)."""
    scene = fp.scene_from_arrays(scn)
    out = {}
    for dt in (torch.float64, torch.float32):
        lim = torch.from_numpy(fp.limits32(ft.JOINT_LIMITS_REAL)).to(dt)
        res = fp.step(torch.from_numpy(start).to(dt), torch.from_numpy(fp.line(qs, qg, start.shape[2])).to(dt), scene,
                      lim[:, 0], lim[:, 1], want_fragile=(dt == torch.float64))
        out[dt] = res[0].double() if isinstance(res, tuple) else res.double()
        if isinstance(res, tuple):
            fragile = res[1]
    d = (out[torch.float64] - out[torch.float32]).abs().amax(-1)[:, :, 1:-1]  # [B,K,n]
    drop = fragile  # (the waypoints of the leave-out rule; measured: leaving their whole candidates out changes nothing)
    return float(d[~drop].max()), float(d.median()), float(drop.float().mean())


# what the bar of tests/test_gpu_plan.py's one-step test is 4x of (recorded on the CPU)
ONE_STEP_REFERENCE = 2.4e-7
LEFT_OUT_CAP = 0.01


def test_one_step_bar_can_be_derived_again(oracle):
    """Reference against reference on the inputs of the GPU one-step test: the float32 run of the restatement's step
    differs from the float64 run by 2.37e-7 rad at most (one float32 ulp of a joint angle above 2 rad; median 5.9e-8)
    over the waypoints the leave-out rule keeps (0.23 % are left out; the largest move of the step is 0.28 rad).  The GPU
    test's bar is 4x the recorded figure; here the measurement is repeated and must land within a factor 2 of it."""
    scn, qs, qg, start = one_step_inputs(oracle)
    worst, median, left_out = one_step_reference_difference(scn, qs, qg, start)
    print(f"one step, float32 vs float64 restatement: max {worst:.3e}, median {median:.3e}, left out {left_out:.4f} "
          f"of {len(qs)} x 8 x 48 waypoints")
    assert left_out <= LEFT_OUT_CAP
    assert ONE_STEP_REFERENCE / 2 <= worst <= ONE_STEP_REFERENCE * 2


# recorded by test_restatement_solved_share (the margin of the GPU share tests is 2x the disagreement count, at least 2)
SHARE_PROBLEMS, SHARE_SEED = 176, 0  # scenes drawn; the ~3 in 4 whose start and goal the CPU solves are the problems (>= 128)
RECORDED_DISAGREEMENTS = 0


def test_restatement_solved_share(oracle):
    """N mixed-scene problems with the default options, float64 and float32: the share solved, per-candidate validity and
    the number of problems on which the two runs disagree about solved / unsolved (recorded; no floor fixed in advance).
    Measured: 139 problems, share solved 0.9928 in float64 (62 s on 16 threads) and in float32, the line alone 0.9640,
    0 disagreements."""
    scn, qs, qg = host_problems(oracle, SHARE_PROBLEMS, SHARE_SEED)
    scene = fp.scene_from_arrays(scn)
    t0 = time.time()
    _, st64, ch64, _, bits64 = fp.solve(qs, qg, scene)
    t1 = time.time()
    _, st32, _, _, bits32 = fp.solve(qs, qg, scene, dtype=torch.float32)
    disagree = int(((st64 == 0) != (st32 == 0)).sum())
    print(f"restatement on {len(qs)} mixed-scene problems: share solved {np.mean(st64 == 0):.4f} (float64, {t1 - t0:.0f} s), "
          f"{np.mean(st32 == 0):.4f} (float32); status 2: {(st64 == 2).sum()}; per-candidate validity "
          f"{np.round((bits64 == 0).mean(0), 3).tolist()}; line alone {np.mean(bits64[:, 0] == 0):.4f}; "
          f"float32 / float64 disagreements {disagree}")
    assert disagree <= RECORDED_DISAGREEMENTS + 2
    assert np.mean(st64 == 0) >= np.mean(bits64[:, 0] == 0)  # (the line is candidate 0: optimising cannot lose what it had)
    ok = st64 == 0
    assert (bits64[ok, :][np.arange(ok.sum()), ch64[ok]] == 0).all()
    first = np.where((bits64 == 0).any(1), (bits64 == 0).argmax(1), -1)
    assert np.array_equal(first[st64 != 2], ch64[st64 != 2])


def test_pick_is_the_lowest_valid_candidate():
    at = np.arange(3 * 4 * 5 * 7, dtype=np.float64).reshape(3, 4, 5, 7)
    bits = np.array([[1, 4, 0, 0], [2, 1, 5, 7], [0, 0, 0, 0]], np.int32)
    traj, st, ch = fp.pick(at, bits)
    assert st.tolist() == [0, 1, 0] and ch.tolist() == [2, -1, 0]
    assert np.array_equal(traj[0], at[0, 2]) and np.isnan(traj[1]).all() and np.array_equal(traj[2], at[2, 0])


def _call(lib, B=4, T=50, S=0, M1=0, opts=None, traj=256, status=256, env_offset=0):
    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched
    sph = one if S else None
    cub = one if M1 else None
    return lib.mpx_franka_plan(one, one, B, T, 0.025, one, sph, sph, sph, S, cub, cub, M1, None, None, None, 0,
                               None if opts is None else ctypes.byref(opts), 0, env_offset,
                               ctypes.c_void_p(traj) if traj else None, ctypes.c_void_p(status) if status else None,
                               None, None, None, None)


def test_bad_arguments_are_refused_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert lib.mpx_version() == 341
    good = dict(candidates=8, iterations=10, step=1e-3, smooth_weight=1.0, epsilon=0.05, spread=0.5, substeps=4,
                check_margin=1e-4, clearance=0.0, max_jerk=0.15, check_self=1)
    assert _call(lib, traj=0) != 0 and b"NULL output" in lib.mpx_last_error()
    assert _call(lib, status=0) != 0 and b"NULL output" in lib.mpx_last_error()
    for T in (1, 65):
        assert _call(lib, T=T) != 0 and b"waypoints" in lib.mpx_last_error()
    for K in (0, 17):
        assert _call(lib, opts=_lib.PlanOptions(**dict(good, candidates=K))) != 0 and b"candidates" in lib.mpx_last_error()
    assert _call(lib, S=65) != 0 and b"65" in lib.mpx_last_error()
    assert _call(lib, M1=65, S=56) != 0 and b"64 cuboids" in lib.mpx_last_error()
    assert _call(lib, M1=4, S=0) != 0  # primitives without spheres to test them with
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, step=0.0))) != 0 and b"step" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, epsilon=-1.0))) != 0 and b"epsilon" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, substeps=0))) != 0 and b"substeps" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, iterations=-1))) != 0 and b"iterations" in lib.mpx_last_error()
    assert _call(lib, env_offset=-1) != 0 and b"env_offset" in lib.mpx_last_error()
    assert _call(lib, B=0, traj=0, status=0) == 0  # nothing to do, nothing touched


def test_python_entry_points_refuse_cpu_tensors_and_unknown_options():
    import inspect

    from mpinets_amd import _lib, robot

    q = torch.zeros(2, 7)
    with pytest.raises(_lib.MpxError):
        robot.franka_plan(q, q)
    sig = inspect.signature(robot.franka_plan).parameters
    assert sig["T"].default == 50 and sig["return_all"].default is False
    assert inspect.signature(scenes.make_problem_batch).parameters["expert"].default is False
    with pytest.raises(AssertionError):
        scenes.problems_to_dataset({"q": q})
    # the Python defaults, the restatement's and the header's are one set
    assert robot.PLAN_DEFAULTS == fp.DEFAULTS
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpinets_hip.h")).read()
    import re

    for key in ("candidates", "iterations", "step", "smooth_weight", "epsilon", "spread", "substeps", "check_margin", "max_jerk"):
        m = re.search(r"#define MPX_PLAN_DEFAULT_%s\s+([0-9.e+-]+)f?" % key.upper(), text)
        assert m and float(m.group(1)) == pytest.approx(float(robot.PLAN_DEFAULTS[key]), rel=1e-6), key


def test_plan_kernel_for_up_to_8_candidates_uses_no_scratch():
    """The seven joint frames, the waypoint and its gradient live in registers when a workgroup has at most 8 waves (256
    VGPRs each); the 16-candidate build has 128 and may spill."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "franka_plan_kernelILi8E" in n}
    assert len(hits) == 1
    (f,) = hits.values()
    print({k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0
