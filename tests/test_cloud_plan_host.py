"""CPU: the float64 restatement of the cloud planner (tests/float64_cloud_plan.py) stands on its own -- the refinement's
fma emulation, the bar and the leave-out cap of the GPU one-step test, the solved counts the GPU share tests compare
against -- and ``mpx_franka_plan_cloud`` refuses bad arguments on the host, before any launch."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_field as fcf  # noqa: E402
import float64_cloud_plan as fcp  # noqa: E402
import float64_plan as fp  # noqa: E402
from test_plan_host import host_problems  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402

NUM_POINTS = 4096
ONE_STEP_SCENES, ONE_STEP_SEED, ONE_STEP_B, ONE_STEP_POINT_RADIUS = 28, 21, 16, 0.01
SHARE_SCENES, SHARE_SEED, SHARE_POINT_RADIUS = 26, 3, 0.01


def mixed_problems(oracle, scenes_drawn, seed, keep=None):
    """Mixed scenes whose start and goal the CPU solves against the primitives, and the scenes' clouds
    (``scenes.sample_scene_clouds_host``, 4096 points each).  -> scn, q_start, q_goal, cloud float32 [B,4096,3]."""
    scn, qs, qg = host_problems(oracle, scenes_drawn, seed)
    if keep is not None:
        assert len(qs) >= keep
        scn, qs, qg = {k: v[:keep] for k, v in scn.items()}, qs[:keep], qg[:keep]
    return scn, qs, qg, fcp.scene_cloud_points(scn, NUM_POINTS, seed)


def one_step_inputs(oracle):
    """The inputs of tests/test_gpu_cloud_plan.py's one-step test: 16 mixed scenes, their clouds, all 8 candidates drawn at
    seed 5, env_offset 1000."""
    scn, qs, qg, cloud = mixed_problems(oracle, ONE_STEP_SCENES, ONE_STEP_SEED, ONE_STEP_B)
    return scn, qs, qg, cloud, fp.candidates(qs, qg, seed=5, env_offset=1000)


def host_field(cloud, point_radius, counts=None):
    grid = fcp.default_grid(fcp.truncation(point_radius))
    return fcf.build_fast(cloud, counts, grid), grid


def one_step_reference_difference(qs, qg, start, field, grid, point_radius):
    out = {}
    for dt in (torch.float64, torch.float32):
        lim = torch.from_numpy(fp.limits32(ft.JOINT_LIMITS_REAL)).to(dt)
        res = fcp.step(torch.from_numpy(start).to(dt), torch.from_numpy(fp.line(qs, qg, start.shape[2])).to(dt), field, grid,
                       lim[:, 0], lim[:, 1], point_radius, want_fragile=(dt == torch.float64))
        out[dt] = res[0].double() if isinstance(res, tuple) else res.double()
        if isinstance(res, tuple):
            fragile = res[1]
    d = (out[torch.float64] - out[torch.float32]).abs().amax(-1)[:, :, 1:-1]
    moved = float((out[torch.float64] - torch.from_numpy(start).double()).abs().max())
    return float(d[~fragile].max()), float(d.median()), float(fragile.float().mean()), moved


# what the bar of tests/test_gpu_cloud_plan.py's one-step test is 4x of (recorded on the CPU)
CLOUD_ONE_STEP_REFERENCE = 2.4e-7
LEFT_OUT_CAP = 0.01


def test_refinement_emulates_the_device_fma():
    rng = np.random.default_rng(0)
    traj = rng.uniform(-2, 2, size=(3, 2, 9, 7)).astype(np.float32)
    fine = fcp.refine32(traj, 4)
    assert fine.shape == (3, 2, 33, 7) and fine.dtype == np.float32
    assert np.array_equal(fine[:, :, ::4], traj)  # i = 0: the waypoint itself, bit for bit
    ref = fp.refine(torch.from_numpy(traj).double(), 4).numpy()
    assert np.abs(fine - ref).max() < 3e-7
    assert np.array_equal(fcp.refine32(traj, 1), traj)


def test_one_step_bar_can_be_derived_again(oracle):
    """Reference against reference on the inputs of the GPU one-step test: the float32 run of the restated step against
    the float64 run from the same float32 numbers.  The GPU bar is 4x the recorded figure; here the measurement is
    repeated and must land within a factor 2 of it.  The leave-out rule (a sphere with d within 1e-5 m of 0 or epsilon, D
    within 1e-5 of trunc, a centre within 1e-5 cells of a face; the last two only where d < epsilon, see
    ``float64_cloud_plan.obstacle_gradient``) stays under 1 % of the waypoints.  Measured: max 2.38e-7 rad (one float32
    ulp of a joint angle above 2 rad), median 5.8e-8, 0.11 % left out, the largest move of the step 0.16 rad."""
    scn, qs, qg, cloud, start = one_step_inputs(oracle)
    field, grid = host_field(cloud, ONE_STEP_POINT_RADIUS)
    worst, median, left_out, moved = one_step_reference_difference(qs, qg, start, field, grid, ONE_STEP_POINT_RADIUS)
    print(f"one step against a cloud, float32 vs float64 restatement: max {worst:.3e}, median {median:.3e}, left out "
          f"{left_out:.4f} of {len(qs)} x 8 x 48 waypoints, largest move {moved:.3e} rad")
    assert left_out <= LEFT_OUT_CAP
    assert moved > 1e-3
    assert CLOUD_ONE_STEP_REFERENCE / 2 <= worst <= CLOUD_ONE_STEP_REFERENCE * 2


# recorded by test_restatement_solved_counts: what tests/test_gpu_cloud_plan.py's share tests compare against
DETOUR_SOLVED, DETOUR_PLANNED = 7, 13
SHARE_SOLVED, SHARE_PLANNED = 25, 25
RECORDED_DISAGREEMENTS = 0


def test_restatement_solved_counts(oracle):
    """The restatement's whole solve, float64 and float32, on the forced detour drawn as a cloud (24 problems) and on
    the mixed scenes' clouds (about 24 problems): solved counts (recorded above) and the number of problems on which the
    two runs disagree about solved / unsolved.  Measured: the detour plans 13 of 24 (11 have an endpoint that touches
    the wall's balls or the robot itself: status 2) and solves 7 in float64 and in float32, choices 1 x 5 and 4 x 2; the
    25 mixed-scene problems are all solved by both (the line alone solves 24); 0 disagreements; 47 s on 16 threads."""
    t0 = time.time()
    qs, qg, lim, cloud, _ = fcp.detour_problems()
    _, st64, ch64, at64, b64 = fcp.solve(qs, qg, cloud, point_radius=fcp.WALL_POINT_RADIUS, limits=lim, seed=9)
    _, st32, _, _, _ = fcp.solve(qs, qg, cloud, point_radius=fcp.WALL_POINT_RADIUS, limits=lim, seed=9, dtype=torch.float32)
    _, st0, _, _, b0 = fcp.solve(qs, qg, cloud, point_radius=fcp.WALL_POINT_RADIUS, limits=lim, seed=9, iterations=0)
    planned = st64 != 2
    assert ((b0[planned, 0] & 1) != 0).all()  # the straight line of every planned problem runs through the wall
    dis_detour = int(((st64 == 0) != (st32 == 0)).sum())
    print(f"forced detour as a cloud: {int(planned.sum())} of {len(qs)} planned, float64 solved {int((st64 == 0).sum())}, "
          f"float32 {int((st32 == 0).sum())}, disagreements {dis_detour}, choice histogram "
          f"{np.bincount(ch64[st64 == 0], minlength=8).tolist()} ({time.time() - t0:.0f} s)")
    scn, qs, qg, cloud = mixed_problems(oracle, SHARE_SCENES, SHARE_SEED)
    _, s64, c64, _, bits64 = fcp.solve(qs, qg, cloud, point_radius=SHARE_POINT_RADIUS)
    _, s32, _, _, _ = fcp.solve(qs, qg, cloud, point_radius=SHARE_POINT_RADIUS, dtype=torch.float32)
    dis_share = int(((s64 == 0) != (s32 == 0)).sum())
    print(f"mixed scenes' clouds: {len(qs)} problems, {int((s64 != 2).sum())} planned, float64 solved {int((s64 == 0).sum())}, "
          f"float32 {int((s32 == 0).sum())}, disagreements {dis_share}, line alone {int((bits64[:, 0] == 0).sum())} "
          f"({time.time() - t0:.0f} s)")
    assert max(dis_detour, dis_share) <= RECORDED_DISAGREEMENTS + 2
    assert (int((st64 == 0).sum()), int(planned.sum())) == (DETOUR_SOLVED, DETOUR_PLANNED)
    assert (int((s64 == 0).sum()), int((s64 != 2).sum())) == (SHARE_SOLVED, SHARE_PLANNED)
    ok = s64 == 0
    assert (bits64[ok, :][np.arange(ok.sum()), c64[ok]] == 0).all()


def _call(lib, B=4, T=50, S=56, opts=None, traj=256, status=256, env_offset=0, grid="good", field=256, cloud=256, N=64,
          stride=3, point_radius=0.0, scratch=4096, scratch_bytes=None):
    from mpinets_amd import _lib

    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched
    sph = one if S else None
    g = None
    if grid is not None:
        kw = dict(lo=(0.0, 0.0, 0.0), h=0.1, nx=4, ny=4, nz=4, trunc=0.2)
        kw.update({} if grid == "good" else grid)
        g = _lib.FieldGrid((ctypes.c_float * 3)(*kw["lo"]), kw["h"], kw["nx"], kw["ny"], kw["nz"], kw["trunc"])
    K = 8 if opts is None else opts.candidates
    sub = 4 if opts is None else opts.substeps
    if scratch_bytes is None:
        scratch_bytes = max(int(lib.mpx_franka_plan_cloud_scratch(max(B, 0), T, K, sub)), 0)
    return lib.mpx_franka_plan_cloud(one, one, B, T, 0.025, one, sph, sph, sph, S, ctypes.c_void_p(field) if field else None,
                                     None if g is None else ctypes.byref(g), ctypes.c_void_p(cloud) if cloud else None,
                                     N * stride, stride, N, None, point_radius, None if opts is None else ctypes.byref(opts), 0,
                                     env_offset, ctypes.c_void_p(traj) if traj else None,
                                     ctypes.c_void_p(status) if status else None, None, None, None,
                                     ctypes.c_void_p(scratch) if scratch else None, scratch_bytes, None)


def test_scratch_size():
    from mpinets_amd import _lib

    lib = _lib.load()
    f = lib.mpx_franka_plan_cloud_scratch
    B, T, K, sub = 5, 50, 8, 4
    R = (T - 1) * sub + 1
    words = K * B * R * 7 + B * K * T * 7 + B * 14 + (K + 1) * B + B * K + B
    assert f(B, T, K, sub) == (4 * words + 15) // 16 * 16
    assert f(0, T, K, sub) == 0
    for bad in ((-1, T, K, sub), (B, 1, K, sub), (B, 65, K, sub), (B, T, 0, sub), (B, T, 17, sub), (B, T, K, 0), (B, T, K, 65)):
        assert f(*bad) == -1, bad
    assert f(1024, 50, 8, 4) < 64 << 20  # (a thousand problems at the defaults: 57 MB)


def test_bad_arguments_are_refused_on_the_host():
    """Every refusal of ``mpx_franka_plan`` and the new ones: a scratch that is too small, NULL or unaligned, a grid
    outside its limits, point_radius < 0, a point stride below 3."""
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
    assert _call(lib, S=0) != 0 and b"without collision spheres" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, step=0.0))) != 0 and b"step" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, epsilon=-1.0))) != 0 and b"epsilon" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, substeps=0))) != 0 and b"substeps" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, iterations=-1))) != 0 and b"iterations" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, smooth_weight=-1.0))) != 0 and b"smooth_weight" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, check_margin=-1.0))) != 0 and b"check_margin" in lib.mpx_last_error()
    assert _call(lib, opts=_lib.PlanOptions(**dict(good, clearance=float("nan")))) != 0 and b"NaN" in lib.mpx_last_error()
    assert _call(lib, env_offset=-1) != 0 and b"env_offset" in lib.mpx_last_error()
    # the new ones
    assert _call(lib, point_radius=-0.01) != 0 and b"point_radius" in lib.mpx_last_error()
    assert _call(lib, stride=2) != 0 and b"stride" in lib.mpx_last_error()
    need = int(lib.mpx_franka_plan_cloud_scratch(4, 50, 8, 4))
    assert _call(lib, scratch_bytes=need - 1) != 0 and b"scratch" in lib.mpx_last_error()
    assert _call(lib, scratch=0) != 0 and b"scratch" in lib.mpx_last_error()
    assert _call(lib, scratch=4100) != 0 and b"aligned" in lib.mpx_last_error()
    assert _call(lib, grid=None) != 0 and b"NULL grid" in lib.mpx_last_error()
    for bad, word in ((dict(h=0.0), b"spacing"), (dict(trunc=-1.0), b"trunc"), (dict(nx=1), b"nodes"), (dict(ny=1025), b"nodes"),
                      (dict(nx=1024, ny=1024, nz=17), b"in all")):
        assert _call(lib, grid=bad) != 0 and word in lib.mpx_last_error(), bad
    assert _call(lib, B=0, traj=0, status=0, scratch=0) == 0  # nothing to do, nothing touched
    assert _call(lib, B=0, T=65) != 0  # (refused even when there is nothing to do, as mpx_franka_plan does)


def test_python_entry_points_refuse_cpu_tensors_and_unknown_options():
    import inspect

    from mpinets_amd import _lib, robot, scenes

    q = torch.zeros(2, 7)
    with pytest.raises(_lib.MpxError):
        robot.franka_plan_cloud(q, q, torch.zeros(2, 8, 3))
    sig = inspect.signature(robot.franka_plan_cloud).parameters
    assert sig["T"].default == 50 and sig["return_all"].default is False and sig["point_radius"].default == 0.0
    assert sig["field"].default is None and sig["counts"].default is None
    sig = inspect.signature(scenes.make_problem_batch).parameters
    assert sig["expert_from"].default == "primitives"
    with pytest.raises(ValueError):
        scenes.make_problem_batch(0, device="cpu", expert_from="mesh")
    assert robot.plan_cloud_truncation(0.01, 0.0, 0.05, 0.03) == pytest.approx(fcp.truncation(0.01))
    rmax = float(ft.collision_sphere_table(False)[1].max())
    assert fcp.truncation() == pytest.approx(rmax + 0.05 + 0.06)


def test_new_kernels_use_no_scratch():
    """The build, the sampler, the select kernel and the planner for up to 8 candidates keep everything in registers
    (32 / 24 / 7 / 156 VGPRs, LDS 8204 B static for the build's two tiles); the 16-candidate build has 128 VGPRs and may
    spill, as ``franka_plan_kernel<16>`` does."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    meta = kernel_metadata(LIB)
    for key in ("cloud_field_build_kernel", "cloud_field_sample_kernel", "franka_plan_cloud_select_kernel",
                "franka_plan_cloud_kernelILi8E"):
        hits = {n: f for n, f in meta.items() if key in n}
        assert len(hits) == 1, key
        (f,) = hits.values()
        print(key, {k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
        assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0, key
