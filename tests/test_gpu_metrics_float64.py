"""GPU: every output of ``mpx_trajectory_metrics``, ``mpx_franka_success`` and ``mpx_franka_fk`` (csrc/franka.hip) against
the float64 restatement of tests/float64_metrics.py -- not against the float32 C mirror of the kernels, which shares
their formulas and so cannot see a mistake in one.

Every bar is ``float64_metrics.BARS``: 4x the difference between the float32 and the float64 run of the restatement on
the same inputs (tests/test_metrics_host.py derives them again on the CPU).  Every figure is printed before it is asserted.

Measured on an MI355X with the library as it was before (acos of the trace; summed over the path, always upward):
orientation path off by up to +0.40 deg at T = 150 (full 93 / 98 deg reaches: +0.05, +0.11) and up to +10.8 deg at
T = 2000 (full reaches: +9.3 on 58 deg, +7.0 on 93 deg); orientation error off by 0.04 deg at a 0 deg target, 0.028 at
180 deg, 5.6e-5 at 14.99 deg.  With the atan2 form: 1.4e-4 deg at T = 150 (bar 4.6e-4), 4.6e-4 deg at T = 2000 (bar
1.35e-3), at most 9.8e-6 deg at every constructed target (bar 3.5e-5)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_metrics as fm  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOATS = ("position_error", "orientation_error", "eff_position_path_length", "eff_orientation_path_length")
FLAGS = ("joint_limit_violation", "self_collision")


def evaluate(traj, targets, lengths=None):
    """``BatchedEvaluator.evaluate_trajectories`` -> the kernel's six outputs as numpy arrays."""
    from mpinets_amd.metrics import BatchedEvaluator

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    got = BatchedEvaluator(DEV).evaluate_trajectories(T(traj), T(targets), None if lengths is None else T(lengths))
    torch.cuda.synchronize()
    return {k: got[k].cpu().numpy() for k in FLOATS + FLAGS}


def report(what, got, ref, bar):
    d = np.abs(got.astype(np.float64) - ref)
    i = int(d.argmax())
    print(f"{what}: max |kernel - float64| {d.max():.3e} (row {i}: {got[i]:.9g} vs {ref[i]:.12g}), bar {bar:.3e}")
    return d.max()


def compare_flags(got, ref, what, n_left_out_max):
    """limit flag: the float64 comparison, every row.  Self collision: rows whose float64 margin exceeds the position bar."""
    np.testing.assert_array_equal(got["joint_limit_violation"], ref["joint_limit_violation"], err_msg=what)
    keep = ref["self_margin"] > fm.BARS["fk_translation"]
    print(f"{what}: self collision {int(ref['self_collision'].sum())} of {len(keep)} hit, {int((~keep).sum())} rows left out")
    assert (~keep).sum() <= n_left_out_max
    np.testing.assert_array_equal(got["self_collision"][keep], ref["self_collision"][keep], err_msg=what)


@pytest.mark.parametrize("T", fm.TRAJECTORY_T)
def test_trajectory_metrics_against_float64(T):
    """Minimum-jerk reaches and random walks of T waypoints; lengths {1, 2, 63, 64, 65, 127, 128, 129, T} in one batch (the
    64-waypoint pass boundaries and the carried slot 64), ``lengths=None``, and tails of NaN / inf / huge numbers past
    ``lengths[b]``, which must not change a single bit."""
    traj, lengths, goals = fm.trajectory_cases(T)
    tg = fm.poses_of(goals)
    worst = {}
    for name, ln in (("lengths", lengths), ("None", None)):
        ref = fm.trajectory_metrics(traj, ln, tg)
        got = evaluate(traj, tg, ln)
        for k in FLOATS:
            bar = fm.BARS["traj_" + k]
            bar = bar[T] if isinstance(bar, dict) else bar
            worst[name, k] = (report(f"T = {T}, lengths = {name}, {k}", got[k], ref[k], bar), bar)
        if T >= 150 and ln is None:  # (rows 8 and 17: full-length reaches)
            print(f"T = {T}: orientation path of the full reaches, kernel - float64 = "
                  f"{got['eff_orientation_path_length'][[8, 17]] - ref['eff_orientation_path_length'][[8, 17]]} "
                  f"on {ref['eff_orientation_path_length'][[8, 17]]} deg")
        compare_flags(got, ref, f"T = {T}, lengths = {name}", 0)
        if ln is not None:
            junk = evaluate(fm.with_garbage_tail(traj, ln), tg, ln)
            for k in FLOATS + FLAGS:
                assert junk[k].tobytes() == got[k].tobytes(), f"T = {T}: the tail past lengths[b] changed {k}"
            assert (got["eff_position_path_length"][ln == 1] == 0).all() and (got["eff_orientation_path_length"][ln == 1] == 0).all()
    for (name, k), (d, bar) in worst.items():
        assert d <= bar, f"T = {T}, lengths = {name}, {k}: {d:.3e} > {bar:.3e}"


def test_lengths_are_clamped_to_1_T():
    traj, lengths, goals = fm.trajectory_cases(150)
    tg = fm.poses_of(goals)
    wild = lengths.copy()
    wild[:4], wild[4:8] = [0, -3, 0, -1], [151, 1000, 2 ** 30, 150]
    a, b = evaluate(traj, tg, wild), evaluate(traj, tg, np.clip(wild, 1, 150))
    for k in FLOATS + FLAGS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_closed_forms_on_the_device():
    """Only joint 7 moves: orientation path = sum |dq7|, position path 0.  Only joint 1 moves: orientation path = sum |dq1|,
    position path = the chords of the gripper's circle about the z axis.  Out and back = twice one way (additive, not
    net).  The expected values are the closed forms (float64 of the float32 waypoints), not a run of any FK."""
    n = fm.CLOSED_PER_KIND
    traj, closed = fm.closed_form_cases()
    T = traj.shape[1]
    tg = fm.poses_of(traj[:, -1])
    got = evaluate(traj, tg)
    one_way = fm.trajectory_metrics(traj[2 * n:], np.full(n, T // 2), tg[2 * n:])
    _, t = fm.fk(traj[n:2 * n, 0])
    r = torch.linalg.norm(t[:, fm.GRIPPER, :2], dim=-1).numpy()
    want_rot = np.concatenate([closed["joint7_orientation"], closed["joint1_orientation"], 2 * one_way["eff_orientation_path_length"]])
    want_pos = np.concatenate([np.zeros(n), r * closed["joint1_chord_factor"], 2 * one_way["eff_position_path_length"]])
    bar_rot, bar_pos = fm.BARS["closed_eff_orientation_path_length"], fm.BARS["closed_eff_position_path_length"]
    res = []
    for name, rows in (("joint 7 only", slice(0, n)), ("joint 1 only", slice(n, 2 * n)), ("out and back", slice(2 * n, 3 * n))):
        res.append((report(f"{name}, orientation path", got["eff_orientation_path_length"][rows], want_rot[rows], bar_rot), bar_rot))
        res.append((report(f"{name}, position path", got["eff_position_path_length"][rows], want_pos[rows], bar_pos), bar_pos))
    assert all(d <= bar for d, bar in res), res
    # the device, too, gives the one-way length for the first half
    half = evaluate(traj[2 * n:], tg[2 * n:], np.full(n, T // 2, np.int32))
    assert np.abs(half["eff_orientation_path_length"] - one_way["eff_orientation_path_length"]).max() <= bar_rot


def test_orientation_error_at_constructed_targets():
    """Targets turned from the final pose about a random axis by 0, 1e-3, 0.1, 14.99, 15.01, 90, 179.9 and 180 degrees:
    where acos of the trace has no digits left (0, 180) and at the two sides of the 15 degree success threshold."""
    q, tg, deg = fm.rotated_target_cases()
    ref = fm.trajectory_metrics(q[:, None], None, tg)
    got = evaluate(q[:, None], tg)
    bar = fm.BARS["rotated_orientation_error"]
    worst = [report(f"target turned by {a} deg", got["orientation_error"][rows], ref["orientation_error"][rows], bar)
             for a, rows in ((a, slice(i * fm.ROTATED_PER_ANGLE, (i + 1) * fm.ROTATED_PER_ANGLE)) for i, a in enumerate(fm.ROTATED_ANGLES))]
    assert max(worst) <= bar
    assert ((got["orientation_error"] < 15) == (deg < 15)).all()  # what BatchedEvaluator's `success` asks
    assert report("position error at the final position", got["position_error"], ref["position_error"],
                  fm.BARS["rotated_position_error"]) <= fm.BARS["rotated_position_error"]


def call_success(q, targets, done, steps, cos_tol=fm.COS_15):
    from mpinets_amd import _lib

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    B = len(q)
    tq, tt, d, s = T(q), T(targets), T(done), T(steps)
    pe, ca = torch.full((B,), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
    _lib.call("mpx_franka_success", _lib.ptr(tq), _lib.ptr(tt), B, ft.FINGER_OPENING, 0.01, cos_tol, _lib.ptr(d), _lib.ptr(s),
              _lib.ptr(pe), _lib.ptr(ca))
    torch.cuda.synchronize()
    return pe.cpu().numpy(), ca.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy()


def test_success_against_float64():
    """``pos_err`` and ``cos_angle`` to the bar; ``done`` = the float64 decision wherever its margin exceeds the bar; the
    step counter counts only rows not yet done (as they were BEFORE the call); a row already done stays done."""
    q, tg, done, steps = fm.success_cases()
    ref = fm.success(q, tg, done, steps)
    pe, ca, d1, s1 = call_success(q, tg, done, steps)
    bp, bc = fm.BARS["success_pos_err"], fm.BARS["success_cos_angle"]
    dp, dc = report("success pos_err", pe, ref["pos_err"], bp), report("success cos_angle", ca, ref["cos_angle"], bc)
    keep = fm.success_decidable(ref, bp, bc)
    print(f"success: {int((~keep).sum())} of {len(q)} rows left out, {int(ref['decision'].sum())} decided true")
    assert dp <= bp and dc <= bc
    assert (~keep).sum() <= len(q) // 100
    np.testing.assert_array_equal(d1[keep], ref["done"][keep])
    np.testing.assert_array_equal(s1, ref["steps"])
    was = done != 0
    assert (d1[was] == 1).all() and (~ref["decision"][was]).any()  # done rows stay done, also where the test now fails
    assert np.array_equal(s1[was], steps[was]) and np.array_equal(s1[~was], steps[~was] + 1)
    # a second call from the state the first one left: rows that were done by then do not count another step
    _, _, d2, s2 = call_success(q, tg, d1, s1)
    np.testing.assert_array_equal(s2, s1 + (d1 == 0))
    np.testing.assert_array_equal(d2, d1)


def test_joint_limit_flag_next_to_every_published_bound():
    """One joint of the middle waypoint on the float32 nearest to each of the 14 published bounds, and one float32 below /
    above it: the flag equals the float64 comparison with the bound as published, in every one of the 42 rows (for 11
    bounds the nearest float32 lies outside the bound: the evaluator hands the kernel limits rounded inward)."""
    traj, what = fm.limit_neighbour_cases()
    tg = fm.poses_of(traj[:, -1])
    ref = fm.trajectory_metrics(traj, None, tg)
    got = evaluate(traj, tg)
    wrong = [w for w, g, r in zip(what, got["joint_limit_violation"], ref["joint_limit_violation"]) if bool(g) != bool(r)]
    print(f"limit neighbours: {int(ref['joint_limit_violation'].sum())} of 42 outside; kernel differs at (joint, side, offset) {wrong}")
    assert not wrong
    assert 14 < ref["joint_limit_violation"].sum() < 42 - 14


def test_self_collision_flag_against_float64():
    """2048 configurations uniform in the published limits and 2048 around a folded arm: the flag equals the float64 one
    wherever the float64 clearance is further from zero than the position bar; at most 1 % of the rows may be left out
    (the float32 restatement leaves out none, tests/test_metrics_host.py)."""
    q = fm.self_collision_cases()
    tg = fm.poses_of(q)
    compare_flags(evaluate(q[:, None], tg), fm.trajectory_metrics(q[:, None], None, tg), "self-collision cases", len(q) // 100)


def test_fk_frames_against_float64():
    """All 15 frames of 4096 random configurations and of the 128 corners of the empirical limits."""
    from mpinets_amd.robot import franka_fk

    q = fm.fk_cases()
    got = franka_fk(torch.from_numpy(q).to(DEV)).cpu().numpy().astype(np.float64)
    ref = fm.fk_frames(q)
    assert got.shape == ref.shape == (4096 + 128, 15, 12)
    res = []
    for name, rows in (("random", slice(0, 4096)), ("corners", slice(4096, None))):
        for part, cols, key in (("rotation", slice(0, 9), "fk_rotation"), ("translation", slice(9, 12), "fk_translation")):
            d = np.abs(got[rows, :, cols] - ref[rows, :, cols]).max()
            print(f"FK {name}, {part}: max |kernel - float64| {d:.3e}, bar {fm.BARS[key]:.3e}")
            res.append((d, fm.BARS[key]))
    assert all(d <= bar for d, bar in res), res
