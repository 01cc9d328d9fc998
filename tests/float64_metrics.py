"""Restatement of ``mpx_trajectory_metrics``, ``mpx_franka_success`` and ``mpx_franka_fk`` (csrc/franka.hip) on the CPU, in
float64 by default: plain torch / numpy on ``oracle.fk_frames_torch`` (FK in the dtype asked for), no ctypes oracle.

In float64 it is the reference the GPU tests compare with (tests/test_gpu_metrics_float64.py).  ``dtype=torch.float32``
runs the same statements in float32: the reference-against-reference measurement that sets the bars (``BARS`` below;
tests/test_metrics_host.py repeats the measurement and holds every bar between 2x and 8x of it).

What it states, independently of the kernel's arithmetic:

* the angle between two rotations is ``atan2(|antisymmetric part of A B^T|, (trace - 1) / 2)`` (``float64_ik.rotvec``) --
  well conditioned at every angle, unlike ``acos`` of the trace near 0 and 180 degrees;
* ``lengths`` are clamped to [1, T]; waypoints past ``lengths[b]`` take no part in anything;
* joint limits: ``float64(q)`` of the float32 waypoint against the float64 limits AS GIVEN (no float32 cast of them);
* self collision: the four-sphere / body-cylinder model (``float64_ik.self_hits`` states the same test);
* every flag comes with its float64 MARGIN, the distance of the deciding quantity from its threshold, so that a test
  can leave out the rows that float32 arithmetic cannot decide.

The second half of the file builds the inputs ("case families") that the host test measures the bars on and the GPU
test runs the kernels on -- one definition, so the bars belong to the inputs they are applied to.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik as f64ik  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

GRIPPER = 14  # right_gripper, the last of the 15 frames
SELF_SPHERES = ((7, 0.1), (9, 0.01), (12, 0.01), (13, 0.01))  # (frame, radius) against the body cylinder of radius 0.15
COS_15 = float(np.cos(np.radians(15.0)))


# ---------------------------------------------------------------------------------------------- the restatement
def fk(q, finger=ft.FINGER_OPENING, dtype=torch.float64):
    """q [N,7] (numpy float32, the kernel's input) -> R [N,15,3,3], t [N,15,3] torch tensors in ``dtype``."""
    return orc.fk_frames_torch(torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dtype).reshape(-1, 7), finger)


def fk_frames(q, finger=ft.FINGER_OPENING, dtype=torch.float64):
    """-> float64 numpy [N,15,12] in the layout ``mpx_franka_fk`` writes (R row-major, then t)."""
    R, t = fk(q, finger, dtype)
    return torch.cat([R.reshape(R.shape[0], 15, 9), t], dim=-1).double().numpy()


def angle_deg(A, B):
    """angle of A B^T in degrees, tensors [...,3,3]."""
    _, theta = f64ik.rotvec(A, B)
    return torch.rad2deg(theta)


def self_clearance(t):
    """t [N,15,3] frame origins -> [N]: min over the four spheres of (distance to the body segment - 0.15 - radius);
    negative = hit (the strict ``d < 0.15 + r`` of the kernel)."""
    worst = None
    for link, radius in SELF_SPHERES:
        c = t[:, link]
        dz = c[:, 2] - torch.clamp(c[:, 2], -0.3, 0.333)
        d = torch.sqrt(c[:, 0] ** 2 + c[:, 1] ** 2 + dz ** 2) - (0.15 + radius)
        worst = d if worst is None else torch.minimum(worst, d)
    return worst


def trajectory_metrics(traj, lengths, targets, limits=ft.JOINT_LIMITS_PUBLISHED, finger=ft.FINGER_OPENING,
                       dtype=torch.float64):
    """traj float32 [B,T,7], lengths int [B] or None, targets float32 [B,4,4], limits float64 [7,2] -> dict of numpy
    arrays [B]: the six outputs of the kernel under ``BatchedEvaluator``'s names (float64 / bool) plus ``limit_margin``
    [rad] and ``self_margin`` [m]."""
    traj = np.ascontiguousarray(traj, dtype=np.float32)
    B, T, _ = traj.shape
    ln = np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 1, T)
    valid = np.arange(T)[None, :] < ln[:, None]  # [B,T]
    clean = np.where(valid[:, :, None], traj, traj[:, :1])  # rows past the end: never looked at, whatever they hold
    # joint limits: float64 of the float32 waypoint against the limits as given
    lim = np.asarray(limits, dtype=np.float64)
    q64 = clean.astype(np.float64)
    over = np.maximum(lim[:, 0] - q64, q64 - lim[:, 1]).max(axis=(1, 2))  # > 0: outside (the tail repeats waypoint 0)
    R, t = fk(clean.reshape(-1, 7), finger, dtype)
    clear = self_clearance(t).reshape(B, T)
    clear = torch.where(torch.from_numpy(valid), clear, torch.full_like(clear, float("inf"))).amin(dim=1)
    Rg, pg = R[:, GRIPPER].reshape(B, T, 3, 3), t[:, GRIPPER].reshape(B, T, 3)
    seg = torch.from_numpy(valid[:, 1:]).to(dtype)  # segment (t-1, t) counts when t < len
    path_pos = (torch.linalg.norm(pg[:, 1:] - pg[:, :-1], dim=-1) * seg).sum(dim=1)
    path_rot = (angle_deg(Rg[:, 1:], Rg[:, :-1]) * seg).sum(dim=1)
    last = torch.from_numpy(ln - 1)
    rows = torch.arange(B)
    tg = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float32)).to(dtype)
    pos_err = 100.0 * torch.linalg.norm(pg[rows, last] - tg[:, :3, 3], dim=-1)
    rot_err = angle_deg(Rg[rows, last], tg[:, :3, :3])
    n = lambda x: x.double().numpy()
    return {"position_error": n(pos_err), "orientation_error": n(rot_err), "eff_position_path_length": n(path_pos),
            "eff_orientation_path_length": n(path_rot), "joint_limit_violation": over > 0, "limit_margin": np.abs(over),
            "self_collision": n(clear) < 0, "self_margin": np.abs(n(clear))}


def success(q, targets, done, steps, pos_tol=0.01, cos_tol=COS_15, finger=ft.FINGER_OPENING, dtype=torch.float64):
    """q float32 [B,7], targets float32 [B,4,4], done / steps int32 [B] as they are BEFORE the call -> dict:
    ``pos_err`` [m], ``cos_angle`` ((trace(R_eff R_t^T) - 1) / 2), ``decision`` (err < pos_tol and cos > cos_tol, the
    tolerances being the float32 numbers the kernel receives), ``done`` / ``steps`` after the call, and the signed
    margins ``pos_margin`` = pos_tol - err, ``cos_margin`` = cos - cos_tol (positive: that condition holds)."""
    R, t = fk(q, finger, dtype)
    tg = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float32)).to(dtype)
    err = torch.linalg.norm(t[:, GRIPPER] - tg[:, :3, 3], dim=-1).double().numpy()
    cos = (0.5 * ((R[:, GRIPPER] * tg[:, :3, :3]).sum(dim=(1, 2)) - 1.0)).double().numpy()
    pt, ct = float(np.float32(pos_tol)), float(np.float32(cos_tol))
    decision = (err < pt) & (cos > ct)
    done, steps = np.asarray(done), np.asarray(steps)
    return {"pos_err": err, "cos_angle": cos, "decision": decision, "pos_margin": pt - err, "cos_margin": cos - ct,
            "done": ((done != 0) | decision).astype(np.int32), "steps": (steps + (done == 0)).astype(np.int32)}


def success_decidable(ref, pos_bar, cos_bar):
    """Rows whose decision survives an error of ``pos_bar`` in the position error and ``cos_bar`` in the cosine: both
    conditions hold by more than their bar, or one of them fails by more than its bar."""
    pm, cm = ref["pos_margin"], ref["cos_margin"]
    return ((pm > pos_bar) & (cm > cos_bar)) | (pm < -pos_bar) | (cm < -cos_bar)


# ---------------------------------------------------------------------------------------------- the bars
# Each bar = 4 x the largest difference between the float32 and the float64 run of the restatement above on the case
# family named (the measured value is in the comment; tests/test_metrics_host.py::test_bars_can_be_derived_again repeats
# every measurement and fails when a bar is below 2x or above 8x of it).  The factor covers what the kernel does not share
# with the torch float32 run: its own sincos, FMA contraction, the order of its 64-lane reduction.  Nothing here was
# derived from a kernel's output.  Units: position_error cm, angles degrees, path length / frames m.
TRAJECTORY_T = (1, 2, 50, 150, 500, 2000)
BARS = {
    # min-jerk reaches and random walks, T waypoints, lengths {1, 2, 63, 64, 65, 127, 128, 129, T} and None (trajectory_cases)
    "traj_position_error": 7.04e-5,  # measured 1.76e-5 cm
    "traj_orientation_error": 7.13e-5,  # measured 1.78e-5 deg
    "traj_eff_position_path_length": {1: 0.0, 2: 4.73e-7, 50: 3.57e-6, 150: 4.28e-6, 500: 1.68e-5, 2000: 2.14e-5},
    #                       measured {1: 0,   2: 1.18e-7, 50: 8.92e-7, 150: 1.07e-6, 500: 4.20e-6, 2000: 5.35e-6} m
    "traj_eff_orientation_path_length": {1: 0.0, 2: 3.89e-5, 50: 1.95e-4, 150: 4.64e-4, 500: 1.03e-3, 2000: 1.35e-3},
    #                          measured {1: 0,   2: 9.74e-6, 50: 4.88e-5, 150: 1.16e-4, 500: 2.59e-4, 2000: 3.37e-4} deg
    # the 3 x 16 closed-form trajectories at T = 150 (closed_form_cases)
    "closed_eff_position_path_length": 7.45e-7,  # measured 1.86e-7 m
    "closed_eff_orientation_path_length": 1.31e-4,  # measured 3.27e-5 deg
    # orientation error at targets rotated by 0 ... 180 degrees from the final pose (rotated_target_cases)
    "rotated_orientation_error": 3.47e-5,  # measured 8.67e-6 deg
    "rotated_position_error": 7.38e-5,  # measured 1.85e-5 cm (the target stands on the float64 final position)
    # mpx_franka_success (success_cases)
    "success_pos_err": 6.99e-7,  # measured 1.75e-7 m
    "success_cos_angle": 1.20e-6,  # measured 3.01e-7
    # mpx_franka_fk frames: 4096 random configurations and the 128 corners of the empirical limits (fk_cases)
    "fk_rotation": 9.79e-7,  # measured 2.45e-7
    "fk_translation": 9.87e-7,  # measured 2.47e-7 m
}


# What the reference Evaluator's recorded results (tests/golden/metrics_golden.npz) allow.  They were made on a FLOAT32
# forward kinematics (the generator's stand-in for robofin's FK), in float64 from there on; against the float64 FK here
# that is the float32 FK error: 2.5e-7 in a frame entry -> 2.5e-5 cm, about 1.4e-5 deg per angle, summed over up to 39
# segments for the path lengths.  Measured float64 restatement vs recorded (tests/test_metrics_host.py prints it):
# position error 5.4e-6 cm, orientation error 6.5e-6 deg, position path 2.1e-7 m, orientation path 2.1e-5 deg; allowed:
# 4x those -- three orders of magnitude below the 6e-2 / 5e-2 deg that acos of the trace needed.
GOLDEN_ATOL = {"position_error": 2.2e-5, "orientation_error": 2.7e-5, "eff_position_path_length": 8.4e-7,
               "eff_orientation_path_length": 8.3e-5}


# ---------------------------------------------------------------------------------------------- case families
def _inside(q):
    lim = ft.JOINT_LIMITS_REAL
    return np.clip(q, lim[:, 0] + 1e-3, lim[:, 1] - 1e-3)


def batch_lengths(T):
    """The 64-waypoint pass boundaries of the kernel (one wave, 64 waypoints per pass, slot 64 carries the last pose of a
    pass into the next), the two shortest trajectories and the full one."""
    return np.minimum(np.array([1, 2, 63, 64, 65, 127, 128, 129, T]), T).astype(np.int32)


def trajectory_cases(T, seed=0):
    """-> traj float32 [36,T,7], lengths int32 [36], goals float32 [36,7]: rows 0-17 minimum-jerk reaches of about 0.6 rad
    per joint over the T waypoints, rows 18-35 random walks (steps of 0.6 / sqrt(T) rad per joint); each length of
    ``batch_lengths(T)`` twice per kind, so rows 8, 17 (reaches) and 26, 35 (walks) run the full T.  The goal is 2 cm-ish
    away from the last valid waypoint on even rows and a random configuration on odd ones."""
    from mpinets_amd.scenes import random_configurations

    rng = np.random.default_rng(1000 * T + seed)
    B = 36
    a = _inside(random_configurations(B, 200 + T).astype(np.float64))
    s = np.linspace(0.0, 1.0, T) if T > 1 else np.zeros(1)
    s = 10 * s ** 3 - 15 * s ** 4 + 6 * s ** 5
    b = _inside(a + rng.uniform(0.4, 0.8, (B, 7)) * rng.choice([-1.0, 1.0], (B, 7)))
    traj = a[:, None] + s[None, :, None] * (b - a)[:, None]
    walk = a[18:, None] + np.cumsum(rng.standard_normal((18, T, 7)) * (0.6 / np.sqrt(T)), axis=1)
    traj[18:] = _inside(walk)
    traj = traj.astype(np.float32)
    lengths = np.tile(batch_lengths(T), 4)
    last = traj[np.arange(B), lengths - 1]
    goals = random_configurations(B, 300 + T)
    goals[::2] = last[::2] + rng.normal(0, 0.01, (B // 2, 7)).astype(np.float32)
    return traj, lengths, goals.astype(np.float32)


def with_garbage_tail(traj, lengths):
    """A copy whose waypoints past ``lengths[b]`` hold NaN, infinities and huge numbers."""
    out = traj.copy()
    junk = np.array([np.nan, np.inf, -np.inf, 1e30, -7.5, 3e4, 123.0], np.float32)
    for b, L in enumerate(lengths):
        out[b, L:] = np.roll(junk, b)
    return out


CLOSED_PER_KIND = 16


def closed_form_cases(T=150, seed=0):
    """-> traj float32 [48,T,7] and, in float64 from the float32 waypoints, the closed forms [16] each.  Sixteen random
    bases and amplitudes per kind:
    rows 0-15:  only joint 7 moves (a sweep with a reversal): orientation path = sum |dq7| in degrees, position path = 0
                (the gripper origin lies on the joint's axis);
    rows 16-31: only joint 1 moves: orientation path = sum |dq1|, position path = r x sum of 2 sin(|dq1| / 2), the chords
                of the circle of radius r = the gripper's distance from the z axis (the caller takes r from the FK);
    rows 32-47: out and back along a reach (waypoint T - 1 - k equals waypoint k): twice the one-way length, which the
                test takes from the restatement on the first half."""
    n = CLOSED_PER_KIND
    rng = np.random.default_rng(800 + seed)
    base = np.array([0.3, -0.6, -0.4, -2.0, 0.5, 1.9, 0.2]) + rng.uniform(-0.3, 0.3, (3 * n, 7))
    traj = np.repeat(base[:, None], T, axis=1)
    u = np.linspace(0.0, 1.0, T)
    traj[:n, :, 6] = 0.2 + rng.uniform(1.2, 1.9, (n, 1)) * np.sin(rng.uniform(2.0, 2.6, (n, 1)) * u)  # up, then partly back
    traj[n:2 * n, :, 0] = -1.5 + rng.uniform(1.5, 3.0, (n, 1)) * u ** 2
    half = T // 2
    leg = base[2 * n:, None] + np.sin(0.5 * np.pi * u[None, :half, None] / u[half - 1]) * rng.uniform(0.3, 0.6, (n, 1, 7)) \
        * rng.choice([-1.0, 1.0], (n, 1, 7))
    traj[2 * n:, :half] = leg
    traj[2 * n:, half:] = leg[:, -1:]
    traj[2 * n:, T - half:] = leg[:, ::-1]
    traj = np.clip(traj, ft.JOINT_LIMITS_PUBLISHED[:, 0] + 1e-2, ft.JOINT_LIMITS_PUBLISHED[:, 1] - 1e-2).astype(np.float32)
    q = traj.astype(np.float64)
    d7, d1 = np.abs(np.diff(q[:n, :, 6], axis=1)), np.abs(np.diff(q[n:2 * n, :, 0], axis=1))
    return traj, {"joint7_orientation": np.degrees(d7.sum(axis=1)), "joint1_orientation": np.degrees(d1.sum(axis=1)),
                  "joint1_chord_factor": (2.0 * np.sin(d1 / 2.0)).sum(axis=1)}


ROTATED_ANGLES = (0.0, 1e-3, 0.1, 14.99, 15.01, 90.0, 179.9, 180.0)
ROTATED_PER_ANGLE = 64


def axis_angle_matrix(axis, deg):
    """Rodrigues, float64: axis [N,3] (unit), deg [N] -> [N,3,3]."""
    th = np.radians(deg)[:, None, None]
    K = np.zeros((len(axis), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    return np.eye(3)[None] + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def rotated_target_cases(seed=0):
    """-> q float32 [512,7], targets float32 [512,4,4], nominal angle [512]: the target is the float64 final pose turned
    about a random axis by each of ``ROTATED_ANGLES`` (64 rows each), at the final position."""
    from mpinets_amd.scenes import random_configurations

    n = ROTATED_PER_ANGLE * len(ROTATED_ANGLES)
    q = random_configurations(n, 400 + seed)
    rng = np.random.default_rng(401 + seed)
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    deg = np.repeat(np.array(ROTATED_ANGLES), ROTATED_PER_ANGLE)
    R, t = fk(q)
    targets = np.tile(np.eye(4), (n, 1, 1))
    targets[:, :3, :3] = axis_angle_matrix(axis, deg) @ R[:, GRIPPER].numpy()
    targets[:, :3, 3] = t[:, GRIPPER].numpy()
    return q, targets.astype(np.float32), deg


def success_cases(seed=0):
    """-> q float32 [1024,7], targets float32 [1024,4,4], done int32 [1024], steps int32 [1024] (before the call).
    Quarters: near hits and misses (the target is the pose of a configuration about 0.007 rad per joint away); targets rotated by
    14 ... 16 degrees and shifted by 0.8 ... 1.2 cm (both thresholds approached from both sides); exact hits; far
    misses.  Every fifth row is already done, and the step counters start at different values."""
    from mpinets_amd.scenes import random_configurations

    n = 1024
    rng = np.random.default_rng(500 + seed)
    q = random_configurations(n, 501 + seed)
    k = n // 4
    qt = q.astype(np.float64).copy()
    qt[:k] += rng.normal(0, 0.007, (k, 7))
    qt[3 * k:] = random_configurations(k, 502 + seed)
    R, t = fk(qt.astype(np.float32))
    Rn, tn = R[:, GRIPPER].numpy().copy(), t[:, GRIPPER].numpy().copy()
    axis = rng.standard_normal((k, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    Rn[k:2 * k] = axis_angle_matrix(axis, rng.uniform(14.0, 16.0, k)) @ Rn[k:2 * k]
    shift = rng.standard_normal((k, 3))
    tn[k:2 * k] += shift / np.linalg.norm(shift, axis=1, keepdims=True) * rng.uniform(0.008, 0.012, (k, 1))
    targets = np.tile(np.eye(4), (n, 1, 1))
    targets[:, :3, :3], targets[:, :3, 3] = Rn, tn
    done = (np.arange(n) % 5 == 0).astype(np.int32)
    steps = rng.integers(0, 70, n).astype(np.int32)
    return q, targets.astype(np.float32), done, steps


def limit_neighbour_cases():
    """-> traj float32 [42,3,7], what [42] (joint, side, offset): the middle waypoint of a trajectory at the centre of the
    published limits has ONE joint on the float32 nearest to one of the 14 published bounds, or one float32 below / above it."""
    lim = ft.JOINT_LIMITS_PUBLISHED
    mid = lim.mean(axis=1).astype(np.float32)
    rows, what = [], []
    for j in range(7):
        for side in (0, 1):
            on = np.float32(lim[j, side])
            for off, v in ((-1, np.nextafter(on, np.float32(-np.inf))), (0, on), (1, np.nextafter(on, np.float32(np.inf)))):
                tr = np.tile(mid, (3, 1))
                tr[1, j] = v
                rows.append(tr), what.append((j, side, off))
    return np.stack(rows).astype(np.float32), what


def self_collision_cases(seed=0):
    """-> q float32 [4096,7]: 2048 configurations uniform in the PUBLISHED limits (they fold further than the empirical
    ones) and 2048 scattered (0.25 rad per joint) around a folded arm whose hand is inside the body cylinder."""
    rng = np.random.default_rng(600 + seed)
    lim = ft.JOINT_LIMITS_PUBLISHED
    a = lim[:, 0] + rng.random((2048, 7)) * (lim[:, 1] - lim[:, 0])
    folded = np.array([0.0, -1.7, 0.0, -3.0, 0.0, 0.3, 0.0])
    b = np.clip(folded + rng.normal(0, 0.25, (2048, 7)), lim[:, 0] + 1e-3, lim[:, 1] - 1e-3)
    return np.concatenate([a, b]).astype(np.float32)


def fk_cases():
    """-> q float32 [4096 + 128, 7]: random configurations, then every corner of the empirical limits."""
    from mpinets_amd.scenes import random_configurations

    lim = ft.JOINT_LIMITS_REAL
    corners = np.array([[lim[j, (c >> j) & 1] for j in range(7)] for c in range(128)])
    return np.concatenate([random_configurations(4096, 700), corners.astype(np.float32)]).astype(np.float32)


def poses_of(q):
    """float32 [N,4,4] right_gripper poses of q by the float64 FK (targets for the cases above)."""
    R, t = fk(q)
    out = np.tile(np.eye(4), (len(q), 1, 1))
    out[:, :3, :3], out[:, :3, 3] = R[:, GRIPPER].numpy(), t[:, GRIPPER].numpy()
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------- the measurement
def _gap(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def measure_reference_gaps():
    """float32 against float64 run of the restatement on every case family -> the same nested dict as ``BARS``."""
    f32 = torch.float32
    out = {"traj_eff_position_path_length": {}, "traj_eff_orientation_path_length": {}}
    pe, oe = 0.0, 0.0
    for T in TRAJECTORY_T:
        traj, lengths, goals = trajectory_cases(T)
        tg = poses_of(goals)
        for ln in (lengths, None):
            a, b = trajectory_metrics(traj, ln, tg), trajectory_metrics(traj, ln, tg, dtype=f32)
            pe, oe = max(pe, _gap(a["position_error"], b["position_error"])), max(oe, _gap(a["orientation_error"], b["orientation_error"]))
            for k in ("eff_position_path_length", "eff_orientation_path_length"):
                out["traj_" + k][T] = max(out["traj_" + k].get(T, 0.0), _gap(a[k], b[k]))
    out["traj_position_error"], out["traj_orientation_error"] = pe, oe
    traj, _ = closed_form_cases()
    tg = poses_of(traj[:, -1])
    a, b = trajectory_metrics(traj, None, tg), trajectory_metrics(traj, None, tg, dtype=f32)
    for k in ("eff_position_path_length", "eff_orientation_path_length"):
        out["closed_" + k] = _gap(a[k], b[k])
    q, tg, _ = rotated_target_cases()
    a, b = trajectory_metrics(q[:, None], None, tg), trajectory_metrics(q[:, None], None, tg, dtype=f32)
    for k in ("orientation_error", "position_error"):
        out["rotated_" + k] = _gap(a[k], b[k])
    q, tg, done, steps = success_cases()
    a, b = success(q, tg, done, steps), success(q, tg, done, steps, dtype=f32)
    out["success_pos_err"], out["success_cos_angle"] = _gap(a["pos_err"], b["pos_err"]), _gap(a["cos_angle"], b["cos_angle"])
    a, b = fk_frames(fk_cases()), fk_frames(fk_cases(), dtype=f32)
    out["fk_rotation"], out["fk_translation"] = _gap(a[..., :9], b[..., :9]), _gap(a[..., 9:], b[..., 9:])
    return out
