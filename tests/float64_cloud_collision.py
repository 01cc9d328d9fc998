"""Restatement of csrc/cloud_collision.hip (``mpx_franka_cloud_collision``) on the CPU, squared distances in float64.

Inputs are what the kernel itself works from: FLOAT32 sphere centres (``FrankaCollisionSampler.sphere_centers``, which the
kernel reproduces bit for bit; on a machine without a GPU the oracle's FK gives the same table within its own parity bar)
and float32 points.  ``dx = c.x - p.x`` (likewise y, z) is formed in float32 -- exactly the kernel's subtraction -- and
only then widened: ``d2 = dx^2 + dy^2 + dz^2`` in float64.  What is left between this and the device is the three
roundings of ``mpx_sqdist`` (one product, two fused multiply-adds, all terms non-negative): the device's d2 is within
``3 * 2^-24`` relative of the float64 value; the bands below use ``BAND = 4 * 2^-24``.

``R2`` is computed as the kernel computes it -- ``R = (r_s + point_radius) + clearance`` and ``R * R`` in float32 -- and
then widened.  A (sphere, point) pair is a definite hit when ``d2 < R2 (1 - BAND)``, a definite miss when
``d2 > R2 (1 + BAND)`` and UNDECIDED in between; an environment is undecided when it has no definite hit and at least one
undecided pair.  A point with a NaN or infinite coordinate has ``d2 = +inf`` here: never a hit, never nearest.

Also here: the shapes and the seeded inputs of tests/test_gpu_cloud_collision.py (``CASES``, ``make_case``), so that
tests/test_cloud_collision_host.py can show on the CPU that the restatement alone stays inside the undecided cap.
"""
import re
import os

import numpy as np

BAND = 4.0 * 2.0 ** -24
UNDECIDED_CAP = 0.02  # share of environments per case that may be undecided

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_constant(name):
    text = open(os.path.join(ROOT, "include", "mpinets_hip.h")).read()
    return int(re.search(r"#define %s\s+(\d+)" % name, text).group(1))


WAYPOINT_CHUNK = 64  # MPX_CLOUD_TC: waypoints one workgroup takes
TILE = 256           # MPX_CLOUD_TILE: points per LDS tile

# the robot's reach box the test clouds are uniform in (metres)
REACH_LO = np.array([-0.9, -0.9, -0.3], np.float32)
REACH_HI = np.array([0.9, 0.9, 1.2], np.float32)

# (B, T, with_base_link, N, point_radius, clearance): B in {1, 3, 70}, T in {1, 2, 50, chunk + 1}, S = 56 / 57,
# N in {1, 63, 64, 65, tile - 1, tile, tile + 1, 2 tile + 3}, both radii, both clearances -- and one T per
# pairs-per-thread instantiation of the launcher (T * S / 512 rounded up = 1 .. 8)
CASES = [
    (1, 1, False, 1, 0.0, 0.0),
    (3, 1, True, 63, 0.01, 0.0),
    (3, 1, False, 2 * TILE + 3, 0.0, 0.005),
    (3, 2, False, 64, 0.0, 0.005),
    (3, 2, True, 65, 0.01, 0.005),
    (3, 50, False, TILE - 1, 0.0, 0.0),
    (3, 50, True, TILE, 0.01, 0.0),
    (70, 2, False, TILE + 1, 0.0, 0.005),
    (70, 50, False, 65, 0.01, 0.0),
    (3, 50, True, 2 * TILE + 3, 0.0, 0.0),
    (3, WAYPOINT_CHUNK + 1, False, 2 * TILE + 3, 0.01, 0.005),
    (1, WAYPOINT_CHUNK + 1, True, TILE + 1, 0.0, 0.0),
    (2, 9, False, 65, 0.0, 0.0),    # 504 pairs: 2 per thread
    (2, 10, False, 65, 0.01, 0.0),  # 560: 4
    (2, 25, False, 65, 0.0, 0.005),  # 1400: 6
    (2, 32, False, 65, 0.0, 0.0),   # 1792: 8
    (2, 40, False, 65, 0.01, 0.005),  # 2240: 10
    (2, 64, True, 65, 0.0, 0.0),    # 3648: 16
]


def case_id(case):
    B, T, base, N, pr, cl = case
    return f"B{B}-T{T}-S{57 if base else 56}-N{N}-pr{pr}-cl{cl}"


def make_case(case, seed=None):
    """-> q float32 [B,T,7] (straight joint-space lines between two configurations inside the limits) and cloud float32
    [B,N,3] uniform in the reach box; seeded by the case itself."""
    from mpinets_amd import scenes

    B, T, base, N, pr, cl = case
    if seed is None:
        seed = 1000 + CASES.index(case) if case in CASES else 999
    q = scenes.linear_trajectories(B, T, seed)
    rng = np.random.default_rng(seed)
    cloud = (REACH_LO + rng.random((B, N, 3), dtype=np.float32) * (REACH_HI - REACH_LO)).astype(np.float32)
    return q, cloud


def oracle_centres(q, with_base_link):
    """Sphere centres float32 [B,T,S,3] by the oracle's FK on the CPU."""
    from mpinets_amd import franka_tables as ft
    from oracle import oracle as orc

    c, r, l, _ = ft.collision_sphere_table(with_base_link)
    B, T, _ = q.shape
    fr = orc.franka_fk(q.reshape(B * T, 7))
    return orc.transform_table(fr, c, l).reshape(B, T, -1, 3)


def radius2_device(radii, point_radius, clearance):
    """R * R as the kernel forms it, float32 [S]."""
    R = (np.asarray(radii, np.float32) + np.float32(point_radius)) + np.float32(clearance)
    return (R * R).astype(np.float32)


def pair_d2(centres, points):
    """centres float32 [P,3], points float32 [n,3] -> d2 float64 [P,n]: float32 differences, float64 squares and sum;
    +inf where the point has a non-finite coordinate."""
    c = np.asarray(centres, np.float32)
    p = np.asarray(points, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (c[:, None, :] - p[None, :, :]).astype(np.float64)  # the subtraction itself is float32
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    d2[:, ~np.isfinite(p).all(axis=1)] = np.inf
    d2[np.isnan(d2)] = np.inf
    return d2


def restate(centres, cloud, radii, point_radius=0.0, clearance=0.0, counts=None):
    """centres float32 [B,T,S,3], cloud float32 [B,N,3], radii [S] -> dict of
      d2_min     float64 [B,T,S]   (+inf for an environment without usable points)
      nearest    int64   [B,T,S]   lowest index attaining d2_min in float64 (-1 without points)
      in_band    callable(b, idx [T,S]) -> bool [T,S]: is idx a point whose float64 d2 is within BAND of the minimum
      hit, undecided  bool [B,T,S]: a definite hit / an undecided pair exists for this (waypoint, sphere)
      env_hit, env_undecided  bool [B]
    """
    centres = np.asarray(centres, np.float32)
    cloud = np.asarray(cloud, np.float32)
    B, T, S, _ = centres.shape
    N = cloud.shape[1]
    R2 = radius2_device(radii, point_radius, clearance).astype(np.float64)  # [S]
    d2_min = np.full((B, T, S), np.inf)
    nearest = np.full((B, T, S), -1, np.int64)
    hit = np.zeros((B, T, S), bool)
    und = np.zeros((B, T, S), bool)
    for b in range(B):
        n = N if counts is None else int(min(max(int(counts[b]), 0), N))
        if n == 0:
            continue
        d2 = pair_d2(centres[b].reshape(T * S, 3), cloud[b, :n]).reshape(T, S, n)
        d2_min[b] = d2.min(axis=2)
        any_finite = np.isfinite(d2_min[b])
        nearest[b] = np.where(any_finite, d2.argmin(axis=2), -1)
        r2 = R2[None, :, None]
        hit[b] = (d2 < r2 * (1 - BAND)).any(axis=2)
        und[b] = (np.abs(d2 - r2) <= BAND * r2).any(axis=2)

    def in_band(b, idx):
        idx = np.asarray(idx)
        n = N if counts is None else int(min(max(int(counts[b]), 0), N))
        ok = (idx >= 0) & (idx < n)
        c = centres[b].reshape(T * S, 3)
        p = cloud[b][np.clip(idx.reshape(-1), 0, max(N - 1, 0))] if N else np.zeros((T * S, 3), np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            d = (c - p).astype(np.float64)
        own = (d * d).sum(axis=1).reshape(T, S)
        own[~np.isfinite(own)] = np.inf
        with np.errstate(invalid="ignore"):
            return ok & np.isfinite(own) & (np.abs(own - d2_min[b]) <= BAND * d2_min[b])

    env_hit = hit.reshape(B, -1).any(axis=1)
    env_und = ~env_hit & und.reshape(B, -1).any(axis=1)
    return {"d2_min": d2_min, "nearest": nearest, "in_band": in_band, "hit": hit, "undecided": und,
            "env_hit": env_hit, "env_undecided": env_und}
