"""Restatement of ``mpx_franka_cloud_collision_each`` and ``mpx_franka_ik_cloud`` on the CPU, built from the two
restatements they are made of: tests/float64_cloud_collision.py (the pair test, its ``BAND`` and ``UNDECIDED_CAP``, the
18 ``CASES`` and ``make_case``) and tests/float64_ik.py (the solver and the first-free-start rule).

Per waypoint: a waypoint is a DEFINITE HIT when some (sphere, point) pair is a definite hit, UNDECIDED when it has no
definite hit and at least one pair in the band, a definite miss otherwise.

The IK inputs (``IK_CASES``): 24 targets, the right_gripper poses of ``scenes.random_configurations(24, 41)``, solved
with seed 3 and the self test on, against clouds uniform in the reach box,
``REACH_LO + default_rng(N).random((24, N, 3), float32) * (REACH_HI - REACH_LO)``.
"""
import numpy as np

import float64_cloud_collision as fcc
import float64_ik as fik

BAND, UNDECIDED_CAP = fcc.BAND, fcc.UNDECIDED_CAP
CASES, make_case, case_id, restate = fcc.CASES, fcc.make_case, fcc.case_id, fcc.restate

IK_B, IK_TARGET_SEED, IK_SEED = 24, 41, 3
IK_CASES = [(65, 0.02), (255, 0.0)]  # (N, point_radius)


def waypoint_verdicts(ref):
    """``restate``'s result -> (definite hit, undecided) bool [B,T]."""
    hit = ref["hit"].any(axis=2)
    return hit, ~hit & ref["undecided"].any(axis=2)


def verdicts(centres, cloud, radii, point_radius=0.0, clearance=0.0, counts=None):
    """centres float32 [B,T,S,3], cloud float32 [B,N,3] -> (definite hit, undecided) bool [B,T]."""
    return waypoint_verdicts(restate(centres, cloud, radii, point_radius, clearance, counts))


def ik_targets():
    """float32 [24,4,4] by the oracle's FK on the CPU, and the generating configurations float32 [24,7]."""
    from mpinets_amd import scenes
    from oracle import oracle as orc

    q = scenes.random_configurations(IK_B, IK_TARGET_SEED)
    return orc.frames_to_4x4(orc.franka_fk(q)[:, orc.RIGHT_GRIPPER_FRAME]).astype(np.float32), q


def ik_cloud(N, B=IK_B):
    rng = np.random.default_rng(N)
    return (fcc.REACH_LO + rng.random((B, N, 3), dtype=np.float32) * (fcc.REACH_HI - fcc.REACH_LO)).astype(np.float32)


def fold(all_q, all_status, hit):
    """Bits 0 and 2 of every start [B,64] and the cloud verdicts bool [B,64] -> (q, status, bits): bit 1 on the starts that
    converged and hit the cloud; the lowest start with bits == 1."""
    bits = (all_status & ~fik.BIT_ENV_HIT) | np.where(((all_status & fik.BIT_CONVERGED) != 0) & hit, fik.BIT_ENV_HIT, 0)
    bits = bits.astype(np.int32)
    return (*fik.pick(all_q, bits), bits)


def solve(target_poses, cloud, point_radius=0.0, counts=None, with_base_link=False, **kw):
    """-> q [B,7], status [B], all_q [B,64,7], bits [B,64], undecided bool [B,64]: ``float64_ik.solve`` without a scene,
    then the cloud verdict of every start's configuration (sphere centres by the oracle's FK of the float32 cast)."""
    from mpinets_amd import franka_tables as ft

    clearance = kw.get("clearance", 0.0)
    _, _, all_q, ast = fik.solve(target_poses, with_base_link=with_base_link, **kw)
    centres = fcc.oracle_centres(all_q.astype(np.float32), with_base_link)
    radii = ft.collision_sphere_table(with_base_link)[1]
    hit, und = verdicts(centres, cloud, radii, point_radius, clearance, counts)
    q, status, bits = fold(all_q, ast, hit)
    return q, status, all_q, bits, und


def moved_winners(bits, status):
    """Problems with a result whose winner is not the lowest converged start."""
    first_conv = ((bits & fik.BIT_CONVERGED) != 0).argmax(1)
    winner = (bits == fik.BIT_CONVERGED).argmax(1)
    return int(((status == 0) & (winner != first_conv)).sum())
