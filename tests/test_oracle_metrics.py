"""CPU: the oracle's trajectory metrics (row N3) vs vectors produced by RUNNING the reference's Evaluator methods
(tests/golden/gen_metrics_golden.py): final position / orientation error, joint-limit flag, end-effector path lengths,
SPARC smoothness of ragged trajectories."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_metrics as fm  # noqa: E402


def _targets(oracle, g):
    return oracle.frames_to_4x4(oracle.franka_fk(g["goals"])[:, oracle.RIGHT_GRIPPER_FRAME])


def test_trajectory_metrics_match_the_reference_evaluator(oracle, metrics_golden):
    from mpinets_amd import franka_tables as ft

    g = metrics_golden
    res = oracle.trajectory_metrics(g["traj"], g["lengths"], _targets(oracle, g), ft.JOINT_LIMITS_PUBLISHED)
    np.testing.assert_allclose(res["position_error"], g["m_position_error"], rtol=0, atol=2e-3)  # centimetres
    # degrees (the reference: float64 quaternions): the float32 bar against float64 + what the recorded results allow --
    # the bounds tests/test_gpu_metrics.py holds the kernel to; acos of the trace needed 6e-2 and 5e-2 here
    np.testing.assert_allclose(res["orientation_error"], g["m_orientation_error"], rtol=0,
                               atol=fm.BARS["traj_orientation_error"] + fm.GOLDEN_ATOL["orientation_error"])
    np.testing.assert_allclose(res["eff_position_path_length"], g["m_eff_position_path_length"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(res["eff_orientation_path_length"], g["m_eff_orientation_path_length"], rtol=0,
                               atol=fm.BARS["traj_eff_orientation_path_length"][50] + fm.GOLDEN_ATOL["eff_orientation_path_length"])
    np.testing.assert_array_equal(res["joint_limit_violation"], g["m_joint_limit_violation"].astype(bool))
    assert g["m_position_error"][6] < 1e-3 and g["m_eff_position_path_length"][4] == 0  # on target / never moved


def test_trajectory_smoothness_matches_the_reference_evaluator(oracle, metrics_golden):
    g = metrics_golden
    cs, es = oracle.trajectory_smoothness(g["traj"], g["lengths"], float(g["dt"]))
    ok = g["lengths"] >= 2
    np.testing.assert_allclose(cs[ok], g["m_config_smoothness"][ok], rtol=0, atol=1e-4)
    np.testing.assert_allclose(es[ok], g["m_eff_smoothness"][ok], rtol=0, atol=2e-3)
    assert g["m_config_smoothness"][4] == 0 and cs[4] == 0  # sparc's all-zero branch
