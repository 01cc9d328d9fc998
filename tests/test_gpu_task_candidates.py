"""``mpx_task_candidates`` (csrc/task_candidates.hip, ``solvers.task_candidates``) on the GPU against its float64 restatement
(tests/float64_task_candidates.py), and ``make_problem_batch(problems="task")`` end to end.

The batch is the host test's (``float64_task_candidates.problem_batch``): B = 5 at ``env_offset`` = 3 -- tabletop, cubby,
dresser, a roofed table on which few draws are free, a cubby with one pocket excluded -- M1 = M2 = 16, S = 8 with padding;
N in {1, 64, 100} (one lane, exactly one wave, a part-filled second wave), C in {1, 8}, both roles.  Twelve launches of five
workgroups; the restatement of all of them takes about a second.

A float32 device may decide a draw that lies within ``BAND`` of a decision boundary the other way.  Poses are compared on
the draws outside the band; kept lists on the problems with no banded draw up to their last kept one, which the host test
holds to at least 90 % of all (tests/test_task_candidates_host.py fixes the seed by that).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_task_candidates as ftc  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_plan import dev, prims_of  # noqa: E402
from test_task_candidates_host import BAND, CLEAN_SHARE, CONFIGS, DRAW_SEED, POS_TOL, ROT_TOL, SCENE_SEED  # noqa: E402

pytestmark = pytest.mark.gpu


def _call(boxes, kinds, cub, cyl, exclude, env_offset, N, C, role, seed=DRAW_SEED):
    from mpinets_amd import solvers

    ex = None if exclude is None else torch.from_numpy(exclude).to(dev())
    out = solvers.task_candidates(torch.from_numpy(boxes).to(dev()), torch.from_numpy(kinds).to(dev()), cub, cyl, C=C, seed=seed,
                                  env_offset=env_offset, role=role, exclude=ex, draws=N)
    return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope="module")
def batch():
    scn, boxes, kinds, exclude = ftc.problem_batch(SCENE_SEED)
    cub, cyl = prims_of(scn)
    return scn, boxes, kinds, exclude, cub, cyl


@pytest.fixture(scope="module")
def runs(batch):
    """(N, C, role) -> (the device's outputs, the restatement's dict per problem): every launch once."""
    scn, boxes, kinds, exclude, cub, cyl = batch
    return {(N, C, role): (_call(boxes, kinds, cub, cyl, exclude, ftc.TEST_ENV_OFFSET, N, C, role),
                           ftc.restate_batch(scn, boxes, kinds, exclude, ftc.TEST_ENV_OFFSET, C, DRAW_SEED, role, draws=N))
            for N, C, role in CONFIGS}


def test_poses_match_float64_outside_the_band(runs):
    """Every kept candidate whose draw lies outside the band is the restatement's pose of that draw: positions within
    ``POS_TOL``, rotation entries within ``ROT_TOL`` (ten times the deviation measured on these shapes, see the host test)."""
    pos_dev, rot_dev, compared = 0.0, 0.0, 0
    for (N, C, role), ((poses, draw, support, count), ref) in runs.items():
        for b, r in enumerate(ref):
            for j in range(int(count[b])):
                n = int(draw[b, j])
                assert 0 <= n < N
                if r["margin"][n] < BAND:
                    continue
                d = np.abs(poses[b, j].astype(np.float64) - r["all_poses"][n])
                pos_dev, rot_dev, compared = max(pos_dev, d[:3, 3].max()), max(rot_dev, d[:3, :3].max()), compared + 1
                assert support[b, j] == r["pick"][n]
                assert (poses[b, j, 3] == [0, 0, 0, 1]).all()
    print(f"task candidates vs float64: {compared} poses, position deviation {pos_dev:.3e} m, rotation entries {rot_dev:.3e}")
    assert compared >= 100
    assert pos_dev <= POS_TOL and rot_dev <= ROT_TOL


def test_kept_lists_equal_float64_on_clean_problems(runs):
    """``draw``, ``support`` and ``count`` are the restatement's, exactly, wherever no draw up to the last kept one is banded;
    at least ``CLEAN_SHARE`` of the problems are of that kind."""
    clean = total = 0
    for (N, C, role), ((poses, draw, support, count), ref) in runs.items():
        for b, r in enumerate(ref):
            total += 1
            if not ftc.clean(r, BAND):
                continue
            clean += 1
            assert count[b] == r["count"], (N, C, role, b)
            assert (draw[b] == r["draw"]).all() and (support[b] == r["support"]).all(), (N, C, role, b)
    print(f"task candidates: {clean} of {total} problems without a banded draw")
    assert clean >= CLEAN_SHARE * total


def test_order_tail_and_exclusion(runs):
    """``draw`` ascends strictly over the kept rows; rows past ``count`` hold NaN poses and -1; the roofed table keeps fewer
    than C at N = 100; the excluded pocket of problem 4 is never drawn from; the two roles draw different poses."""
    for (N, C, role), ((poses, draw, support, count), ref) in runs.items():
        for b in range(len(count)):
            k = int(count[b])
            assert 0 <= k <= min(C, N)
            assert (np.diff(draw[b, :k]) > 0).all() and (draw[b, :k] >= 0).all() and (support[b, :k] >= 0).all()
            assert np.isnan(poses[b, k:]).all() and (draw[b, k:] == -1).all() and (support[b, k:] == -1).all()
            assert np.isfinite(poses[b, :k]).all()
        assert (support[4] != 1).all()
    (poses, draw, support, count), ref = runs[(100, 8, 0)]
    assert 0 < ref[3]["count"] < 8 and count[3] == ref[3]["count"]  # (the NaN / -1 tail behind a kept row)
    assert not np.array_equal(runs[(100, 8, 0)][0][0][0], runs[(100, 8, 1)][0][0][0])


def test_rows_depend_on_the_global_id_alone(batch, runs):
    """Row b of a call at ``env_offset`` = o is row 0 of a call at o + b on that problem alone, and a second call gives the
    same bits."""
    scn, boxes, kinds, exclude, cub, cyl = batch
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    first = runs[(100, 8, 1)][0]
    again = _call(boxes, kinds, cub, cyl, exclude, ftc.TEST_ENV_OFFSET, 100, 8, 1)
    for a, c in zip(first, again):
        assert np.array_equal(a, c, equal_nan=True)
    for b in (1, 4):
        one = _call(boxes[b:b + 1], kinds[b:b + 1], TorchCuboids(cub.centers[b:b + 1], cub.dims[b:b + 1], cub.quats[b:b + 1]),
                    TorchCylinders(cyl.centers[b:b + 1], cyl.radii[b:b + 1], cyl.heights[b:b + 1], cyl.quats[b:b + 1]),
                    exclude[b:b + 1], ftc.TEST_ENV_OFFSET + b, 100, 8, 1)
        for a, c in zip(first, one):
            assert np.array_equal(a[b], c[0], equal_nan=True)


def test_without_primitives_only_the_self_test_rejects():
    """M1 = M2 = 0: a surface over the robot's base, where the body column rejects draws, and an all-padding problem, which
    reports count 0."""
    boxes = np.zeros((2, ftc.TEST_S, 12), np.float32)
    boxes[..., 6] = 1.0
    boxes[0, 0] = [0.0, 0.0, 0.3, 0.7, 0.7, 0.05, 1, 0, 0, 0, 0.0, 1.0]
    kinds = np.zeros((2, ftc.TEST_S), np.int32)
    kinds[0, 0] = ftc.SURFACE
    poses, draw, support, count = _call(boxes, kinds, None, None, None, ftc.TEST_ENV_OFFSET, 100, 8, 0)
    ref = ftc.restate_batch(None, boxes, kinds, None, ftc.TEST_ENV_OFFSET, 8, DRAW_SEED, 0, draws=100)
    assert 0 < (~ref[0]["free"]).sum() < 100  # (the self test rejects some draws, not all)
    assert ftc.clean(ref[0], BAND)
    assert count[0] == ref[0]["count"] and (draw[0] == ref[0]["draw"]).all() and (support[0] == ref[0]["support"]).all()
    assert np.abs(poses[0, :count[0]] - ref[0]["poses"][:count[0]]).max() <= max(POS_TOL, ROT_TOL)
    assert count[1] == 0 and np.isnan(poses[1]).all() and (draw[1] == -1).all() and (support[1] == -1).all()


def test_task_problems_end_to_end():
    """``make_problem_batch(problems="task")``: every valid row's start and goal are free by ``FrankaCollisionSampler``, their
    FK meets the chosen candidate poses within the IK's tolerances, tabletop goals sit 1 to 12 cm above a support or object
    top with the gripper pointing down, cubby goals lie inside ``target_volume`` and not in the start's pocket, and the
    expert still plans on these problems."""
    from mpinets_amd import robot, scenes, solvers
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    B, kinds = 8, ("tabletop", "cubby")
    prob = scenes.make_problem_batch(B, seed=0, kinds=kinds, collision_free=True, problems="task", expert=True)
    valid = prob["valid"].cpu().numpy()
    print(f"task problems: {int(valid.sum())} of {B} valid, {int(prob['expert_valid'].sum())} with an expert trajectory")
    assert valid.any()
    cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
    cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
    sampler = robot.FrankaCollisionSampler(dev())
    gripper = ft.LINK_ID["right_gripper"]
    v = prob["valid"]
    for q, pose in ((prob["q"], prob["start_pose"]), (prob["q_goal"], prob["target_pose"])):
        qv = torch.where(v[:, None], q, prob["q"])  # (an invalid row's goal is NaN: it is judged by nothing)
        assert not sampler.check(qv, cub, cyl)[v].any()
        fk = robot.frames_to_matrix(robot.franka_fk(qv)[:, gripper])[v].double().cpu().numpy()
        want = pose[v].double().cpu().numpy()
        assert np.linalg.norm(fk[:, :3, 3] - want[:, :3, 3], axis=-1).max() <= solvers.IK_DEFAULTS["pos_tol"] + 1e-6
        cos = (np.einsum("nij,nij->n", fk[:, :3, :3], want[:, :3, :3]) - 1) / 2
        assert np.arccos(np.clip(cos, -1, 1)).max() <= solvers.IK_DEFAULTS["rot_tol"] + 1e-5
    scn = {k: prob[k].cpu().numpy() for k in prob if k.startswith(("cuboid_", "cylinder_"))}
    goal, start = prob["target_pose"].double().cpu().numpy(), prob["start_pose"].double().cpu().numpy()
    volume = prob["target_volume"].double().cpu().numpy()
    support = prob["target_support"].cpu().numpy()
    for b in np.flatnonzero(valid):
        p = goal[b, :3, 3]
        if kinds[b % 2] == "tabletop":
            assert goal[b, 2, 2] < 0  # (the gripper's z axis points down)
            assert np.isnan(volume[b]).all()
            above = [p[2] - top for sdf, top in ftc.live_primitives(ftc.scene_row(scn, b))
                     if sdf(np.array([p[0], p[1], top])) <= ftc.SNAP + 1e-4]
            assert any(0.01 - 1e-4 <= g <= 0.12 + 1e-4 for g in above), (b, above)
        else:
            assert support[b] >= 0 and np.isfinite(volume[b]).all()
            assert ftc.cuboid_sdf(p, volume[b, :3], volume[b, 3:6], volume[b, 6:10]) <= 1e-5
            assert ftc.cuboid_sdf(start[b, :3, 3], volume[b, :3], volume[b, 3:6], volume[b, 6:10]) > 0
            negative = prob["target_negative_volumes"][b].cpu().numpy()
            assert np.isfinite(negative).all(-1).sum() == 3 and np.isnan(negative[support[b]]).all()
    ev = prob["expert_valid"]
    assert not (ev & ~v).any()
    assert torch.isfinite(prob["global_solutions"][ev]).all() and torch.isnan(prob["global_solutions"][~ev]).all()
