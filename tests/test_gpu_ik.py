"""GPU: batched collision-free inverse kinematics (csrc/ik.hip, ``robot.franka_ik``) against its float64 restatement
(tests/float64_ik.py) and against the two kernels that already judge a configuration: ``FrankaCollisionSampler.check``
(mpx_franka_collision) and the ``self_collision`` output of mpx_trajectory_metrics.

Targets: right_gripper poses of ``scenes.random_configurations(B, seed)`` -- uniform in the empirical limits, so every
target is reachable."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_ik as f64  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402
from mpinets_amd import scenes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_FULL = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "problem_batch_default.npz")
POS_TOL, ROT_TOL = 1e-3, float(np.radians(0.5))
LIMITS = ft.JOINT_LIMITS_REAL  # float64, as passed to franka_ik: results are held to THESE, not to a float32 cast of them


def _robot():
    from mpinets_amd import robot

    return robot


def target_poses(B, seed=0):
    r = _robot()
    q = torch.from_numpy(scenes.random_configurations(B, seed)).to(DEV)
    return r.frames_to_matrix(r.franka_fk(q)[:, ft.LINK_ID["right_gripper"]]), q


def pose_errors(q, poses):
    """float64 position error and rotation angle of right_gripper(q) -- the frame mpx_franka_fk writes -- against poses."""
    r = _robot()
    fr = r.franka_fk(q.contiguous())[:, ft.LINK_ID["right_gripper"]].double().cpu()
    T = poses.double().cpu()
    _, theta = f64.rotvec(T[:, :3, :3], fr[:, :9].reshape(-1, 3, 3))
    return torch.linalg.norm(T[:, :3, 3] - fr[:, 9:], dim=-1).numpy(), theta.numpy()


def assert_reaches(q, poses, what):
    perr, theta = pose_errors(q, poses)
    print(f"{what}: {len(perr)} rows, max position error {perr.max(initial=0):.3e} m, max angle {theta.max(initial=0):.3e} rad")
    assert (perr <= POS_TOL).all() and (theta <= ROT_TOL).all(), what
    qn = q.double().cpu().numpy()
    on_limit = int(((np.abs(qn - LIMITS[:, 0]) < 1e-6) | (np.abs(qn - LIMITS[:, 1]) < 1e-6)).any(1).sum())
    print(f"{what}: {on_limit} rows have a joint on a limit")
    assert ((qn >= LIMITS[:, 0]) & (qn <= LIMITS[:, 1])).all(), f"{what}: outside the (float64) limits"


def prims_of(scn, lo=0, hi=None):
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    t = {k: torch.from_numpy(np.ascontiguousarray(v[lo:hi])).to(DEV) for k, v in scn.items()}
    cub = TorchCuboids(t["cuboid_centers"], t["cuboid_dims"], t["cuboid_quats"])
    cyl = TorchCylinders(t["cylinder_centers"], t["cylinder_radii"], t["cylinder_heights"], t["cylinder_quats"])
    return cub, cyl


def scene_prims(B, seed=0):
    scn = scenes.make_scenes(B, seed, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16)
    return (scn,) + prims_of(scn)


def judges(q, poses, cub, cyl):
    """-> (environment collision, self collision) bool [B] by the kernels that predate the IK; q rows must be finite."""
    from mpinets_amd.metrics import BatchedEvaluator
    from mpinets_amd.robot import FrankaCollisionSampler

    env = FrankaCollisionSampler(DEV).check(q.contiguous(), cub, cyl)
    res = BatchedEvaluator(DEV).evaluate_trajectories(q[:, None].contiguous(), poses)
    return env.cpu().numpy(), res["self_collision"].cpu().numpy()


@pytest.fixture(scope="module")
def free_space():
    poses, _ = target_poses(B_FULL)
    q, st, aq, ast = _robot().franka_ik(poses, return_all=True)
    torch.cuda.synchronize()
    return poses, q, st, aq, ast


def test_round_trip_every_solved_row_and_every_converged_seed(free_space):
    poses, q, st, aq, ast = free_space
    ok = st == 0
    assert torch.isnan(q[~ok]).all() and torch.isfinite(q[ok]).all()
    assert_reaches(q[ok], poses[ok], "status-0 rows")
    conv = (ast & 1) != 0
    assert_reaches(aq[conv], poses[:, None].expand(-1, 64, -1, -1)[conv], "converged seeds")
    # the result is the lowest converged seed (free space: nothing else to test), and without return_all it is the same
    first = conv.int().argmax(1)
    assert torch.equal(q[ok], aq[torch.arange(B_FULL, device=DEV), first][ok])
    q2, st2 = _robot().franka_ik(poses)
    assert torch.equal(st2, st) and torch.equal(q2[ok], q[ok])


@pytest.mark.parametrize("B", [0, 1, 65])
def test_round_trip_batch_edges(B):
    poses, _ = target_poses(B, seed=3)
    q, st, aq, ast = _robot().franka_ik(poses, return_all=True)
    assert q.shape == (B, 7) and st.shape == (B,) and aq.shape == (B, 64, 7) and ast.shape == (B, 64)
    ok = st == 0
    assert_reaches(q[ok], poses[ok], f"B = {B}")
    assert int(ok.sum()) >= B - 1  # (0.99 of 65 leaves room for no more than one)


def test_solved_share_in_free_space(free_space):
    """64 seeds x 64 iterations on 4096 reachable targets: the share of status 0 is at least the float64 restatement's
    share on the same targets minus 0.005 (20 problems: float32 / float64 seeds that end on the other side of a
    tolerance), and at least 0.99 in any case.  The restatement's own share (tests/test_ik_host.py) is 0.9995 (4094 of 4096)."""
    poses, q, st, aq, ast = free_space
    share = float((st == 0).float().mean())
    _, st64, _, ast64 = f64.solve(poses.cpu().numpy())
    share64 = float((st64 == 0).mean())
    per_seed, per_seed64 = float(((ast & 1) != 0).float().mean()), float((ast64 & 1).mean())
    print(f"share solved: device {share:.4f}, float64 restatement {share64:.4f}; converged seeds: {per_seed:.4f} / {per_seed64:.4f}")
    assert share >= share64 - 0.005
    assert share >= 0.99


def test_one_step_against_float64():
    """One iteration from a given start (lane 0), 4096 starts, against the float64 restatement's step from the same
    float32 numbers.  Bar: 4x the largest difference between the restatement run in float32 and in float64 on these
    very inputs (reference against reference, measured on the CPU and repeated by
    tests/test_ik_host.py::test_one_step_bars_can_be_derived_again): 5.37e-4 rad -> bar 2.15e-3 rad (the median of
    that difference is 5.9e-7: the largest values sit at starts close to singular, where J J^T + lambda^2 I has a
    condition number of ~1e3).  Starts whose Jacobian's smallest singular value (float64) is below 1e-3 are left out:
    5 of 4096 here; the cap on what may be left out is 1 %."""
    bar = 4 * 5.37e-4
    poses, _ = target_poses(B_FULL)
    q0 = torch.from_numpy(scenes.random_configurations(B_FULL, 1)).to(DEV)
    _, _, aq, _ = _robot().franka_ik(poses, q_init=q0, return_all=True, iterations=1)
    got = aq[:, 0].double().cpu()
    T = poses.double().cpu()
    lim = torch.from_numpy(f64.limits32(LIMITS)).double()
    want = f64.step(q0.double().cpu(), T[:, :3, :3], T[:, :3, 3], lim[:, 0], lim[:, 1])
    J, _, _ = f64.jacobian(q0.double().cpu())
    keep = torch.linalg.svdvals(J)[:, -1] >= 1e-3
    left_out = int((~keep).sum())
    diff = (got - want).abs().amax(1)
    print(f"one step: max |dq| difference {diff[keep].max():.3e} (all starts {diff.max():.3e}, median {diff.median():.3e}), "
          f"bar {bar:.3e}, left out {left_out} of {B_FULL}")
    assert left_out <= B_FULL // 100
    assert float(diff[keep].max()) <= bar


def test_one_step_on_every_lane_pins_the_philox_starts():
    """One iteration, no q_init, all 64 lanes of 64 problems at env_offset 1000: ``all_q`` against the float64 step from
    ``float64_ik.starts`` -- the restatement's Philox draws (counter (2 lane + k, env_offset + row, stream 13, 0), key =
    seed) mapped into the inward-rounded limits.  A kernel that drew from another counter layout, stream or problem id
    would be off by radians.  Bar as in the test above: 4x the float32-vs-float64 difference of the restatement on
    these 4096 starts, 3.55e-5 rad -> 1.42e-4 rad (tests/test_ik_host.py repeats the measurement); 6 starts are near
    singular and left out, cap 1 %."""
    bar = 4 * 3.55e-5
    B, off, seed = 64, 1000, 5
    poses, _ = target_poses(B, seed=17)
    _, _, aq, _ = _robot().franka_ik(poses, return_all=True, iterations=1, seed=seed, env_offset=off)
    got = aq.double().cpu().reshape(-1, 7)
    q0 = torch.from_numpy(f64.starts(B, LIMITS, seed=seed, env_offset=off)).double().reshape(-1, 7)
    T = poses.double().cpu()[:, None].expand(-1, 64, -1, -1).reshape(-1, 4, 4)
    lim = torch.from_numpy(f64.limits32(LIMITS)).double()
    want = f64.step(q0, T[:, :3, :3], T[:, :3, 3], lim[:, 0], lim[:, 1])
    J, _, _ = f64.jacobian(q0)
    keep = torch.linalg.svdvals(J)[:, -1] >= 1e-3
    left_out = int((~keep).sum())
    diff = (got - want).abs().amax(1)
    print(f"one step, every lane: max |dq| difference {diff[keep].max():.3e} (all starts {diff.max():.3e}, median "
          f"{diff.median():.3e}), bar {bar:.3e}, left out {left_out} of {len(diff)}")
    assert left_out <= len(diff) // 100
    assert float(diff[keep].max()) <= bar


@pytest.fixture(scope="module")
def in_scenes():
    poses, _ = target_poses(B_FULL)
    scn, cub, cyl = scene_prims(B_FULL)
    out = _robot().franka_ik(poses, cub, cyl, return_all=True)
    torch.cuda.synchronize()
    return (poses, scn, cub, cyl) + tuple(out)


def test_collision_free_is_what_the_existing_kernels_say(in_scenes):
    poses, scn, cub, cyl, q, st, aq, ast = in_scenes
    counts = [int((st == k).sum()) for k in range(3)]
    print(f"scenes (tabletop / cubby / dresser): status 0 / 1 / 2 = {counts}")
    assert counts[0] > 0 and counts[1] > 0  # (both branches below see rows)
    ok = st == 0
    assert torch.isnan(q[~ok]).all()
    assert_reaches(q[ok], poses[ok], "status-0 rows in scenes")
    probe = torch.where(ok[:, None], q, torch.zeros_like(q))
    env, self_ = judges(probe, poses, cub, cyl)
    okn = ok.cpu().numpy()
    assert not env[okn].any(), "mpx_franka_collision flags a returned configuration"
    assert not self_[okn].any(), "mpx_trajectory_metrics flags a returned configuration as self-colliding"
    # the choice is the defined one: the lowest seed whose bits say converged and free, bit for bit
    free = ast == 1
    first = free.int().argmax(1)
    assert torch.equal(free.any(1), ok)
    assert torch.equal(q[ok], aq[torch.arange(B_FULL, device=DEV), first][ok])
    # status 1: every converged seed is flagged by one of the two judges (seed by seed, over all 64 lanes)
    blocked = (st == 1).cpu().numpy()
    conv = ((ast & 1) != 0).cpu().numpy()
    assert conv[blocked].any(1).all() and not conv[(st == 2).cpu().numpy()].any()
    for lane in range(64):
        rows = blocked & conv[:, lane]
        if not rows.any():
            continue
        env, self_ = judges(aq[:, lane], poses, cub, cyl)
        assert (env | self_)[rows].all(), f"seed {lane}: a converged seed of a status-1 row is free by both judges"
        bits = ast[:, lane].cpu().numpy()
        assert (((bits & 2) != 0) == env)[rows].all() and (((bits & 4) != 0) == self_)[rows].all()
    # stopping at the first free candidate (no all_status) returns the same rows
    q2, st2 = _robot().franka_ik(poses, cub, cyl)
    assert torch.equal(st2, st) and torch.equal(q2[ok], q[ok])


def test_seed_zero_right_but_blocked():
    """q_init = the configuration that generated the target, a 10 cm cuboid on that configuration's link-4 sphere
    centre: seed 0 converges at once and collides.  The row returned differs from q_init, reaches the pose and is
    free -- or the status is 1.  Floor: status 0 in at least half of the 256 problems; the float64 restatement
    solves 0.891 of them, and so does the device (printed below)."""
    from mpinets_amd.geometry import TorchCuboids
    from mpinets_amd.robot import FrankaCollisionSampler

    B = 256
    poses, q_gen = target_poses(B, seed=5)
    coll = FrankaCollisionSampler(DEV)
    s4 = int(np.nonzero(coll.links.cpu().numpy() == ft.LINK_ID["panda_link4"])[0][0])
    centre = coll.sphere_centers(q_gen)[:, s4]
    centers = centre[:, None, :].contiguous()
    dims = torch.full((B, 1, 3), 0.1, device=DEV)
    quats = torch.tensor([1.0, 0, 0, 0], device=DEV).expand(B, 1, 4).contiguous()
    cub = TorchCuboids(centers, dims, quats)
    q, st, aq, ast = _robot().franka_ik(poses, cub, None, q_init=q_gen, return_all=True, check_self=False)
    assert ((ast[:, 0] & 3) == 3).all(), "seed 0 (the generating configuration) must converge and hit the cuboid"
    assert int((st == 2).sum()) == 0
    ok = st == 0
    assert_reaches(q[ok], poses[ok], "blocked seed 0")
    assert not coll.check(torch.where(ok[:, None], q, q_gen + 10.0).contiguous(), cub, None)[ok].any()
    assert ((q[ok] - q_gen[ok]).abs().amax(1) > 0).all()
    scene = {"cuboid_centers": centers.cpu().numpy(), "cuboid_dims": dims.cpu().numpy(), "cuboid_quats": quats.cpu().numpy(),
             "cylinder_centers": np.zeros((B, 1, 3), np.float32), "cylinder_radii": np.zeros((B, 1, 1), np.float32),
             "cylinder_heights": np.zeros((B, 1, 1), np.float32),
             "cylinder_quats": np.tile(np.array([1, 0, 0, 0], np.float32), (B, 1, 1))}
    _, st64, _, _ = f64.solve(poses.cpu().numpy(), q_init=q_gen.cpu().numpy(), scene=scene, check_self=False)
    share, share64 = float(ok.float().mean()), float((st64 == 0).mean())
    print(f"seed 0 blocked: status 0 in {share:.3f} of {B} (float64 restatement {share64:.3f})")
    assert share64 >= 0.5
    assert share >= 0.5


def test_unreachable_targets_and_guard_rows():
    B = 130
    poses, _ = target_poses(B, seed=9)
    poses = poses.clone()
    poses[:, :3, 3] = torch.nn.functional.normalize(poses[:, :3, 3], dim=1) * 2.0  # 2 m from the base
    r = _robot()
    from mpinets_amd import _lib

    lim = torch.from_numpy(ft.limits_float32_inward(LIMITS)).to(DEV)
    G = 8
    qbuf = torch.full((B + 2 * G, 7), 7.25, device=DEV)
    sbuf = torch.full((B + 2 * G,), -77, dtype=torch.int32, device=DEV)
    abuf = torch.full((B + 2 * G, 64, 7), 7.25, device=DEV)
    bbuf = torch.full((B + 2 * G, 64), -77, dtype=torch.int32, device=DEV)
    _lib.call("mpx_franka_ik", _lib.ptr(poses), B, ft.FINGER_OPENING, _lib.ptr(lim), None, None, None, None, 0, None, None, 0,
              None, None, None, 0, None, 0, 0, _lib.ptr(qbuf[G:]), _lib.ptr(sbuf[G:]), _lib.ptr(abuf[G:]), _lib.ptr(bbuf[G:]))
    torch.cuda.synchronize()
    assert (sbuf[G:G + B] == 2).all() and torch.isnan(qbuf[G:G + B]).all()
    assert (bbuf[G:G + B] == 0).all() and torch.isfinite(abuf[G:G + B]).all()
    for buf, fill in ((qbuf, 7.25), (sbuf, -77), (abuf, 7.25), (bbuf, -77)):
        assert (buf[:G] == fill).all() and (buf[G + B:] == fill).all(), "a guard row was written"
    q, st = r.franka_ik(poses)
    assert (st == 2).all() and torch.isnan(q).all()


def test_determinism_and_sharding():
    B, cut = 1040, 515
    poses, _ = target_poses(B, seed=11)
    scn, cub, cyl = scene_prims(B, seed=11)
    r = _robot()
    a = r.franka_ik(poses, cub, cyl, seed=21, return_all=True)
    b = r.franka_ik(poses, cub, cyl, seed=21, return_all=True)
    for x, y in zip(a, b):
        assert torch.equal(torch.nan_to_num(x.float(), nan=-9.0), torch.nan_to_num(y.float(), nan=-9.0))
    for lo, hi in ((0, cut), (cut, B)):
        cu, cy = prims_of(scn, lo, hi)
        part = r.franka_ik(poses[lo:hi].contiguous(), cu, cy, seed=21, env_offset=lo, return_all=True)
        for x, y in zip(a, part):
            assert torch.equal(torch.nan_to_num(x[lo:hi].float(), nan=-9.0), torch.nan_to_num(y.float(), nan=-9.0)), (lo, hi)
    other = r.franka_ik(poses, cub, cyl, seed=22, return_all=True)
    assert not torch.equal(a[2][:, 1:], other[2][:, 1:])  # another seed: other starts


def test_make_problem_batch_default_is_unchanged():
    """Defaults are bit-equal to the function's output before ``collision_free`` existed (tests/golden/problem_batch_default.md)."""
    want = dict(np.load(GOLDEN, allow_pickle=False))
    got = scenes.make_problem_batch(8, seed=0, device=DEV)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else np.asarray(got[k])
        assert g.dtype == v.dtype and g.shape == v.shape, k
        assert g.tobytes() == v.tobytes(), f"make_problem_batch()[{k!r}] changed"


def test_make_problem_batch_collision_free():
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    B = 96
    kinds = ("tabletop", "cubby", "dresser")
    prob = scenes.make_problem_batch(B, seed=2, device=DEV, kinds=kinds, M1=40, collision_free=True)
    base = scenes.make_problem_batch(B, seed=2, device=DEV, kinds=kinds, M1=40)
    once = scenes.make_problem_batch(B, seed=2, device=DEV, kinds=kinds, M1=40, collision_free=True, max_redraws=0)
    valid, valid_once = prob["valid"], once["valid"]
    print(f"collision_free=True: {int(valid.sum())} of {B} problems valid, {int(valid_once.sum())} without redraws")
    assert valid.dtype == torch.bool
    # floor: a call solves 0.878 of uniformly drawn poses in these scenes (3597 of 4096, the test above), so start AND goal
    # succeed in ~0.77 of the attempts; without redraws that is 74 of 96 (floor: 3 standard deviations below, 61), and five
    # attempts leave 0.23^5 = 0.06 % invalid, i.e. none or one of 96 (floor 94)
    assert int(valid_once.sum()) >= 61
    assert int(valid.sum()) >= 94
    # the redraws add problems and touch no problem that was valid at once
    assert int(valid.sum()) > int(valid_once.sum()) and bool(valid[valid_once].all())
    for k in ("q", "q_goal", "target_pose"):
        assert torch.equal(prob[k][valid_once], once[k][valid_once]), k
    redrawn = valid & ~valid_once
    assert not torch.equal(prob["target_pose"][redrawn], base["target_pose"][redrawn])
    assert torch.isnan(once["q_goal"][~valid_once]).all() and torch.isfinite(prob["q_goal"][valid]).all()
    assert torch.equal(once["q"][~valid_once], base["q"][~valid_once])  # invalid rows keep their first draws
    cub = TorchCuboids(prob["cuboid_centers"], prob["cuboid_dims"], prob["cuboid_quats"])
    cyl = TorchCylinders(prob["cylinder_centers"], prob["cylinder_radii"], prob["cylinder_heights"], prob["cylinder_quats"])
    vn = valid.cpu().numpy()
    for key in ("q", "q_goal"):
        env, self_ = judges(torch.where(valid[:, None], prob[key], prob["q"]), prob["target_pose"], cub, cyl)
        assert not env[vn].any() and not self_[vn].any(), key
    assert_reaches(prob["q_goal"][valid], prob["target_pose"][valid], "q_goal")
    # the scenes are those of the default path, and the slab's robot rows are the start's cloud
    for k in ("cuboid_centers", "cuboid_dims", "cylinder_radii"):
        assert torch.equal(prob[k], base[k])
    sub = scenes.make_problem_batch(40, seed=2, device=DEV, kinds=kinds, M1=40, collision_free=True, env_offset=30,
                                    total_envs=B)
    for k in ("q", "q_goal", "target_pose", "valid"):
        assert torch.equal(torch.nan_to_num(sub[k].float(), nan=-9.0), torch.nan_to_num(prob[k][30:70].float(), nan=-9.0)), \
            f"shard rows differ: {k}"


def test_single_pose_classmethods():
    """``ik`` / ``collision_free_ik`` over 48 poses per class: what they return satisfies the class's own
    ``within_limits`` (float64 limits) and reaches the pose; ``collision_free_ik`` filters self collisions with or
    without primitives."""
    from mpinets_amd.metrics import BatchedEvaluator
    from mpinets_amd.robot import FrankaRealRobot, FrankaRobot

    n = 48
    poses, _ = target_poses(n, seed=13)
    for cls in (FrankaRealRobot, FrankaRobot):
        solved = on_limit = 0
        for i in range(n):
            q = cls.ik(poses[i].cpu().numpy(), device=DEV)
            if q is None:
                continue
            solved += 1
            assert q.shape == (7,) and q.dtype == np.float64 and cls.within_limits(q), (cls.__name__, i, q)
            on_limit += int(((q == cls.JOINT_LIMITS[:, 0]) | (q == cls.JOINT_LIMITS[:, 1])
                             | (np.abs(q - cls.JOINT_LIMITS[:, 0]) < 1e-6) | (np.abs(q - cls.JOINT_LIMITS[:, 1]) < 1e-6)).any())
            perr, theta = pose_errors(torch.from_numpy(q).float().to(DEV)[None], poses[i:i + 1])
            assert perr[0] <= POS_TOL and theta[0] <= ROT_TOL
        print(f"{cls.__name__}.ik: {solved} of {n} solved, {on_limit} with a joint on a limit")
        assert solved >= n - 1  # (0.99 of 48)
    far = np.eye(4)
    far[:3, 3] = [2.0, 0.0, 0.5]
    assert FrankaRealRobot.ik(far, device=DEV) is None
    # free space: collision_free_ik still rejects self collisions (check_self on by default), ik does not look
    ev = BatchedEvaluator(DEV)
    differ = 0
    for i in range(n):
        q = FrankaRealRobot.collision_free_ik(poses[i].cpu().numpy(), device=DEV)
        if q is None:
            continue
        qt = torch.from_numpy(q).float().to(DEV)[None]
        assert FrankaRealRobot.within_limits(q)
        assert not bool(ev.evaluate_trajectories(qt[:, None].contiguous(), poses[i:i + 1])["self_collision"][0])
        plain = FrankaRealRobot.ik(poses[i].cpu().numpy(), device=DEV)
        differ += int(plain is None or not np.array_equal(plain, q))
    print(f"collision_free_ik in free space: {differ} of {n} results differ from ik's (a self-colliding first solution)")
