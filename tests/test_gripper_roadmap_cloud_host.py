"""CPU: ``mpx_gripper_roadmap_cloud`` refuses bad arguments on the host, before any launch; its kernel uses no scratch; the
Python entry and its two callers (``scenes.make_problem_batch(hybrid_guide="gripper_cloud")``,
``capture.plan_to_poses(follow_guide="gripper")``) take what the issue states and hand to C what they should; and the float64
restatement (tests/float64_gripper_roadmap_cloud.py), run as a planner on the wall and the cylinder drawn as clouds with Philox
draws, finds a path on at least 90 % of the rows.  The band of the GPU edge-state comparison, the cap of its left-out problems
and the band of "what the field promises" are derived here, at the seed the GPU tests use (chosen on the CPU, before any
device run).

Recorded at ROADMAP_SEED = 5, lattice pitch 0.02 m, point_radius 0.015 m, the default grid (voxel 0.03 m, 61 x 61 x 51 nodes,
trunc 0.185 m), float64, the default options (64 nodes, 256 rounds):
  wall      (1092 points): 64 of 64 found; hops 2 / 3 / 4: 17 / 45 / 2; rounds at most 213, mean 65.9; none out of rounds
  cylinder  ( 982 points): 64 of 64 found; hops 2 / 3: 37 / 27; rounds at most 50, mean 16.0; none out of rounds
(test_restatement_finds_a_way_round_the_clouds prints the full histograms of hops and rounds.)"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_field as fcf  # noqa: E402
import float64_cloud_plan as fcp  # noqa: E402
import float64_gripper_roadmap as fg  # noqa: E402
import float64_gripper_roadmap_cloud as fgc  # noqa: E402
import solver_call_grid as grid_calls  # noqa: E402
from test_gripper_roadmap_host import FOUND_SHARE, LEFT_OUT_CAP  # noqa: E402  (conditions, not measurements)

from mpinets_amd import _lib, capture, robot, scenes, solvers  # noqa: E402
from mpinets_amd.field import CloudField  # noqa: E402

# The largest float32-against-float64 difference of d = ((D - point_radius) - r_s) - clearance -- the placement of a sphere
# centre from a float32 pose, the trilinear sample there, the two subtractions -- over the unsaturated sphere samples of every
# tested pose (nodes and interior edge poses) of the restatement's own graphs on the two scenarios, the float32 side being the
# float32 restatement of the kernel's arithmetic.  Recorded by test_band_and_left_out_share.  Distances and radii are below
# 0.25 m, where a float32 ulp is 1.5e-8: the placement's three fmas (4.8e-8 m in tests/test_gripper_roadmap_host.py), the eight
# corner values, three fractions and seven lerps account for it.  Measured: 1.845e-7 m over 5.2 million samples.
BAND_REFERENCE = 1.8e-7
CLOUD_BAND = 4 * BAND_REFERENCE  # what a float32 verdict may differ by from the float64 one [m]
# "What the field promises" compares against the EXACT distance to the cloud, so what the field's nodal values lack counts
# too: the device's squared distance is within float64_cloud_field.BAND (4 x 2^-24, relative) of the float64 one, so a nodal
# value below trunc is within trunc x BAND / 2 of the distance, plus half an ulp of the rounded square root (2^-27 below 0.25).
TRUNC = fcp.truncation(fgc.POINT_RADIUS)
PROMISE_BAND = CLOUD_BAND + TRUNC * fcf.BAND / 2 + 2.0 ** -27
LIPSCHITZ = np.sqrt(3) / 2  # the trilinear interpolant of a 1-Lipschitz field is within this many voxels of it
CONSERVATIVE_SLACK = 0.866 * fcp.VOXEL

# ---- refusals ------------------------------------------------------------------------------------------------------------------
GOOD = dict(nodes=64, resolution=0.01, rot_weight=0.12, orient_spread=0.5, connect_radius=float("inf"), max_rounds=8,
            check_margin=1e-4, clearance=0.0, check_self=1)


def _grid(trunc=0.2, n=(8, 8, 8), h=0.05):
    return _lib.FieldGrid((ctypes.c_float * 3)(0.0, 0.0, 0.0), h, n[0], n[1], n[2], trunc)


def _p(v):  # any non-NULL "device pointer": refused before it is touched
    return ctypes.c_void_p(v) if v else None


def _call(lib, B=4, W=8, S=56, field=256, grid="good", point_radius=0.02, field_slack=0.0, opts=None, env_offset=0, poses=256,
          status=256, path=256, hops=256, sp=256, gp=256, bounds=256, table=256):
    g = _grid() if grid == "good" else grid
    return lib.mpx_gripper_roadmap_cloud(_p(sp), _p(gp), B, W, _p(bounds), 0.025, _p(table), _p(table), _p(table), S, _p(field),
                                         None if g is None else ctypes.byref(g), point_radius, field_slack,
                                         None if opts is None else ctypes.byref(opts), 0, env_offset, _p(poses), _p(status),
                                         _p(path), _p(hops), None, None, None, None)


def test_gripper_roadmap_cloud_refuses_bad_arguments_on_the_host():
    lib = _lib.load()
    opt = lambda **kw: _lib.GripperRoadmapOptions(**dict(GOOD, **kw))  # noqa: E731
    err = lib.mpx_last_error
    # what mpx_gripper_roadmap refuses
    for V in (-1, 0, 1, 257):
        assert _call(lib, opts=opt(nodes=V)) != 0 and b"nodes" in err()
    for W in (-1, 0, 65):
        assert _call(lib, W=W) != 0 and b"guide poses" in err()
    for res in (0.0, -0.01, float("nan")):
        assert _call(lib, opts=opt(resolution=res)) != 0 and b"resolution" in err()
    for rw in (0.0, -0.12, float("nan"), float("inf")):
        assert _call(lib, opts=opt(rot_weight=rw)) != 0 and b"rot_weight" in err()
    for spread in (-0.5, float("nan")):
        assert _call(lib, opts=opt(orient_spread=spread)) != 0 and b"orient_spread" in err()
    assert _call(lib, opts=opt(connect_radius=float("nan"))) != 0 and b"connect_radius" in err()
    assert _call(lib, opts=opt(max_rounds=0)) != 0 and b"max_rounds" in err()
    assert _call(lib, opts=opt(check_margin=-1e-4)) != 0 and b"check_margin" in err()
    assert _call(lib, opts=opt(clearance=float("nan"))) != 0 and b"clearance" in err()
    for out in ("poses", "status", "path", "hops"):
        assert _call(lib, **{out: 0}) != 0 and b"NULL output" in err()
    for operand in ("sp", "gp", "bounds"):
        assert _call(lib, **{operand: 0}) != 0 and b"NULL operand" in err()
    assert _call(lib, table=0) != 0 and b"sphere table" in err()
    assert _call(lib, B=-1) != 0 and b"negative size" in err()
    assert _call(lib, S=-1) != 0 and b"negative size" in err()
    assert _call(lib, S=65) != 0 and b"65" in err()
    for bad in (-1, 1 << 32):
        assert _call(lib, env_offset=bad) != 0 and b"env_offset" in err()
    assert _call(lib, B=1 << 25, W=64) != 0 and b"B x W x 16" in err()  # 2^25 x 64 x 16 = 2^35 entries
    # what the grid check refuses
    assert _call(lib, grid=None) != 0 and b"NULL grid" in err()
    assert _call(lib, grid=_grid(n=(1, 8, 8))) != 0 and b"nodes" in err()
    assert _call(lib, grid=_grid(h=0.0)) != 0 and b"spacing" in err()
    assert _call(lib, grid=_grid(trunc=float("inf"))) != 0 and b"trunc" in err()
    # what mpx_franka_roadmap_cloud refuses about the field
    for bad in (-0.01, float("nan"), float("inf")):
        assert _call(lib, field_slack=bad) != 0 and b"field_slack" in err()
        assert _call(lib, point_radius=bad) != 0 and b"point_radius" in err()
    assert _call(lib, S=0, table=0) != 0 and b"without collision spheres" in err()
    # trunc must exceed 0.08 + point_radius + max(clearance, 0) + check_margin + field_slack (the JOINT roadmap's bound,
    # although the gripper's largest sphere is smaller): 0.1001 here ...
    assert _call(lib, grid=_grid(trunc=0.1)) != 0 and b"trunc" in err()
    assert _call(lib, B=0, grid=_grid(trunc=0.1002)) == 0
    # ... 0.1261 with a slack of 0.866 x 3 cm, 0.1501 with a clearance of 5 cm (a negative clearance gives no room back)
    assert _call(lib, B=0, grid=_grid(trunc=0.126), field_slack=0.026) != 0 and b"trunc" in err()
    assert _call(lib, B=0, grid=_grid(trunc=0.1262), field_slack=0.026) == 0
    assert _call(lib, B=0, grid=_grid(trunc=0.15), opts=opt(clearance=0.05)) != 0 and b"trunc" in err()
    assert _call(lib, B=0, grid=_grid(trunc=0.1), opts=opt(clearance=-0.05)) != 0 and b"trunc" in err()
    assert b"mpx_gripper_roadmap_cloud" in err()
    assert fgc.refused(fcf.make_grid((8, 8, 8), trunc=0.1), 0.02, 0.0) and not fgc.refused(fcf.make_grid((8, 8, 8), trunc=0.1002), 0.02, 0.0)
    assert not fgc.refused(fgc.scenario_grid(), fgc.POINT_RADIUS, CONSERVATIVE_SLACK)  # (plan_cloud_truncation satisfies it)
    # nothing to do, nothing touched: without a field no grid is read and S may be 0; a bad option is refused even then
    assert _call(lib, B=0, poses=0, status=0, path=0, hops=0, sp=0, gp=0, bounds=0, table=0) == 0
    assert _call(lib, B=0, field=0, grid=None, S=0, table=0) == 0
    assert _call(lib, B=0, opts=opt(nodes=1)) != 0 and _call(lib, B=0, field_slack=-1.0) != 0


def test_python_entry_point_and_defaults():
    M = torch.eye(4).expand(2, 4, 4)
    with pytest.raises(_lib.MpxError):
        robot.gripper_roadmap_cloud(M, M, None)  # (CPU tensors)
    with pytest.raises(_lib.MpxError):
        robot.gripper_roadmap_cloud(M, M, torch.zeros(2, 5, 3))
    assert robot.gripper_roadmap_cloud is solvers.gripper_roadmap_cloud
    sig = inspect.signature(robot.gripper_roadmap_cloud).parameters
    assert list(sig)[:3] == ["start_pose", "goal_pose", "cloud"]
    want = dict(counts=None, field=None, point_radius=0.0, field_slack=0.0, W=8, bounds=None, seed=0, env_offset=0,
                return_graph=False, with_base_link=False, finger=robot.ft.FINGER_OPENING)
    assert {k: sig[k].default for k in want} == want and sig["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(sig)[3:-1] == list(want)
    with grid_calls.recording():
        with pytest.raises(TypeError):
            robot.gripper_roadmap_cloud(M, M, None, node=3)
    assert _lib.load().mpx_version() == 341
    for word in ("sqrt(3)/2", "graze", "check_cloud"):  # (what franka_roadmap_cloud's docstring says about the field)
        assert word in robot.gripper_roadmap_cloud.__doc__ and word in robot.franka_roadmap_cloud.__doc__


def test_what_the_wrapper_hands_to_c():
    """No cloud and no field: NULL field and grid; a cloud: one field build on the default grid with the truncation of
    ``plan_cloud_truncation(point_radius, clearance)``, then the entry with that field; a given field: no build."""
    B = 3
    M = torch.eye(4).repeat(B, 1, 1)
    cloud = torch.zeros(B, 9, 4)[:, 2:7, :3]
    with grid_calls.recording() as calls:
        out = robot.gripper_roadmap_cloud(M, M, None, W=5, seed=7, env_offset=2, nodes=16)
    assert [c[0] for c in calls] == ["mpx_gripper_roadmap_cloud"] and len(out) == 2
    a = calls[0][1]
    assert a[2] == B and a[3] == 5 and a[9] == 56 and a[10] is None and a[11] is None and a[12] == 0.0 and a[13] == 0.0
    assert a[14]._obj.nodes == 16 and a[15] == 7 and a[16] == 2 and a[21:24] == (None, None, None)
    assert out[0].shape == (B, 5, 4, 4) and out[1].shape == (B,)
    with grid_calls.recording() as calls:
        out = robot.gripper_roadmap_cloud(M, M, cloud, point_radius=0.01, field_slack=0.02, return_graph=True, clearance=0.03)
    assert [c[0] for c in calls] == ["mpx_cloud_field_build", "mpx_gripper_roadmap_cloud"] and len(out) == 7
    built, a = calls[0][1], calls[1][1]
    assert built[6]._obj.trunc == pytest.approx(robot.plan_cloud_truncation(0.01, 0.03, robot.FOLLOW_DEFAULTS["epsilon"]), rel=1e-6)
    assert a[10] == built[7] and a[11]._obj is built[6]._obj and a[12] == 0.01 and a[13] == 0.02
    assert a[14]._obj.clearance == pytest.approx(0.03) and None not in a[17:24]
    assert out[4].shape == (B, 64, 7) and out[5].shape == (B, 64, 64) and out[5].dtype == torch.uint8
    with grid_calls.recording():
        field = CloudField.build(cloud)
    with grid_calls.recording() as calls:
        robot.gripper_roadmap_cloud(M, M, None, field=field)
    assert [c[0] for c in calls] == ["mpx_gripper_roadmap_cloud"] and calls[0][1][10] == field.values.data_ptr()
    # the primitive entry's call is what it was (one helper now makes the bounds of both)
    with grid_calls.recording() as calls:
        robot.gripper_roadmap(M, M, W=5, seed=7, env_offset=2)
    assert [c[0] for c in calls] == ["mpx_gripper_roadmap"] and calls[0][1][2:4] == (B, 5)


def test_gripper_roadmap_cloud_kernel_metadata():
    """Exactly one kernel of that name; no scratch, no VGPR spills; LDS is dynamic (33 804 B at 256 nodes, 8192 B below the
    primitive kernel's: no primitive rows).  The figures are printed and recorded in profiles/gripper_roadmap_cloud_timing.md."""
    from test_code_objects import LIB, NO_SCRATCH_FIELDS, kernel_metadata

    hits = {n: f for n, f in kernel_metadata(LIB).items() if "gripper_roadmap_cloud_kernel" in n}
    assert len(hits) == 1
    (f,) = hits.values()
    print({k: f[k] for k in NO_SCRATCH_FIELDS + (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size")})
    assert int(f[".private_segment_fixed_size"]) == 0 and int(f[".vgpr_spill_count"]) == 0

    def lds(V, rows):  # the two layouts of the sources, in bytes
        return 4 * (rows + 64 * 4 + V * 7 + 2 * V + 6 * V + V + 1 + 1 + 1 + (V * V + 15) // 16)
    assert lds(256, 0) == 33804 and lds(256, 128 * 16) - lds(256, 0) == 8192 and lds(64, 0) == 6156


def test_make_problem_batch_takes_the_gripper_cloud_guide_only_against_the_cloud():
    kw = dict(device="cpu", collision_free=True, expert=True, hybrid=True)
    sig = inspect.signature(scenes.make_problem_batch).parameters
    assert sig["hybrid_guide"].default == "global" and sig["hybrid_against"].default == "primitives"
    assert sig["hybrid"].default is False and sig["expert_from"].default == "primitives"
    with pytest.raises(ValueError, match="gripper_cloud.*needs hybrid_against='cloud'"):
        scenes.make_problem_batch(1, hybrid_guide="gripper_cloud", **kw)
    with pytest.raises(ValueError, match="gripper_cloud.*needs hybrid_against='cloud'"):
        scenes.make_problem_batch(1, hybrid_guide="gripper_cloud", expert_from="roadmap", **kw)
    with pytest.raises(ValueError, match="hybrid_guide must be"):
        scenes.make_problem_batch(1, hybrid_guide="cloud", **kw)
    with pytest.raises(ValueError, match="gripper roadmap has no cloud form: use 'gripper_cloud'"):
        scenes.make_problem_batch(1, hybrid_against="cloud", expert_from="cloud", hybrid_guide="gripper", **kw)
    # the cloud follower's helper: one field build, the gripper roadmap and the follower read it; seed and env_offset key the draw
    B = 2
    q0, q1, valid = torch.zeros(B, 7), torch.full((B, 7), 0.1), torch.ones(B, dtype=torch.bool)
    big, plan = torch.zeros(B, 5, 3), torch.zeros(B, scenes.EXPERT_LENGTH, 7)
    with grid_calls.recording() as calls:
        out = scenes._hybrid_trajectories_cloud(big, q0, plan, valid, 0.02, q1, 5, 2, gripper_guide=True)
    names = [c[0] for c in calls]
    assert [n for n in names if "fk" not in n] == ["mpx_cloud_field_build", "mpx_gripper_roadmap_cloud", "mpx_franka_follow_cloud"]
    build, rm, fol = (calls[names.index(n)][1] for n in ("mpx_cloud_field_build", "mpx_gripper_roadmap_cloud", "mpx_franka_follow_cloud"))
    assert rm[10] == build[7] == fol[11] and rm[12] == pytest.approx(0.02) and rm[13] == 0.0
    assert rm[3] == scenes.HYBRID_GUIDE_POSES and rm[15] == 5 and rm[16] == 2
    assert sorted(out) == ["hybrid_guide_poses", "hybrid_guide_status", "hybrid_solutions", "hybrid_target_pose", "hybrid_valid"]
    with grid_calls.recording() as calls:
        out = scenes._hybrid_trajectories_cloud(big, q0, plan, valid, 0.02)
    assert "mpx_gripper_roadmap_cloud" not in [c[0] for c in calls]
    assert sorted(out) == ["hybrid_solutions", "hybrid_target_pose", "hybrid_valid"]


def test_plan_to_poses_takes_the_gripper_guide_only_with_the_follower():
    sig = inspect.signature(capture.plan_to_poses).parameters
    assert sig["follow_guide"].default == "plan" and sig["follow_guide"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["gripper_options"].default is None and sig["gripper_options"].kind is inspect.Parameter.KEYWORD_ONLY
    B = 3
    q0, poses = torch.zeros(B, 7), torch.eye(4).repeat(B, 1, 1)
    cloud, counts = torch.zeros(B, 9, 4)[:, 2:7, :3], torch.full((B,), 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs follow=True"):
        capture.plan_to_poses(cloud, q0, poses, follow_guide="gripper")
    with pytest.raises(ValueError, match="follow_guide must be"):
        capture.plan_to_poses(cloud, q0, poses, follow=True, follow_guide="global")
    with grid_calls.recording() as calls:
        res = capture.plan_to_poses(cloud, q0, poses, counts=counts, T=grid_calls.T, seed=5, env_offset=2, follow=True,
                                    follow_poses=6, follow_guide="gripper", gripper_options=dict(nodes=16, field_slack=0.02))
    names = [c[0] for c in calls if "fk" not in c[0]]
    assert names == ["mpx_cloud_field_build", "mpx_franka_ik_cloud", "mpx_franka_plan_cloud", "mpx_gripper_roadmap_cloud",
                     "mpx_franka_follow_cloud"]
    by = {c[0]: c[1] for c in calls}
    rm = by["mpx_gripper_roadmap_cloud"]
    assert rm[10] == by["mpx_cloud_field_build"][7] == by["mpx_franka_follow_cloud"][11]  # ONE field
    assert rm[3] == 6 and rm[13] == pytest.approx(0.02) and rm[14]._obj.nodes == 16 and rm[15] == 5 and rm[16] == 2
    assert res["follow_guide_poses"].shape == (B, 6, 4, 4) and res["follow_guide_status"].shape == (B,)
    with grid_calls.recording():
        plain = capture.plan_to_poses(cloud, q0, poses, counts=counts, T=grid_calls.T, follow=True, follow_poses=6)
    assert sorted(res) == sorted(list(plain) + ["follow_guide_poses", "follow_guide_status"])


# ---- the restatement as a planner on the GPU tests' scenarios -------------------------------------------------------------------
@pytest.fixture(scope="module")
def planned():
    B = 64
    sp, gp = fg.problems(B)
    out = {}
    for kind in ("wall", "cylinder"):
        cloud, grid, field = fgc.scenario_field(kind)
        out[kind] = (cloud, grid, field, fgc.solve(sp, gp, field, grid, fgc.POINT_RADIUS, seed=fgc.ROADMAP_SEED))
    return sp, gp, out


def test_clouds_cover_their_obstacles():
    """Every point lies on its obstacle's surface, and no surface point is farther than ``POINT_RADIUS`` from the lattice
    (checked on a lattice four times as fine): pitch / sqrt(2) = 0.01414 m on a flat face."""
    assert fgc.PITCH / np.sqrt(2) < fgc.POINT_RADIUS and fgc.surface_cloud("free") is None
    assert fgc.scenario_grid()["h"] == np.float32(fcp.VOXEL) and float(fgc.scenario_grid()["trunc"]) == pytest.approx(TRUNC, rel=1e-6)
    c, half = np.float64(fg.WALL_CENTRE), np.float64(fg.WALL_DIMS) / 2
    wall = fgc.surface_cloud("wall").astype(np.float64) - c
    assert (np.abs(wall) <= half + 1e-6).all() and (np.abs(np.abs(wall) - half) < 1e-6).any(-1).all()
    cyl = fgc.surface_cloud("cylinder").astype(np.float64) - c
    rho, hh = np.hypot(cyl[:, 0], cyl[:, 1]), fg.CYLINDER_HEIGHT / 2
    assert ((np.abs(rho - fg.CYLINDER_RADIUS) < 1e-6) | ((np.abs(np.abs(cyl[:, 2]) - hh) < 1e-6) & (rho < fg.CYLINDER_RADIUS))).all()
    for kind, coarse in (("wall", wall), ("cylinder", cyl)):
        fine = fgc.surface_cloud(kind, fgc.PITCH / 4).astype(np.float64) - c
        gap = fcf.nearest_distance(coarse, fine).max()
        print(f"{kind}: {len(coarse)} points, largest gap from the surface to a point {gap:.4f} m")
        assert gap <= fgc.POINT_RADIUS


def test_restatement_finds_a_way_round_the_clouds(planned):
    """Float64, the default options, Philox draws at ROADMAP_SEED: a path on at least FOUND_SHARE of the rows, each with at
    least 2 hops (the obstacle sits between every start and its goal); status-0 guide poses are valid by the restatement's
    own rule; the path costs what Dijkstra says on its own graph.  The module docstring records the figures."""
    sp, gp, out = planned
    for kind, (cloud, grid, field, (poses, st, path, hops, nodes, es, rounds)) in out.items():
        found = st == 0
        print(f"{kind}: status 0 / 1 / 2 {np.bincount(st, minlength=3).tolist()}, hops histogram {np.bincount(hops[found]).tolist()}, "
              f"rounds max {rounds.max()} mean {rounds.mean():.1f}, out of rounds {int(((st == 1) & (rounds == 256)).sum())}, "
              f"rounds histogram (bins of 32) {np.bincount(rounds // 32).tolist()}")
        assert found.mean() >= FOUND_SHARE
        assert (hops[found] >= 2).all()
        assert np.isnan(poses[~found]).all() and (path[~found] == -1).all()
        assert np.array_equal(poses[found][:, -1, :3], gp[found][:, :3].astype(np.float64))
        assert np.array_equal(nodes, fg.draw_nodes(sp, gp, fg.default_bounds(sp, gp), 64, fgc.ROADMAP_SEED)[0])  # the primitive form's
        low = np.inf
        for b in np.flatnonzero(found):
            env, own = fgc.margins(fg.pose_nodes(poses[b].astype(np.float32)), field, grid, fgc.POINT_RADIUS)
            low = min(low, float(np.minimum(env, own).min()))
        print(f"{kind}: smallest margin of a guide pose {low:.3e} m")
        assert low > 0
        for b in np.flatnonzero(found)[:8]:
            p = path[b, :hops[b] + 1]
            assert fg.path_cost(nodes[b], p) == pytest.approx(fg.dijkstra_cost(nodes[b], es[b]), rel=1e-12)


def test_band_and_left_out_share(planned):
    """``CLOUD_BAND`` = 4 x the largest float32-against-float64 difference of d over every tested pose of the two scenarios
    (the measurement is repeated here and must land within a factor 2 of the recorded figure); the share of problems with a
    deciding pose inside that band stays below LEFT_OUT_CAP for the restatement alone, and its graph agrees with the
    verdicts recomputed from the float32 poses everywhere else."""
    sp, gp, out = planned
    worst, samples = 0.0, 0
    for kind, (cloud, grid, field, (poses, st, path, hops, nodes, es, rounds)) in out.items():
        left = wrong = 0
        for b in range(len(st)):
            want, in_band, tested = fgc.graph_verdicts(nodes[b], np.ones(nodes.shape[1], bool), es[b], field, grid, CLOUD_BAND,
                                                       point_radius=fgc.POINT_RADIUS)
            left += in_band
            t = want != 0
            wrong += (not in_band) and not np.array_equal(want[t], es[b][t])
            d64, l64 = fgc.margins(tested.astype(np.float64), field, grid, fgc.POINT_RADIUS, check_self=False, want_samples=True)[2:]
            d32, l32 = fgc.margins(tested, field, grid, fgc.POINT_RADIUS, check_self=False, dtype=np.float32, want_samples=True)[2:]
            both = l64 & l32
            samples += int(both.sum())
            if both.any():
                worst = max(worst, float(np.abs(d64 - d32)[both].max()))
        print(f"{kind}: {left} of {len(st)} left out ({left / len(st):.4f}), {wrong} disagree")
        assert left / len(st) <= LEFT_OUT_CAP and wrong == 0
    print(f"|d_float32 - d_float64| over {samples} unsaturated sphere samples of the tested poses: max {worst:.3e} m; "
          f"CLOUD_BAND {CLOUD_BAND:.3e} m, PROMISE_BAND {PROMISE_BAND:.3e} m")
    assert samples > 10000 and BAND_REFERENCE / 2 <= worst <= BAND_REFERENCE * 2


def promised_margin(poses, cloud, point_radius=fgc.POINT_RADIUS, clearance=0.0):
    """Guide poses [N,4,4] -> the smallest ``dist - point_radius - r_s - clearance`` over the gripper's spheres, dist the
    EXACT float64 distance from the sphere centre to the nearest point of ``cloud`` [n,3] (brute force or a k-d tree:
    ``float64_cloud_field.nearest_distance``)."""
    pts, radii, _, _ = fg.gripper_points()
    x = fg.place(fg.pose_nodes(np.asarray(poses, np.float64)), pts)
    dist = fcf.nearest_distance(cloud, x.reshape(-1, 3)).reshape(x.shape[:2])
    return float((dist - point_radius - radii[None] - clearance).min())


def test_what_the_field_promises_for_the_restatement(planned):
    """With ``field_slack = 0.866 x voxel`` every sphere of every guide pose of a found row is free by the exact distance to
    the cloud: margin > check_margin - PROMISE_BAND; with no slack the same margin is above -(sqrt(3)/2) voxel - PROMISE_BAND.
    (Distance is 1-Lipschitz, so the interpolant is within (sqrt(3)/2) h of it: sum w_i |c_i - x| <= sqrt(sum w_i |c_i - x|^2)
    = h sqrt(sum_axes f (1 - f)) <= (sqrt(3)/2) h.  The slack run is made on the first 16 rows.)"""
    sp, gp, out = planned
    for kind, (cloud, grid, field, run) in out.items():
        slack = fgc.solve(sp[:16], gp[:16], field, grid, fgc.POINT_RADIUS, CONSERVATIVE_SLACK, seed=fgc.ROADMAP_SEED)
        for name, (poses, st), floor in (("no slack", run[:2], -LIPSCHITZ * fcp.VOXEL - PROMISE_BAND),
                                         ("0.866 voxel", slack[:2], fg.DEFAULTS["check_margin"] - PROMISE_BAND)):
            found = st == 0
            assert found.any()
            low = min(promised_margin(poses[b], cloud) for b in np.flatnonzero(found))
            print(f"{kind}, {name}: {int(found.sum())} of {len(st)} rows found; smallest exact margin of a guide pose's sphere "
                  f"{low:.4e} m (floor {floor:.4e})")
            assert low > floor
