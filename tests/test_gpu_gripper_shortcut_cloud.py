"""GPU: ``mpx_gripper_shortcut_cloud`` (csrc/gripper_shortcut_cloud.hip), ``robot.gripper_plan_cloud`` and its two callers
(``make_problem_batch(..., hybrid_guide="gripper_cloud", hybrid_shortcut=True)``, ``capture.plan_to_poses(...,
follow_guide="gripper", follow_shortcut=True)``) against the restatement (tests/float64_gripper_shortcut.py with
tests/float64_gripper_roadmap_cloud.py's field rule), by the checks of tests/test_gpu_gripper_shortcut.py.  One module-scoped
fixture: the wall and the upright cylinder drawn as clouds, the field the DEVICE built (copied to the host, so these tests judge
the shortcut kernel and not the field build), the device's own gripper roadmap with its graph on the 64 problems at
ROADMAP_SEED, the polylines ``nodes[path]`` and the default shortcut with the trace."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_gripper_roadmap as fg  # noqa: E402
import float64_gripper_roadmap_cloud as fgc  # noqa: E402
import float64_gripper_shortcut as fgs  # noqa: E402
from mpinets_amd import franka_tables as ft  # noqa: E402
from test_gpu_cloud_plan import build_field, grid_dict  # noqa: E402
from test_gpu_gripper_shortcut import (B, CASES, KINDS, NAMES, W, _t, check_against_restatement, check_edge_case,  # noqa: E402
                                       check_identities, check_properties, dev, run_form, same)
from test_gpu_roadmap_cloud import sliced  # noqa: E402
from test_gripper_roadmap_cloud_host import CLOUD_BAND  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = fgc.ROADMAP_SEED
PR = fgc.POINT_RADIUS


class CloudForm:
    """``mpx_gripper_shortcut_cloud`` on one scenario: the device call and the restatement's rule (one cloud, one field, the
    same for every row).  ``field``: a ``CloudField`` of batch B on another grid than the default one."""
    band = CLOUD_BAND

    def __init__(self, kind, field=None):
        from mpinets_amd.field import CloudField

        self.kind = kind
        self.cloud = _t(fgc.surface_cloud(kind))[None].repeat(B, 1, 1)
        self.field = build_field(self.cloud, PR) if field is None else field
        assert isinstance(self.field, CloudField) and torch.equal(self.field.values, self.field.values[:1].expand_as(self.field.values))
        self.values, self.grid = self.field.values[0].cpu().numpy(), grid_dict(self.field.grid)

    def roadmap(self, sp, gp, **kw):
        from mpinets_amd import robot

        return robot.gripper_roadmap_cloud(sp, gp, self.cloud, field=self.field, point_radius=PR, W=W, seed=SEED,
                                           return_graph=True, **kw)

    def shortcut(self, pts, cnt, rows=slice(None), **kw):
        from mpinets_amd import robot

        return robot.gripper_shortcut_cloud(pts, cnt, self.cloud[rows], field=sliced(self.field, rows), point_radius=PR,
                                            W=kw.pop("W", W), **kw)

    def rule(self, b, clearance=0.0):
        return fgs.field_rule(self.values, self.grid, PR, clearance=clearance)

    def rule_without_env(self):
        return fgs.field_rule(None, None)

    def c_call(self, rows, with_env, pts, cnt, Bn, Pin, Wn, goal, opt, outs):
        """The C entry on the scenario's rows ``rows`` (``with_env`` False: field NULL and S = 0)."""
        from mpinets_amd import _lib, robot

        p = _lib.ptr
        sc, sr, sl = robot._ik_sphere_table(dev(), False) if with_env else (None, None, None)
        values = self.field.values[rows].contiguous() if with_env else None
        _lib.call("mpx_gripper_shortcut_cloud", p(pts), p(cnt), Bn, Pin, Wn, p(goal), ft.FINGER_OPENING, p(sc), p(sr), p(sl),
                  int(sc.size(0)) if with_env else 0, p(values), ctypes.byref(self.field.grid) if with_env else None, PR, 0.0,
                  ctypes.byref(opt), *[p(o) for o in outs])


@pytest.fixture(scope="module")
def runs():
    torch.cuda.set_device(0)
    sp, gp = fg.problems(B)
    return {kind: run_form(CloudForm(kind), sp, gp) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_decisions_and_outputs_against_float64(runs, kind):
    check_against_restatement(runs[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_properties_of_the_devices_own_output(runs, kind):
    check_properties(runs[kind])


@pytest.mark.parametrize("kind", KINDS)
def test_no_passes_halves_and_negated_quaternions(runs, kind):
    check_identities(runs[kind])


def test_without_a_field_it_is_the_primitive_form_without_primitives(runs):
    """``field=None`` and no cloud: every output equals ``gripper_shortcut`` without primitives on the same polylines, bit
    for bit (only the self test can block a chord)."""
    from mpinets_amd import robot

    run = runs["wall"]
    bare = robot.gripper_shortcut(run["pts"], run["cnt"], W=W, goal_pose=run["b"], return_trace=True)
    none = robot.gripper_shortcut_cloud(run["pts"], run["cnt"], None, W=W, goal_pose=run["b"], return_trace=True)
    for name, a, b in zip(NAMES, bare, none):
        assert same(a, b), name
    ok = bare[1] == 0
    assert bool((bare[3][ok] >= 2).all()) and int((bare[3][ok] == 2).sum()) > int(ok.sum()) // 2  # most rows: one edge


def test_gripper_plan_cloud_composes_the_two(runs):
    """``gripper_plan_cloud(shortcut=None)`` is ``gripper_roadmap_cloud``; with the default its poses are
    ``gripper_shortcut_cloud``'s on the roadmap's ``nodes[path]`` through the same field, its status the roadmap's."""
    from mpinets_amd import robot

    run = runs["cylinder"]
    form, a, b = run["form"], run["a"], run["b"]
    kw = dict(field=form.field, point_radius=PR, W=W, seed=SEED)
    off = robot.gripper_plan_cloud(a, b, form.cloud, shortcut=None, **kw)
    assert len(off) == 2 and same(off[0], run["road"][0]) and torch.equal(off[1], run["road"][1])
    on = robot.gripper_plan_cloud(a, b, form.cloud, return_length=True, **kw)
    assert same(on[0], run["out"][0]) and torch.equal(on[1], run["road"][1]) and same(on[2], run["out"][4])
    assert bool(torch.isnan(on[0][on[1] != 0]).all()) and not bool(torch.isnan(on[0][on[1] == 0]).any())
    own = robot.gripper_plan_cloud(a, b, form.cloud, point_radius=PR, W=W, seed=SEED)  # (its own field: the default grid's)
    assert same(own[0], on[0])


# ---- the edges of the shape space ------------------------------------------------------------------------------------------------
CLOUD_CASES = dict(CASES, smallest_grid=dict(grid="smallest"), grid_ends_inside=dict(grid="inside"))


def _other_grid(which, trunc):
    """-> a ``CloudField`` of batch B on a grid of 2 x 2 x 2 nodes one metre apart with hand-made nodal values below
    ``trunc`` (a field built from a cloud would be saturated at every such node), or on a grid of 5 cm voxels that ends at
    x = 0.45, the wall's centre plane, inside the box of every polyline, built from the wall's cloud."""
    from mpinets_amd.field import CloudField, make_grid

    if which == "smallest":
        grid = make_grid((0.0, -0.5, 0.0), (1.0, 0.5, 1.0), 1.0, trunc)
        assert (grid.nx, grid.ny, grid.nz) == (2, 2, 2)
        values = _t(np.float32([0.03, 0.17, 0.12, 0.05, 0.16, 0.04, 0.06, 0.15]).reshape(1, 2, 2, 2)).repeat(B, 1, 1, 1)
        return CloudField(values.contiguous(), grid)
    grid = make_grid((0.2, -0.5, 0.1), (0.45, 0.5, 0.8), 0.05, trunc)
    assert abs(float(grid.lo[0]) + (grid.nx - 1) * float(grid.h) - 0.45) < 1e-5
    cloud = _t(fgc.surface_cloud("wall"))[None].repeat(B, 1, 1)
    return CloudField.build(cloud, grid=grid)


@pytest.mark.parametrize("case", list(CLOUD_CASES), ids=list(CLOUD_CASES))
def test_edges_of_the_shape_space(runs, case):
    run = runs["wall"]
    c = CLOUD_CASES[case]
    if "grid" in c:
        run = dict(run, form=CloudForm("wall", _other_grid(c["grid"], float(run["form"].field.grid.trunc))))
    check_edge_case(run, case, c)


# ---- the callers -----------------------------------------------------------------------------------------------------------------
def test_make_problem_batch_with_the_shortcut_guide_against_the_cloud():
    """``make_problem_batch(hybrid_guide="gripper_cloud", hybrid_shortcut=True)`` at B = 16: opt-in; the flag off is the call
    without it; only ``hybrid_guide_poses``, ``hybrid_solutions``, ``hybrid_valid`` and ``hybrid_target_pose`` may differ; rows
    that are not ``hybrid_valid`` are NaN.  The counts are printed, not asserted (profiles/gripper_shortcut_timing.md)."""
    from mpinets_amd import scenes

    torch.cuda.set_device(0)
    kw = dict(seed=3, collision_free=True, expert=True, expert_from="cloud", hybrid=True, hybrid_against="cloud",
              hybrid_guide="gripper_cloud")
    base = scenes.make_problem_batch(16, **kw)
    off = scenes.make_problem_batch(16, hybrid_shortcut=False, **kw)
    on = scenes.make_problem_batch(16, hybrid_shortcut=True, **kw)
    assert set(base) == set(off) == set(on)
    for k in base:
        assert same(base[k], off[k]), k
        if k not in ("hybrid_guide_poses", "hybrid_solutions", "hybrid_valid", "hybrid_target_pose"):
            assert same(base[k], on[k]), k
    gst = on["hybrid_guide_status"]
    assert bool(torch.isnan(on["hybrid_guide_poses"][gst != 0]).all()) and not bool(torch.isnan(on["hybrid_guide_poses"][gst == 0]).any())
    assert bool(torch.isnan(on["hybrid_solutions"][~on["hybrid_valid"]]).all())
    assert not bool((on["hybrid_valid"] & ((gst != 0) | ~on["expert_valid"])).any())
    found = gst == 0
    assert torch.equal(on["hybrid_guide_poses"][found][:, -1], base["hybrid_guide_poses"][found][:, -1])  # the goal, bit for bit
    print(f"hybrid_valid of 16 against the scene clouds (expert_valid {int(on['expert_valid'].sum())}, gripper paths "
          f"{int(found.sum())}): roadmap guide {int(base['hybrid_valid'].sum())}, shortcut guide {int(on['hybrid_valid'].sum())}")


def test_plan_to_poses_with_the_shortcut_guide():
    """``follow_guide="gripper", follow_shortcut=True`` on a small cloud: the keys of the call without the flag; every key the
    guide does not feed is unchanged; the guide is NaN exactly where the roadmap found no path and its last pose is the
    roadmap's (the goal) bit for bit; rows the follower did not finish are NaN."""
    from mpinets_amd import capture, scenes

    torch.cuda.set_device(0)
    n, pr = 8, scenes.EXPERT_CLOUD_POINT_RADIUS
    prob = scenes.make_problem_batch(n, device=dev(), device_clouds=True, seed=4, kinds=("tabletop", "cubby", "dresser"), M1=40,
                                     M2=16, collision_free=True)
    cloud = prob["xyz"][:, 2048:6144, :3]
    kw = dict(point_radius=pr, seed=4, follow=True, follow_guide="gripper")
    off = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], **kw)
    on = capture.plan_to_poses(cloud, prob["q"], prob["target_pose"], follow_shortcut=True, **kw)
    assert set(on) == set(off)
    fed = ("follow_guide_poses", "followed_trajectory", "follow_status", "follow_bits", "follow_steps")
    for k, v in off.items():
        assert k in fed or same(v, on[k]), k
    gst, st = on["follow_guide_status"], on["follow_status"]
    print(f"plan_to_poses(follow_shortcut=True): guide status {gst.tolist()}, follow status {st.tolist()} (without the shortcut "
          f"{off['follow_status'].tolist()})")
    assert bool(torch.isnan(on["follow_guide_poses"][gst != 0]).all()) and not bool(torch.isnan(on["follow_guide_poses"][gst == 0]).any())
    found = gst == 0
    assert torch.equal(on["follow_guide_poses"][found][:, -1], off["follow_guide_poses"][found][:, -1])
    assert bool((st[gst != 0] == 2).all()) and bool(torch.isnan(on["followed_trajectory"][st != 0]).all())
