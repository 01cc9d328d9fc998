"""The host generators' second stage (parameters -> primitives and supports) against fixtures made by RUNNING the reference
(tests/golden/gen_scene_reference_golden.py -> scene_reference_golden.npz): 16 cubbies with explicitly set parameters in the
four thickness states (``Cubby.cuboids``, ``Cubby.support_volumes``), ``MergedCubbyEnvironment.gen``'s rule on the twelve
ordered pocket pairs, ``place_objects``' greedy walk on scripted points and objects, and ``setup_tables`` under a recorded
random source.  Float64 against float64: 1e-12; discrete results exactly."""
import os

import numpy as np
import pytest

from mpinets_amd import scenes

TOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_reference_golden.npz"))


NAMES = {"cubby_left": "left", "cubby_right": "right", "cubby_bottom": "bottom", "cubby_front": "front", "cubby_back": "back",
         "cubby_top": "top", "cubby_mid_h_z": "mid_h_z", "cubby_mid_v_y": "mid_v_y", "in_cabinet_rotation": "rotation"}


def test_cubby_plates_and_supports_in_the_four_thickness_states(golden):
    assert len(golden["cubby_params"]) >= 4 * 16
    states = set()
    for values, plates, supports, counts in zip(golden["cubby_params"], golden["cubby_plates"], golden["cubby_supports"], golden["cubby_counts"]):
        p = {NAMES.get(k, k): float(v) for k, v in zip(golden["cubby_keys"], values)}
        got_plates, got_supports, yaw = scenes._cubby_reference_primitives(p)
        quat = scenes._yaw_quat(yaw)
        # the reference keeps a zero-thickness cuboid where a plate is removed; here the row is dropped and the later ones move up
        assert counts[0] == 7
        kept = plates[(plates[:, 3:6] != 0).all(1)]
        states.add((p["middle_shelf_thickness"] == 0, p["center_wall_thickness"] == 0))
        assert len(kept) == len(got_plates) == 7 - (p["middle_shelf_thickness"] == 0) - (p["center_wall_thickness"] == 0)
        for ref, (c, d) in zip(kept, got_plates):
            assert np.abs(ref - np.r_[c, d, quat]).max() <= TOL
        assert counts[1] == len(got_supports)
        for ref, (c, d) in zip(supports, got_supports):
            assert np.abs(ref - np.r_[c, d, quat]).max() <= TOL
        assert np.isnan(supports[len(got_supports):]).all()
    assert len(states) == 4


def test_merge_rule_and_pocket_to_support_map(golden):
    rows = golden["merge_rule"]
    assert len(rows) == 12 and len({(a, b) for a, b, *_ in rows}) == 12
    base = scenes._cubby_reference_parameters(np.random.default_rng(3))
    for a, b, shelf_gone, wall_gone, start_support, goal_support in rows:
        p = scenes.merged_cubby_parameters(base, (a, b))
        assert (p["middle_shelf_thickness"] == 0.0) == bool(shelf_gone) and (p["center_wall_thickness"] == 0.0) == bool(wall_gone)
        assert scenes.merged_support_index(int(a), p) == start_support and scenes.merged_support_index(int(b), p) == goal_support


def test_greedy_placement_picks_the_same_candidates_with_the_same_clearance(golden):
    total = 0
    for points, objs, K, accepted, clearance in zip(golden["place_points"], golden["place_objects"], golden["place_K"],
                                                    golden["place_accepted"], golden["place_clearance"]):
        points = points[:10 * K]
        script = [("cylinder", o[1], o[2], o[3]) if o[0] == 1 else ("cuboid", o[1], o[2], o[3], o[4], o[5]) for o in objs if o[0] > 0]
        n = [0]

        def new_object(x, y, m):
            o = script[n[0]]  # the object the reference's scripted ``random_object`` returned for its n-th accept
            n[0] += 1
            return o

        _, got_accepted, got_clearance = scenes._place_objects(points, int(K), new_object)
        want = accepted[accepted >= 0].astype(int).tolist()
        assert got_accepted == want and len(want) == len(script)
        assert np.abs(np.array(got_clearance) - clearance[:len(want)]).max() <= TOL
        total += len(want)
    assert total > 100


def test_setup_tables(golden):
    sides = 0
    for values, task, free in zip(golden["tables_params"], golden["tables_task"], golden["tables_free"]):
        p = {k: float(v) for k, v in zip(golden["table_keys"], values)}
        p["has_side_table"] = bool(p["has_side_table"])
        sides += p["has_side_table"]
        got_task, got_free = scenes._tabletop_reference_tables(p)
        for ref, got in ((task, got_task), (free, got_free)):
            ref = ref[~np.isnan(ref).any(1)]
            assert len(ref) == len(got)
            for r, (c, d) in zip(ref, got):
                assert np.abs(r - np.r_[c, d]).max() <= TOL
    assert 0 < sides < len(golden["tables_params"])
