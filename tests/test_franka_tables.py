"""The robot data the engine ships == the only Franka data the reference tree holds (no GPU).

tests/golden/franka_golden.npz is parsed from /root/reference/config/franka_robot_description.yaml:44-53,57-182 and
franka_fabric_config.yaml:117-140 by tests/golden/gen_franka_golden.py.  Joint limits, FK constants and the
mesh-sampled point tables live in the un-vendored robofin (parity unpinned);
tools/dump_robofin_tables.py produces them for users who have it.
"""
import ast
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "franka_golden.npz"), allow_pickle=False))


def test_collision_spheres_equal_the_reference_yaml(gold):
    from mpinets_amd import franka_tables as ft

    flat = [(link, c, r) for link, spheres in ft.COLLISION_SPHERES.items() for c, r in spheres]
    assert len(flat) == len(gold["sphere_radius"]) == 57
    assert [f[0] for f in flat] == [str(n) for n in gold["sphere_link"]]  # same links, same order
    np.testing.assert_array_equal(np.asarray([f[1] for f in flat], np.float64), gold["sphere_center"])
    np.testing.assert_array_equal(np.asarray([f[2] for f in flat], np.float64), gold["sphere_radius"])
    assert len(set(gold["sphere_radius"].tolist())) == 10


def test_flat_sphere_table_is_a_regrouping_of_the_yaml(gold):
    """collision_sphere_table(): grouped by radius in order of first appearance (model.py:300-312 iterates radius
    groups); every YAML sphere appears exactly once, link0 only when with_base_link."""
    from mpinets_amd import franka_tables as ft

    for with_base in (False, True):
        c, r, l, groups = ft.collision_sphere_table(with_base)
        keep = np.array([with_base or str(n) != "panda_link0" for n in gold["sphere_link"]])
        assert len(r) == keep.sum() == (57 if with_base else 56)
        want = sorted((str(n), tuple(np.float32(cc)), np.float32(rr)) for n, cc, rr in
                      zip(gold["sphere_link"][keep], gold["sphere_center"][keep], gold["sphere_radius"][keep]))
        got = sorted((ft.LINK_NAMES[li], tuple(cc), rr) for li, cc, rr in zip(l, c, r))
        assert got == want
        first_seen = list(dict.fromkeys(np.float32(gold["sphere_radius"][keep]).tolist()))
        assert [np.float32(g[0]) for g in groups] == [np.float32(x) for x in first_seen]
        assert sum(g[2] for g in groups) == len(r) and all(np.all(r[s:s + n] == np.float32(rad)) for rad, s, n in groups)


def test_default_configuration_and_finger_opening(gold):
    from mpinets_amd import franka_tables as ft

    np.testing.assert_array_equal(ft.DEFAULT_Q, gold["default_q"])
    assert ft.DOF == len(gold["cspace"]) == 7
    assert [str(n) for n in gold["finger_joint"]] == ["panda_finger_joint1", "panda_finger_joint2"]
    assert (gold["finger_value"] == ft.FINGER_OPENING).all()


def test_fabric_self_collision_model(gold):
    from mpinets_amd import franka_tables as ft

    np.testing.assert_array_equal(ft.FABRIC_BODY_CYLINDER["pt1"], gold["body_cylinder_pt1"])
    np.testing.assert_array_equal(ft.FABRIC_BODY_CYLINDER["pt2"], gold["body_cylinder_pt2"])
    assert ft.FABRIC_BODY_CYLINDER["radius"] == float(gold["body_cylinder_radius"])
    ref = dict(zip((str(n) for n in gold["self_sphere_name"]), gold["self_sphere_radius"].tolist()))
    for name, radius in ft.FABRIC_SELF_SPHERES:
        assert ref[name] == radius and name in ft.LINK_ID
    # the kernels' one statement of the model (csrc/franka_device.h) holds these numbers ...
    csrc = os.path.join(ROOT, "motion-policy-networks_amd", "csrc")
    src = open(os.path.join(csrc, "franka_device.h")).read()

    def constant(name):
        (text,) = re.findall(r"^constexpr (?:float|int) %s(?:\[\w+\])? = (.+?);" % name, src, re.M)
        return ast.literal_eval(re.sub(r"(?<=\d)f\b", "", text).replace("{", "[").replace("}", "]"))

    z0, z1 = constant("FRANKA_SELF_SEGMENT_Z0"), constant("FRANKA_SELF_SEGMENT_Z1")
    assert (0.0, 0.0, z1) == ft.FABRIC_BODY_CYLINDER["pt1"] and (0.0, 0.0, z0) == ft.FABRIC_BODY_CYLINDER["pt2"]
    assert constant("FRANKA_SELF_BODY_RADIUS") == ft.FABRIC_BODY_CYLINDER["radius"]
    assert constant("FRANKA_SELF_SPHERES") == len(ft.FABRIC_SELF_SPHERES)
    assert constant("FRANKA_SELF_FRAME") == [ft.LINK_ID[n] for n, _ in ft.FABRIC_SELF_SPHERES] == [7, 9, 12, 13]
    assert constant("FRANKA_SELF_RADIUS") == [r for _, r in ft.FABRIC_SELF_SPHERES]
    # ... and nothing else under csrc/ writes the comparison's literal
    others = [f for f in sorted(os.listdir(csrc)) if f != "franka_device.h" and os.path.isfile(os.path.join(csrc, f))
              and not f.endswith((".o", ".so"))]
    assert len(others) > 20 and src.count("0.15f") == 1
    for f in others:
        assert "0.15f" not in open(os.path.join(csrc, f), errors="replace").read(), f


def test_dumped_point_tables_round_trip(tmp_path):
    """The file format of tools/dump_robofin_tables.py -> load_point_tables -> FrankaSampler(point_table=...)."""
    from mpinets_amd import franka_tables as ft

    pts, lids = ft.link_point_table(256, True)
    path = tmp_path / "robofin_tables.npz"
    np.savez(path, points=pts, point_link_name=np.asarray([ft.LINK_NAMES[i] for i in lids], dtype="U32"),
             joint_limits_real=ft.JOINT_LIMITS_REAL)
    got = ft.load_point_tables(str(path))
    np.testing.assert_array_equal(got["point_table"][0], pts)
    np.testing.assert_array_equal(got["point_table"][1], lids)
    np.testing.assert_array_equal(got["joint_limits_real"], ft.JOINT_LIMITS_REAL)
    np.savez(path, points=pts[:1], point_link_name=np.asarray(["no_such_link"], dtype="U32"))
    with pytest.raises(ValueError):
        ft.load_point_tables(str(path))
