"""Host-side checks of the device scene source (no GPU): the float64 restatement of ``mpx_scene_generate``
(tests/float64_scene_gen.py) against the host generators' distributions and against the structure the contract promises, the
entry's refusals that need no device, and ``make_problem_batch``'s ``scene_source`` switch.

The bar of the GPU test (tests/test_gpu_scene_gen.py), derived and not measured.  ``FLOAT_TOL`` = 4e-6 absolute: about 16
float32 ulps at the largest coordinate magnitude of these scenes, 2 m.  By the contract's operation count an output is at
most eight rounded float32 operations from its uniforms -- the longest chain is a dresser plate's x: W (one fma), W / rows,
the local x (one fma), c lx, s ly, their difference, + ox: seven -- each within 0.5 ulp (1.2e-7 at 2 m), plus a float32 sine
or cosine within 2e-7 (the header's figure for ``mpx_task_candidates``) of a yaw that is itself one rounded fma (1.2e-7 rad at
2.6 rad), on a lever arm below 1 m: about 8 x 1.2e-7 + 2e-7 + 1.2e-7 = 1.3e-6 in the worst case, three times headroom.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_scene_gen as fsg  # noqa: E402
from mpinets_amd import scenes  # noqa: E402

FLOAT_TOL = 4e-6  # [m, or quaternion / radian units]
KINDS = ("tabletop", "cubby", "dresser")
N_SCENES, M1, M2, S = 2000, 40, 16, 8


# ---- distribution ------------------------------------------------------------------------------------------------------------
def _per_scene_mean(values, live):
    """Mean of ``values`` [B,M] over each scene's live rows -> [B'] (scenes without a live row left out).  The statistic is a
    mean over SCENES, which are independent, of one number per scene: rows of one scene share its parameters, so a standard
    error taken over the rows would be too small."""
    count = live.sum(1)
    keep = count > 0
    return (np.where(live, values, 0.0).sum(1)[keep] / count[keep])


def statistics(scn, kind):
    """One scene kind's arrays -> {name: float64 [scenes]}: each entry is compared by its mean."""
    scn = {k: np.asarray(v, np.float64) if v.dtype != np.int32 else v for k, v in scn.items()}
    cub, cyl, sup = fsg.live_rows(scn)
    st = {"live cuboids": cub.sum(1), "live cylinders": cyl.sum(1), "live supports": sup.sum(1)}
    if kind == "tabletop":
        st["zero-height table"] = scn["cuboid_centers"][:, 0, 2] == -np.float64(np.float32(0.025))
        st["side table"] = sup.sum(1) == 2
    for a in range(3):
        st[f"cuboid dim {a}"] = _per_scene_mean(scn["cuboid_dims"][..., a], cub)
        st[f"support dim {a}"] = _per_scene_mean(scn["support_boxes"][..., 3 + a], sup)
    st["cylinder radius"] = _per_scene_mean(scn["cylinder_radii"][..., 0], cyl)
    st["cylinder height"] = _per_scene_mean(scn["cylinder_heights"][..., 0], cyl)
    st["cuboid yaw"] = _per_scene_mean(2 * np.arctan2(scn["cuboid_quats"][..., 3], scn["cuboid_quats"][..., 0]), cub)
    st["cuboid centre x"] = _per_scene_mean(scn["cuboid_centers"][..., 0], cub)
    return {k: np.asarray(v, np.float64) for k, v in st.items()}


def _compare(ref, other, what):
    """Every mean of ``other`` within five standard errors of ``ref``'s own sample of ``ref``'s mean."""
    worst = 0.0
    for name, x in ref.items():
        y = other[name]
        if len(x) == 0 or x.std() == 0:  # (a constant of the kind: seven plates, no cylinders, four pockets)
            assert len(y) == len(x) and (len(x) == 0 or (y == x[0]).all()), (what, name)
            continue
        se = x.std(ddof=1) / np.sqrt(len(x))
        z = abs(y.mean() - x.mean()) / se
        worst = max(worst, z)
        assert z <= 5.0, f"{what}: {name}: {y.mean():.6g} against {x.mean():.6g}, {z:.2f} standard errors"
    return worst


@pytest.fixture(scope="module")
def host_samples():
    return {kind: (statistics(scenes.make_task_scenes(N_SCENES, 0, (kind,), M1, M2, S), kind),
                   statistics(scenes.make_task_scenes(N_SCENES, 1, (kind,), M1, M2, S), kind)) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_draws_the_host_generators_distribution(kind, host_samples):
    """2000 scenes per kind at M1 = 40, M2 = 16, S = 8: the share of zero-height tables, the share with a side table, the mean
    counts of live cuboids, cylinders and supports, the means of every dim column (cuboids, supports, cylinder radius and
    height), of the yaw and of the centre's x -- the last ones as means over scenes of each scene's mean over its live rows --
    lie within five standard errors of the host generator's own sample.  The host generator at a second seed is held to the
    same bar: a statistic it missed against itself would be the wrong statistic."""
    host, host_again = host_samples[kind]
    code = scenes.SCENE_KIND_CODES[kind]
    rest = statistics(fsg.generate(np.full(N_SCENES, code), np.arange(N_SCENES), M1, M2, S, seed=0), kind)
    z_self = _compare(host, host_again, f"{kind}, host seed 1 against host seed 0")
    z = _compare(host, rest, f"{kind}, restatement against host")
    print(f"{kind}: largest deviation {z:.2f} standard errors (the host against itself: {z_self:.2f})")


# ---- structure ---------------------------------------------------------------------------------------------------------------
SHAPES = [(16, 16, 8), (64, 64, 64), (3, 0, 1), (5, 2, 4), (40, 16, 8)]


def check_structure(scn, kind, m1, m2, s):
    """What the contract promises of every output, whoever computed it (the GPU test runs this on the kernel's arrays):
    padding rows are zero with the identity quaternion, live rows form a prefix, counts respect M1 / M2 / S."""
    cub, cyl, sup = fsg.live_rows(scn)
    for live, keys in ((cub, ("cuboid_centers", "cuboid_dims", "cuboid_quats")),
                       (cyl, ("cylinder_centers", "cylinder_radii", "cylinder_heights", "cylinder_quats"))):
        assert (np.diff(live.astype(int), axis=1) <= 0).all()  # (a prefix)
        for key in keys:
            pad = np.asarray(scn[key])[~live]
            want = [1, 0, 0, 0] if key.endswith("quats") else 0
            assert (pad == want).all(), key
    assert (np.asarray(scn["cylinder_quats"]) == [1, 0, 0, 0]).all()
    assert (np.asarray(scn["cuboid_quats"])[..., 1:3] == 0).all()
    assert cub.shape[1] == m1 and cyl.shape[1] == m2
    if sup is not None:
        boxes = np.asarray(scn["support_boxes"])
        assert sup.shape[1] == s and (np.diff(sup.astype(int), axis=1) <= 0).all()
        assert (boxes[~sup] == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]).all()
        assert (boxes[sup][:, 3:6] > 0).all() and (boxes[sup][:, 11] > 0).all() and (boxes[..., 7:9] == 0).all()
    kind = np.asarray(kind)
    other = ~np.isin(kind, (0, 1, 2))
    assert not cub[other].any() and not cyl[other].any() and (sup is None or not sup[other].any())
    t, c, d = kind == fsg.TABLETOP, kind == fsg.CUBBY, kind == fsg.DRESSER
    assert (cub[t].sum(1) >= 3).all() and (cub[c].sum(1) == min(7, m1)).all() and not cyl[c | d].any()
    assert (cub[d].sum(1) >= min(12, m1)).all() and (cub[d].sum(1) <= min(40, m1)).all()
    if sup is not None:
        assert (np.asarray(scn["support_kind"])[t][sup[t]] == fsg.SURFACE).all()
        assert (np.asarray(scn["support_kind"])[c | d][sup[c | d]] == fsg.VOLUME).all()
        assert (sup[c].sum(1) == min(4, s)).all() and (sup[d].sum(1) == np.minimum(s, cub[d].sum(1))).all()
        assert ((sup[t].sum(1) >= 1) & (sup[t].sum(1) <= min(2, s))).all()


@pytest.mark.parametrize("m1,m2,s", SHAPES)
def test_restatement_structure(m1, m2, s):
    B = 300
    kind, ids = np.arange(B) % 3, np.arange(B) + 11
    scn = fsg.generate(kind, ids, m1, m2, s, seed=5)
    assert np.isfinite(np.concatenate([np.ravel(v) for v in scn.values()])).all()
    check_structure(scn, kind, m1, m2, s)
    cub, cyl, sup = fsg.live_rows(scn)
    t, c, d = (kind == k for k in (0, 1, 2))
    # a tabletop's first support is cuboid 0's box, weight = the top face's area; the mount table stands behind the tables
    boxes = scn["support_boxes"]
    assert np.array_equal(boxes[t, 0, :6], np.concatenate([scn["cuboid_centers"][t, 0], scn["cuboid_dims"][t, 0]], -1))
    assert np.array_equal(boxes[t, 0, 11], boxes[t, 0, 3] * boxes[t, 0, 4]) and (boxes[t, 0, 10] == 0).all()
    mount = np.where(sup[t].sum(1) == 2, 2, 1) if s >= 2 else None
    if mount is not None:
        assert np.array_equal(scn["cuboid_dims"][t][np.arange(t.sum()), mount], np.tile(np.float32([0.6, 0.6, 0.05]).astype(float), (t.sum(), 1)))
    assert (scn["cuboid_dims"][t, 0, 2] == np.float32(0.05)).all()  # thick
    assert (cub[t].sum(1) <= m1).all() and (cyl[t].sum(1) <= m2).all()
    if m2 >= 14 and m1 >= 17:  # (nothing overflows: 3 tables and 14 objects at most)
        assert ((cub[t].sum(1) + cyl[t].sum(1)) >= 2 + 3).all() and ((cub[t].sum(1) + cyl[t].sum(1)) <= 3 + 14).all()
    elif m1 <= 5:  # the overflow and drop paths are taken
        assert (cub[t].sum(1) == m1).any() and (m2 == 0 or (cyl[t].sum(1) == m2).any())
    # a cubby's pockets lie inside the shelf's bounding box (in the cubby's frame: all share its yaw)
    if m1 >= 7:
        for b in np.flatnonzero(c)[:50]:
            yaw = 2 * np.arctan2(scn["cuboid_quats"][b, 0, 3], scn["cuboid_quats"][b, 0, 0])
            R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
            lo = (scn["cuboid_centers"][b, :7] @ R - scn["cuboid_dims"][b, :7] / 2).min(0)
            hi = (scn["cuboid_centers"][b, :7] @ R + scn["cuboid_dims"][b, :7] / 2).max(0)
            n = min(4, s)
            assert ((boxes[b, :n, :3] @ R - boxes[b, :n, 3:6] / 2) >= lo - 1e-12).all()
            assert ((boxes[b, :n, :3] @ R + boxes[b, :n, 3:6] / 2) <= hi + 1e-12).all()
    # the dresser's approach has a positive world-x component (the contract's simplification holds)
    assert (np.cos(boxes[d][sup[d]][:, 10]) > 0).all()
    # scenes depend on their own id alone
    again = fsg.generate(kind[::-1], ids[::-1], m1, m2, s, seed=5)
    assert all(np.array_equal(again[k][::-1], scn[k]) for k in scn)
    assert not np.array_equal(fsg.generate(kind, ids, m1, m2, s, seed=6)["cuboid_dims"], scn["cuboid_dims"])


def test_restatement_without_supports_is_make_scenes_form():
    kind, ids = np.arange(9) % 3, np.arange(9)
    a, b = fsg.generate(kind, ids, 16, 16, 0), fsg.generate(kind, ids, 16, 16, 8)
    assert set(a) == set(fsg.PRIMITIVE_KEYS) and all(np.array_equal(a[k], b[k]) for k in a)


# ---- the library, without a GPU -------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_operands_without_gpu():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert lib.mpx_version() == 341
    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched

    def call(B=4, m1=16, m2=16, s=8, offset=0, boxes=one, kinds=one):
        return lib.mpx_scene_generate(one, None, B, m1, m2, s, 0, offset, one, one, one, one, one, one, one, boxes, kinds, None)

    for kw, text in ((dict(m1=2), b"M1 = 2"), (dict(m1=65), b"M1 = 65"), (dict(m2=65), b"M2 = 65"), (dict(s=65), b"S = 65"),
                     (dict(boxes=None), b"go together"), (dict(kinds=None), b"go together"),
                     (dict(s=8, boxes=None, kinds=None), b"without support arrays"),
                     (dict(offset=-1), b"scene_offset is negative"), (dict(offset=(1 << 32) - 3), b"exceeds 2^32")):
        assert call(**kw) != 0, kw
        assert text in lib.mpx_last_error(), (kw, lib.mpx_last_error())
    assert lib.mpx_scene_generate(None, None, 0, 16, 16, 0, 0, 0, None, None, None, None, None, None, None, None, None, None) == 0
    assert lib.mpx_scene_generate(None, None, 0, 16, 16, 0, 0, 1 << 32, None, None, None, None, None, None, None, None, None, None) == 0
    assert lib.mpx_scene_generate(None, None, 4, 16, 16, 0, 0, 0, one, one, one, one, one, one, one, None, None, None) != 0
    assert b"NULL operand" in lib.mpx_last_error()
    assert lib.mpx_scene_generate(one, None, 4, 16, 16, 0, 0, 0, one, one, one, None, one, one, one, None, None, None) != 0
    assert b"NULL output" in lib.mpx_last_error()


# ---- make_problem_batch ----------------------------------------------------------------------------------------------------------
def test_scene_source_switch(monkeypatch):
    """An unknown ``scene_source`` and "device" without device clouds are refused; the default and "host" reach ``make_scenes``
    and never the device source; "device" reaches ``make_scenes_device`` with this batch's scene ids and nothing else."""
    assert inspect.signature(scenes.make_problem_batch).parameters["scene_source"].default == "host"
    with pytest.raises(ValueError, match="scene_source must be"):
        scenes.make_problem_batch(2, device="cpu", scene_source="numpy")
    with pytest.raises(ValueError, match="device_clouds=True"):
        scenes.make_problem_batch(2, device="cpu", scene_source="device")
    with pytest.raises(ValueError, match="device_clouds=True"):
        scenes.make_problem_batch(2, device="cpu", scene_source="device", device_clouds=False)

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached

    def wrong(*a, **k):
        raise AssertionError("the other source")

    monkeypatch.setattr(scenes, "make_scenes", reached)
    monkeypatch.setattr(scenes, "make_scenes_device", wrong)
    for kw in ({}, {"scene_source": "host"}, {"scene_source": "host", "device_clouds": True}):
        with pytest.raises(Reached):
            scenes.make_problem_batch(2, device="cpu", **kw)
    seen = {}

    def device_source(B, seed, kinds, m1, m2, S=None, device=None, scene_ids=None, **k):
        seen.update(B=B, S=S, ids=scene_ids.tolist())
        raise Reached

    monkeypatch.setattr(scenes, "make_scenes", wrong)
    monkeypatch.setattr(scenes, "make_task_scenes", wrong)
    monkeypatch.setattr(scenes, "make_scenes_device", device_source)
    with pytest.raises(Reached):
        scenes.make_problem_batch(4, device="cpu", scene_source="device", device_clouds=True, env_offset=5, total_envs=16, scene_pool=3)
    assert seen == dict(B=4, S=None, ids=[2, 0, 1, 2])
    with pytest.raises(Reached):
        scenes.make_problem_batch(2, device="cpu", scene_source="device", device_clouds=True, env_offset=14, problems="task",
                                  collision_free=True)
    assert seen == dict(B=2, S=8, ids=[14, 15])
