"""Host-side checks of the reference's scenes (no GPU): "tabletop_reference", "cubby_reference" and "merged_cubby" -- the
float64 restatement of ``mpx_scene_generate_reference`` (tests/float64_scene_reference.py) against the host generators'
distributions, the bounds and the placement rule both must keep, the structure the contract promises, the refusals that
need no device and ``make_problem_batch``'s handling of the new kinds.

The bar of the GPU test (tests/test_gpu_scene_reference.py), derived and not measured.  ``FLOAT_TOL_REF`` = 5e-6 absolute.
By the contract's operation count the longest chain is a rotated cubby plate's or pocket's x or y: a parameter (one fma;
``back`` is two), the pivot px or py (a sum and a halving), the arm ax or ay (one difference), two products, their
difference or sum, + the pivot: ten rounded float32 operations, each within 0.5 ulp, which is 1.2e-7 at the largest
coordinate magnitude of these scenes, 2 m; plus a float32 sine and cosine within 2e-7 (the header's figure) on a lever arm
below 0.45 m, and the rounding of the yaw (one fma, 1.5e-8 rad) on the same arm: 10 x 1.2e-7 + 2 x 2e-7 x 0.45 + 1e-8 =
1.4e-6 in the worst case.  The pivot about the cabinet's centre is what lengthens the chain over ``FLOAT_TOL``'s eight.
A tabletop object's dims are fma(v, span, 0.05) with span = min(m, 0.15) - 0.05: they carry the error of the least
footprint distance m where m < 0.15, that is between points less than 0.4 m apart -- two positions four operations from
their uniforms each (4 x 1.2e-7 per coordinate difference), a rotation (2 x 2e-7 x 0.4 + three operations below 0.5 m,
3 x 3e-8), a hypotenuse and a difference (3 x 3e-8): about 1.3e-6, below the cubby's chain.  Three times headroom over
1.4e-6, as ``FLOAT_TOL`` keeps: 4.2e-6, rounded up to 5e-6.

FRAGILE scenes.  The tabletop's accept test compares a computed distance with 0.05 and its table pick compares
v_0 (A0 + A1) with A0; float32 and float64 may fall on different sides when the restatement's value lies within the two
sides' difference of the threshold.  That difference is bounded by the float bar (the distance over the whole table: the
same chain on a 2 m arm, 2 x 2e-7 x 2 + 8 x 1.2e-7 = 1.8e-6 < 5e-6), so ``FRAGILE_MARGIN`` = ``FLOAT_TOL_REF``: a scene
whose walk saw |d - 0.05| < 5e-6 m, or a pick within 5e-6 of its threshold in units of the uniform, is left out of the
exact comparison.  At most 1 in 20 of the compared tabletop scenes may be left out; ``test_fragile_scenes_are_rare``
counts them for the GPU test's seed on the CPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_scene_reference as fsr  # noqa: E402
from mpinets_amd import scenes  # noqa: E402
from test_scene_gen_host import _compare, statistics  # noqa: E402

FLOAT_TOL_REF = 5e-6  # [m, or quaternion / radian units]
FRAGILE_MARGIN = FLOAT_TOL_REF
FRAGILE_CAP = 1 / 20
GPU_SEED = 20  # the GPU test's seed: chosen here, from the restatement alone (test_fragile_scenes_are_rare)
KINDS = scenes.REFERENCE_KINDS
N_SCENES, M1, M2, S = 2000, 40, 16, 8


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def record_host(n, seed, kind):
    """``n`` host scenes of ``kind`` -> (make_task_scenes' arrays, per-scene records of the two stages)."""
    records = []
    place, tab_p, cub_p, merge = scenes._place_objects, scenes._tabletop_reference_parameters, \
        scenes._cubby_reference_parameters, scenes.merged_cubby_parameters

    def placing(points, how_many, new_object, **kw):
        got = place(points, how_many, new_object, **kw)
        records[-1].update(objects=got[0], accepted=got[1], clearances=got[2], K=how_many, points=len(points))
        return got

    def tabletop_parameters(rng):
        records.append(dict(params=tab_p(rng)))
        return records[-1]["params"]

    def cubby_parameters(rng):
        records.append(dict(params=cub_p(rng)))
        return records[-1]["params"]

    def merging(p, pair):
        records[-1]["pair"] = tuple(pair)
        return merge(p, pair)

    scenes._place_objects, scenes._tabletop_reference_parameters = placing, tabletop_parameters
    scenes._cubby_reference_parameters, scenes.merged_cubby_parameters = cubby_parameters, merging
    try:
        arrays = scenes.make_task_scenes(n, seed, (kind,), M1, M2, S)
    finally:
        scenes._place_objects, scenes._tabletop_reference_parameters = place, tab_p
        scenes._cubby_reference_parameters, scenes.merged_cubby_parameters = cub_p, merge
    return arrays, records


def least_clearance(objects):
    """The least distance of a placed object's centre to the footprint of an object placed BEFORE it (inf: fewer than two)."""
    return min((scenes._footprint_distance(objects[i], objects[j][1], objects[j][2])
                for j in range(len(objects)) for i in range(j)), default=np.inf)


def objects_of(aux, b):
    """Scene b's placed objects of the restatement, as the host's tuples, in placement order."""
    o = aux["objects"]
    return [("cylinder", o["x"][b, i], o["y"][b, i], o["r"][b, i]) if o["type"][b, i] == 1 else
            ("cuboid", o["x"][b, i], o["y"][b, i], o["dx"][b, i], o["dy"][b, i], float(np.arctan2(o["s"][b, i], o["c"][b, i])))
            for i in range(int(aux["placed"][b]))]


def table_counts(scn):
    """-> (tables, task tables) per scene: a table is a live cuboid with the identity quaternion whose bottom is z = -0.02."""
    scn = {k: np.asarray(v, np.float64) for k, v in scn.items()}
    bottom = scn["cuboid_centers"][..., 2] - scn["cuboid_dims"][..., 2] / 2
    table = (scn["cuboid_dims"] != 0).any(-1) & (scn["cuboid_quats"][..., 0] == 1) & (np.abs(bottom + 0.02) < 1e-6)
    return table.sum(1), (scn["support_kind"] == fsr.SURFACE).sum(1)


def new_statistics(scn, kind, clearance=None, merge_state=None):
    st = statistics(scn, kind)
    if kind == "tabletop_reference":
        tables, task = table_counts(scn)
        st["live task tables"], st["live free tables"] = task.astype(float), (tables - task - 1).astype(float)
        st["zero-height table"] = (np.abs(np.asarray(scn["cuboid_dims"], np.float64)[:, 0, 2] - 0.02) < 1e-6).astype(float)
        finite = np.asarray(clearance)[np.isfinite(clearance)]
        st["least pairwise object clearance"] = finite
    if kind == "merged_cubby":
        for name, state in (("share: shelf and wall removed", 3), ("share: wall alone removed", 2), ("share: shelf alone removed", 1)):
            st[name] = (np.asarray(merge_state) == state).astype(float)
    return st


def merge_state_of_arrays(scn):
    """1 shelf alone gone (two columns), 2 wall alone gone (two rows), 3 both, 0 unmerged -- read off supports and plates."""
    ns = (np.asarray(scn["support_kind"]) != 0).sum(1)
    dims = np.asarray(scn["support_boxes"], np.float64)[:, 0, 3:6]
    plates = (np.asarray(scn["cuboid_dims"]) != 0).any(-1).sum(1)
    assert np.array_equal(plates, np.select([ns == 4, ns == 2, ns == 1], [7, 6, 5]))
    wide = dims[:, 1] > 1.0  # (a support spanning right .. left is at least 1.2 m wide, a pocket at most 0.9 m)
    return np.select([ns == 4, ns == 1, wide], [0, 3, 2], 1)


@pytest.fixture(scope="module")
def samples():
    out = {}
    for kind in KINDS:
        code = scenes.SCENE_KIND_CODES[kind]
        rest, aux = fsr.generate(np.full(N_SCENES, code), np.arange(N_SCENES), M1, M2, S, seed=0, aux=True)
        out[kind] = dict(host=record_host(N_SCENES, 0, kind), again=record_host(N_SCENES, 1, kind), rest=rest, aux=aux[code])
    return out


# ---- distribution ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_draws_the_host_generators_distribution(kind, samples):
    """2000 scenes per kind at M1 = 40, M2 = 16, S = 8: the statistics of tests/test_scene_gen_host.py plus the live task and
    free tables, the share of zero-height tables, the shares of the three merged states and the least pairwise object
    clearance, each within five standard errors of the host generator's own sample; the host at a second seed is the control."""
    smp = samples[kind]
    extra = [{}, {}, {}]
    if kind == "tabletop_reference":
        for e, recs in zip(extra, (smp["host"][1], smp["again"][1])):
            e["clearance"] = [least_clearance(r["objects"]) for r in recs]
        extra[2]["clearance"] = [least_clearance(objects_of(smp["aux"], b)) for b in range(N_SCENES)]
    if kind == "merged_cubby":
        extra[0]["merge_state"], extra[1]["merge_state"] = merge_state_of_arrays(smp["host"][0]), merge_state_of_arrays(smp["again"][0])
        extra[2]["merge_state"] = merge_state_of_arrays(smp["rest"])
        assert np.array_equal(extra[2]["merge_state"], smp["aux"]["no_shelf"] + 2 * smp["aux"]["no_wall"])
    host = new_statistics(smp["host"][0], kind, **extra[0])
    again = new_statistics(smp["again"][0], kind, **extra[1])
    rest = new_statistics(smp["rest"], kind, **extra[2])
    z_self = _compare(host, again, f"{kind}, host seed 1 against host seed 0")
    z = _compare(host, rest, f"{kind}, restatement against host")
    print(f"{kind}: largest deviation {z:.2f} standard errors (the host against itself: {z_self:.2f})")


RANGES = {"height": (0, 0.4), "front_x_min": (0.275, 0.375), "front_x_max": (1.275, 1.375), "front_y_max": (1.5, 1.65),
          "front_task_scalar": (0.55, 0.65), "side_y_max": (-0.325, -0.275), "side_length": (0, 1.375),
          "side_task_scalar": (0.55, 0.65), "mount_x": (-0.02, 0.02), "mount_y": (-0.02, 0.02), "mount_dim_y": (0.9, 0.94),
          "left": (0.6, 0.8), "right": (-0.8, -0.6), "bottom": (0.1, 0.3), "front": (0.45, 0.65), "top": (0.6, 0.8),
          "mid_h_z": (0.35, 0.55), "mid_v_y": (-0.1, 0.1), "thickness": (0.01, 0.03), "rotation": (-np.pi / 18, np.pi / 18)}
REST_NAMES = {"h": "height", "fx0": "front_x_min", "fx1": "front_x_max", "fy1": "front_y_max", "scalar": "front_task_scalar",
              "sy1": "side_y_max", "L": "side_length", "scalar_side": "side_task_scalar", "mcx": "mount_x", "mcy": "mount_y",
              "mdy": "mount_dim_y", "mz": "mid_h_z", "my": "mid_v_y", "t": "thickness", "yaw": "rotation"}
EPS = 1e-7  # (the restatement's bounds are float32 constants: 0.6f is 2.4e-8 above 0.6)


def test_every_parameter_lies_inside_its_range(samples):
    for kind in KINDS:
        for rec in samples[kind]["host"][1]:
            p = rec["params"]
            for name, (lo, hi) in RANGES.items():
                assert name not in p or lo <= p[name] <= hi, (kind, name, p[name])
            if "front_y_min" in p:
                lo, hi = (-1.0, -0.75) if p["has_side_table"] else (-0.75, -0.55)
                assert lo <= p["front_y_min"] <= hi
            if "back" in p:
                assert 0.15 <= p["back"] - p["front"] <= 0.55
        params = samples[kind]["aux"]["params"]
        for short, v in params.items():
            lo, hi = RANGES[REST_NAMES.get(short, short)] if REST_NAMES.get(short, short) in RANGES else (None, None)
            if lo is not None:
                assert (v >= lo - EPS).all() and (v <= hi + EPS).all(), (kind, short)
    tab = samples["tabletop_reference"]["aux"]
    fy0, side = tab["params"]["fy0"], tab["side"]
    assert (fy0[side] >= -1 - EPS).all() and (fy0[side] <= -0.75 + EPS).all()
    assert (fy0[~side] >= -0.75 - EPS).all() and (fy0[~side] <= -0.55 + EPS).all()
    cub = samples["cubby_reference"]["aux"]["params"]
    assert ((cub["back"] - cub["front"]) >= 0.15 - EPS).all() and ((cub["back"] - cub["front"]) <= 0.55 + EPS).all()
    assert ((tab["K"] >= 3) & (tab["K"] <= 14)).all() and set(np.unique(tab["K"])) == set(range(3, 15))


def test_placement_keeps_the_clearance_and_bounds_the_footprint(samples):
    """Both sources: a placed object's centre is more than 0.05 from the footprint of every object placed before it, its
    footprint dims (a cylinder's radius) do not exceed min(clearance, 0.15), nothing is below 0.05, at most K stand."""
    smp = samples["tabletop_reference"]
    aux = smp["aux"]
    sets = [(r["objects"], [min(m, 0.15) for m in r["clearances"]], r["K"]) for r in smp["host"][1]]
    sets += [(objects_of(aux, b), aux["clearance"][b, :aux["placed"][b]], aux["K"][b]) for b in range(N_SCENES)]
    full = 0
    for objects, clearance, K in sets:
        assert len(objects) <= K and len(clearance) == len(objects)
        full += len(objects) == K
        assert least_clearance(objects) > 0.05
        for o, xm in zip(objects, clearance):
            foot = o[3:4] if o[0] == "cylinder" else o[3:5]
            assert all(0.05 - EPS <= v <= xm + EPS for v in foot), (o, xm)
    assert full > 0.9 * len(sets)  # (ten candidates per object: nearly every scene places all K)
    for rec in smp["host"][1]:
        assert rec["points"] == 10 * rec["K"] and rec["accepted"] == sorted(set(rec["accepted"]))


# ---- structure ---------------------------------------------------------------------------------------------------------------
SHAPES = [(7, 0, 1), (8, 2, 4), (16, 16, 8), (64, 64, 64)]
PAD_BOX = [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]


def check_structure(scn, kind, m1, m2, s, weight_rtol=0.0):
    """What the contract promises of every output, whoever computed it (the GPU test runs this on the kernel's arrays).
    ``weight_rtol``: the host computes a surface's weight in float64 and rounds it; the device's is the float32 product."""
    kind = np.asarray(kind)
    own = np.isin(kind, (3, 4, 5))
    scn = {k: np.asarray(v)[own] for k, v in scn.items()}
    kind = kind[own]
    cub, cyl, sup = fsr.live_rows(scn)
    for live, keys in ((cub, ("cuboid_centers", "cuboid_dims", "cuboid_quats")),
                       (cyl, ("cylinder_centers", "cylinder_radii", "cylinder_heights", "cylinder_quats"))):
        assert (np.diff(live.astype(int), axis=1) <= 0).all()  # (a prefix)
        for key in keys:
            assert (scn[key][~live] == ([1, 0, 0, 0] if key.endswith("quats") else 0)).all(), key
    assert (scn["cylinder_quats"] == [1, 0, 0, 0]).all() and (scn["cuboid_quats"][..., 1:3] == 0).all()
    assert (scn["cuboid_dims"][cub] > 0).all()  # (a removed plate leaves no row with a zero dim behind)
    t, c, m = kind == 3, kind == 4, kind == 5
    assert (cub[t].sum(1) >= 3).all() and (cub[t].sum(1) <= min(m1, 5 + 14)).all() and (cyl[t].sum(1) <= min(m2, 14)).all()
    assert (cub[c].sum(1) == 7).all() and np.isin(cub[m].sum(1), (5, 6, 7)).all() and not cyl[c | m].any()
    if sup is not None:
        boxes = scn["support_boxes"]
        assert (np.diff(sup.astype(int), axis=1) <= 0).all() and (boxes[~sup] == PAD_BOX).all()
        assert (boxes[sup][:, 3:6] > 0).all() and (boxes[sup][:, 11] > 0).all() and (boxes[..., 7:9] == 0).all()
        assert (boxes[..., 10] == 0).all()
        assert (scn["support_kind"][t][sup[t]] == fsr.SURFACE).all() and (scn["support_kind"][c | m][sup[c | m]] == fsr.VOLUME).all()
        assert (sup[c].sum(1) == min(4, s)).all() and ((sup[t].sum(1) >= 1) & (sup[t].sum(1) <= min(2, s))).all()
        want = np.select([cub[m].sum(1) == 7, cub[m].sum(1) == 6], [4, 2], 1)
        assert (sup[m].sum(1) == np.minimum(want, s)).all()
        # a surface copies its table: rows 0 (and 1) of the cuboids, weight = the top face's area
        for r in range(min(2, s)):
            rows = np.flatnonzero(t)[sup[t][:, r]]
            assert np.array_equal(boxes[rows, r, :6], np.concatenate([scn["cuboid_centers"][rows, r], scn["cuboid_dims"][rows, r]], -1))
            assert np.allclose(boxes[rows, r, 11], boxes[rows, r, 3] * boxes[rows, r, 4], rtol=weight_rtol, atol=0)


@pytest.mark.parametrize("m1,m2,s", SHAPES)
def test_restatement_structure(m1, m2, s):
    B = 300
    ids = np.arange(B) + 11
    kind = 3 + ids % 3
    scn, aux = fsr.generate(kind, ids, m1, m2, s, seed=5, aux=True)
    assert np.isfinite(np.concatenate([np.ravel(v) for v in scn.values()])).all()
    check_structure(scn, kind, m1, m2, s)
    cub, cyl, sup = fsr.live_rows(scn)
    t = kind == 3
    if m1 <= 8:  # the overflow paths are taken: full cuboid rows, full (or absent) cylinder rows, fewer than K placed
        assert (cub[t].sum(1) == m1).any() and (m2 == 0 or (cyl[t].sum(1) == m2).any())
        assert (aux[3]["placed"] < aux[3]["K"]).any()
    # tables are solid blocks from z = -0.02; the mount table's top is the floor
    T = np.where(aux[3]["side"], 5, 3)
    rows = np.flatnonzero(t)
    for b, n in zip(rows, T):
        bottom = scn["cuboid_centers"][b, :n, 2] - scn["cuboid_dims"][b, :n, 2] / 2
        assert np.allclose(bottom, -0.02, atol=1e-7) and (scn["cuboid_quats"][b, :n] == [1, 0, 0, 0]).all()
        assert abs(scn["cuboid_centers"][b, n - 1, 2] + scn["cuboid_dims"][b, n - 1, 2] / 2) < 1e-7
    # kinds 4 and 5 of one id are the same cubby: the five fixed plates agree
    both = fsr.generate(np.r_[np.full(20, 4), np.full(20, 5)], np.r_[np.arange(20), np.arange(20)], m1, m2, s, seed=5)
    for key in ("cuboid_centers", "cuboid_dims", "cuboid_quats"):
        assert np.array_equal(both[key][:20, :5], both[key][20:, :5])
    # scenes depend on their own id alone; other kinds' rows are untouched
    again = fsr.generate(kind[::-1], ids[::-1], m1, m2, s, seed=5)
    assert all(np.array_equal(again[k][::-1], scn[k]) for k in scn)
    mixed = fsr.generate(ids % 6, ids, m1, m2, s, seed=5)
    assert np.isnan(mixed["cuboid_dims"][ids % 6 < 3]).all() and not np.isnan(mixed["cuboid_dims"][ids % 6 >= 3]).any()


def test_merge_pairs_and_support_map():
    """All twelve ordered pairs on one cubby: which plates go, which supports stand, and the pocket -> support map; (-1, -1)
    and every bad pair leave it unmerged (the device's stated rule); the host refuses a bad pair."""
    ids = np.full(1, 9)
    plain = fsr.generate([4], ids, 8, 0, 8, seed=2)
    for a in range(4):
        for b in range(4):
            got = fsr.generate([5], ids, 8, 0, 8, seed=2, merge_pockets=[[a, b]])
            if a == b:
                assert all(np.array_equal(got[k], plain[k]) for k in got)
                continue
            no_shelf, no_wall = (a >> 1) != (b >> 1), (a & 1) != (b & 1)
            live = (got["cuboid_dims"][0] != 0).any(-1)
            assert live.sum() == 7 - no_shelf - no_wall and np.array_equal(got["cuboid_dims"][0, :5], plain["cuboid_dims"][0, :5])
            if no_wall and not no_shelf:  # the shelf moved up into row 5
                assert np.array_equal(got["cuboid_dims"][0, 5], plain["cuboid_dims"][0, 6])
            sa, sb = fsr.merged_support(a, a, b), fsr.merged_support(b, a, b)
            assert sa == sb  # start and goal end in ONE support
            box = got["support_boxes"][0, sa]
            for p in (a, b):  # ... which contains both original pockets (in the cubby's frame: one shared yaw)
                old = plain["support_boxes"][0, p]
                yaw = 2 * np.arctan2(box[9], box[6])
                R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
                assert ((old[:3] - box[:3]) @ R - old[3:6] / 2 >= -box[3:6] / 2 - 1e-12).all()
                assert ((old[:3] - box[:3]) @ R + old[3:6] / 2 <= box[3:6] / 2 + 1e-12).all()
            host = scenes.merged_cubby_parameters(scenes._cubby_reference_parameters(np.random.default_rng(0)), (a, b))
            assert scenes.merged_support_index(a, host) == sa and scenes.merged_support_index(b, host) == sb
    for bad in ([-1, -1], [0, 4], [-1, 2], [7, 7], [2, 2]):
        got = fsr.generate([5], ids, 8, 0, 8, seed=2, merge_pockets=[bad])
        assert all(np.array_equal(got[k], plain[k]) for k in got)
        if bad != [-1, -1]:
            with pytest.raises(ValueError, match="merge_pockets"):
                scenes.make_task_scenes(1, 0, ("merged_cubby",), 8, 0, 8, merge_pockets=[bad])
            with pytest.raises(ValueError, match="merge_pockets"):
                scenes.make_scenes_device(1, 0, ("merged_cubby",), 8, 0, device="cpu", merge_pockets=[bad])


def test_host_generators_structure_and_stream():
    """The host arrays keep the structure too; the old kinds' scenes do not move when new kinds exist (their generators and
    their rng stream are as they were: tests/golden pins them, this pins the dispatch)."""
    for m1, m2, s in SHAPES:
        scn = scenes.make_task_scenes(60, 3, KINDS, m1, m2, s)
        check_structure(scn, 3 + np.arange(60) % 3, m1, m2, s, weight_rtol=3e-7)
    given = scenes.make_task_scenes(4, 3, ("merged_cubby",), 8, 0, 8, merge_pockets=[[0, 1], [0, 2], [0, 3], [-1, -1]])
    assert ((given["cuboid_dims"] != 0).any(-1).sum(1) == [6, 6, 5, 7]).all()
    assert ((given["support_kind"] != 0).sum(1) == [2, 2, 1, 4]).all()
    plain = scenes.make_task_scenes(4, 3, ("cubby_reference",), 8, 0, 8)
    assert np.array_equal(plain["cuboid_dims"][:, :5], given["cuboid_dims"][:, :5])  # (the same cubbies: the pair costs no draw)
    with pytest.raises(AssertionError, match="M1 >= 7"):
        scenes.make_scenes(1, 0, ("cubby_reference",), 6, 0)
    assert scenes.SCENE_KIND_CODES == {"tabletop": 0, "cubby": 1, "dresser": 2, "tabletop_reference": 3, "cubby_reference": 4,
                                       "merged_cubby": 5}


# ---- the library, without a GPU -------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_operands_without_gpu():
    from mpinets_amd import _lib

    lib = _lib.load()
    assert lib.mpx_version() == 341
    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched

    def call(B=4, m1=16, m2=16, s=8, offset=0, boxes=one, kinds=one, pockets=None):
        return lib.mpx_scene_generate_reference(one, None, pockets, B, m1, m2, s, 0, offset, one, one, one, one, one, one, one,
                                                boxes, kinds, None)

    for kw, text in ((dict(m1=6), b"M1 = 6"), (dict(m1=3), b"M1 = 3"), (dict(m1=65), b"M1 = 65"), (dict(m2=65), b"M2 = 65"),
                     (dict(m2=-1), b"M2 = -1"), (dict(s=65), b"S = 65"), (dict(boxes=None), b"go together"),
                     (dict(kinds=None), b"go together"), (dict(s=8, boxes=None, kinds=None), b"without support arrays"),
                     (dict(offset=-1), b"scene_offset is negative"), (dict(offset=(1 << 32) - 3), b"exceeds 2^32"),
                     (dict(B=-1), b"negative size")):
        assert call(**kw) != 0, kw
        assert text in lib.mpx_last_error() and b"mpx_scene_generate_reference" in lib.mpx_last_error(), (kw, lib.mpx_last_error())
    none = [None] * 9
    assert lib.mpx_scene_generate_reference(None, None, None, 0, 16, 16, 0, 0, 0, *none, None) == 0
    assert lib.mpx_scene_generate_reference(None, None, None, 4, 16, 16, 0, 0, 0, one, one, one, one, one, one, one, None, None, None) != 0
    assert b"NULL operand" in lib.mpx_last_error()
    assert lib.mpx_scene_generate_reference(one, None, None, 4, 16, 16, 0, 0, 0, one, one, one, None, one, one, one, None, None, None) != 0
    assert b"NULL output" in lib.mpx_last_error()
    assert "mpx_scene_generate_reference" in _lib.PROTOTYPES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpinets_hip.h")).read()
    assert "int mpx_scene_generate_reference(const int32_t *scene_kind, const int64_t *scene_ids, const int32_t *merge_pockets" in header


# ---- make_problem_batch ----------------------------------------------------------------------------------------------------------
def test_problem_batch_accepts_the_new_kinds_and_refuses_what_it_cannot_do(monkeypatch):
    with pytest.raises(ValueError, match="kinds must be among"):
        scenes.make_problem_batch(2, device="cpu", kinds=("tabletop", "shelf"))
    with pytest.raises(ValueError, match="M1 >= 7"):
        scenes.make_problem_batch(2, device="cpu", kinds=("cubby_reference",), M1=6)
    for kw in (dict(), dict(scene_source="host", device_clouds=True), dict(scene_source="device"),
               dict(scene_source="device", device_clouds=False)):
        with pytest.raises(ValueError, match="PER ROW|device_clouds=True"):
            scenes.make_problem_batch(2, device="cpu", kinds=KINDS, problems="task", collision_free=True, **kw)
    with pytest.raises(ValueError, match="PER ROW"):
        scenes.make_problem_batch(2, device="cpu", kinds=("merged_cubby",), problems="task", collision_free=True, device_clouds=True)

    class Reached(Exception):
        pass

    seen = {}

    def device_source(B, seed, kinds, m1, m2, S=None, device=None, scene_ids=None, merge_pockets=None, **k):
        seen.update(B=B, S=S, kinds=tuple(kinds), ids=scene_ids.tolist(), pockets=None if merge_pockets is None else merge_pockets.tolist())
        raise Reached

    def host_source(B, seed, kinds, m1, m2, *a, **k):
        seen.update(B=B, kinds=tuple(kinds), host=True)
        raise Reached

    monkeypatch.setattr(scenes, "make_scenes_device", device_source)
    monkeypatch.setattr(scenes, "make_scenes", host_source)
    monkeypatch.setattr(scenes, "make_task_scenes", host_source)
    with pytest.raises(Reached):  # the per-row merge starts from UNMERGED scenes
        scenes.make_problem_batch(2, device="cpu", kinds=KINDS, problems="task", collision_free=True, scene_source="device",
                                  device_clouds=True, env_offset=4)
    assert seen == dict(B=2, S=8, kinds=KINDS, ids=[4, 5], pockets=[[-1, -1], [-1, -1]])
    with pytest.raises(Reached):  # uniform problems: a merged cubby draws its pair
        scenes.make_problem_batch(2, device="cpu", kinds=KINDS, scene_source="device", device_clouds=True)
    assert seen["pockets"] is None and seen["S"] is None
    seen.clear()
    for kw in (dict(), dict(problems="task", collision_free=True, kinds=("tabletop_reference", "cubby_reference"))):
        with pytest.raises(Reached):  # the host source takes them too
            scenes.make_problem_batch(2, device="cpu", **dict(dict(kinds=KINDS), **kw))
        assert seen["host"]


def test_old_kinds_still_equal_the_golden_problem_batch():
    """``make_problem_batch``'s defaults and the old kinds' host scenes are bit for bit what tests/golden pins."""
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "problem_batch_default.npz"))
    keys = [k for k in golden.files if k in fsr.PRIMITIVE_KEYS]
    assert keys
    B = golden[keys[0]].shape[0]
    m1, m2 = golden["cuboid_dims"].shape[1], golden["cylinder_radii"].shape[1]
    scn = scenes.make_scenes(B, 0, ("tabletop",), m1, m2)
    for k in keys:
        assert np.array_equal(scn[k], golden[k]), k


# ---- fragile scenes ----------------------------------------------------------------------------------------------------------
def gpu_cases():
    """The tabletop scenes the GPU test compares exactly: (ids, M1, M2, S) of every launch, shared with that test."""
    cases = []
    for m1, m2, s in SHAPES:
        for B in (1, 5, 9):
            cases.append((3 + np.arange(B), m1, m2, s))
    cases.append(((1 << 32) - 9 + np.arange(9), 16, 16, 8))
    cases.append((np.array([40, 7, 123456789, 7, 0, 8, 41, 3, 9, 12], np.int64), 16, 16, 8))
    return cases


def fragile(aux):
    return aux["margin"] < FRAGILE_MARGIN


def test_fragile_scenes_are_rare():
    """The GPU test's seed, judged on the CPU from the restatement alone: of the tabletop scenes its launches compare, at most
    1 in 20 come within ``FRAGILE_MARGIN`` of a float decision.  Recorded: 0 of 32 at seed 20 (and 0 of 4000); and of 4000 fresh scenes at
    M1 = 40, M2 = 16 the share within the margin is printed (a float64 sketch put 0.08 % within 1e-5 m)."""
    total = left_out = 0
    for ids, m1, m2, s in gpu_cases():
        kind = 3 + ids % 3
        _, aux = fsr.generate(kind, ids, m1, m2, s, seed=GPU_SEED, aux=True)
        if 3 in aux:
            total += len(aux[3]["rows"])
            left_out += int(fragile(aux[3]).sum())
    _, aux = fsr.generate(np.full(4000, 3), np.arange(4000), M1, M2, S, seed=GPU_SEED, aux=True)
    share = fragile(aux[3]).mean()
    print(f"fragile tabletop scenes at seed {GPU_SEED}: {left_out} of {total} compared; {share:.4%} of 4000 fresh scenes")
    assert total >= 30 and left_out <= FRAGILE_CAP * total
    assert share <= FRAGILE_CAP
