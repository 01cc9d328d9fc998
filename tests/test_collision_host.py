"""CPU: the cases of tests/test_gpu_collision_forms.py are sound before anything runs on a GPU -- the route query of
``mpx_franka_collision`` says they reach every launch form at both ends of its range, the float64 restatement agrees with
closed forms and with the C oracle, ``SDF_BAR`` can be derived again, and the restatement alone stays inside the undecided
cap on the seeds the GPU test uses."""
import numpy as np
import pytest

import float64_collision as fc


@pytest.fixture(scope="module")
def evaluated(oracle):
    """Per case: the CPU inputs and both runs of the restatement, computed once and left unchanged."""
    out = {}
    for case in fc.CASES:
        args, radii, scn = fc.cpu_inputs(case)
        out[case] = (args, radii, scn, fc.restate(*args, dtype=np.float64), fc.restate(*args, dtype=np.float32))
    return out


def _identity_frames(centres):
    f = np.tile(np.eye(4, dtype=np.float32), (1, len(centres), 1, 1))
    f[0, :, :3, 3] = -np.asarray(centres, np.float32)
    return f


def _one(points, cub=None, cyl=None, dtype=np.float64):
    """points [P,3] against axis-aligned primitives: cub = (centres [M,3], dims [M,3]), cyl = (centres, radii, heights)."""
    p = np.asarray(points, np.float32).reshape(1, 1, -1, 3)
    cc, cd = cub if cub else (np.zeros((1, 3)), np.zeros((1, 3)))
    yc, yr, yh = cyl if cyl else (np.zeros((1, 3)), np.zeros(1), np.zeros(1))
    return fc.restate(p, _identity_frames(cc), np.asarray(cd, np.float32)[None], _identity_frames(yc),
                      np.asarray(yr, np.float32)[None], np.asarray(yh, np.float32)[None], dtype=dtype)[0, 0]


def test_closed_forms_to_round_off():
    # every number below is a short binary fraction, so the float32 inputs are exact and float64 has bits to spare
    box = ([[0.5, -0.25, 1.0]], [[1.0, 0.5, 0.25]])  # x in [0, 1], y in [-0.5, 0], z in [0.875, 1.125]
    pts = [[1.75, -0.25, 1.0],      # on the +x face normal, 0.75 out
           [0.5, -0.25, 0.375],     # on the -z face normal, 0.5 below
           [1.375, 0.5, 1.625],     # off the (+,+,+) corner by (0.375, 0.5, 0.5)
           [0.5, -0.25, 1.0],       # the centre: the nearest face is z, 0.125 away
           [0.9375, -0.25, 1.0]]    # inside, 0.0625 from the +x face
    want = [0.75, 0.5, np.sqrt(0.375 ** 2 + 0.5 ** 2 + 0.5 ** 2), -0.125, -0.0625]
    np.testing.assert_allclose(_one(pts, cub=box), want, rtol=0, atol=1e-15)
    cyl = ([[0.25, 0.5, -0.5]], [0.5], [1.0])  # axis z through (0.25, 0.5), z in [-1, 0]
    pts = [[0.25 + 1.5, 0.5, -0.5],          # beside: rho 1.5
           [0.25 + 0.9, 0.5 + 1.2, -0.75],   # beside, off axis: rho 1.5 (a 3-4-5 triangle)
           [0.25, 0.5, 0.75],                # above the cap
           [0.25 + 0.8, 0.5 + 0.6, 0.375],   # off the rim: rho 1, 0.5 out and 0.375 up
           [0.25, 0.5, -0.5],                # the centre: radius and half height both 0.5 away
           [0.25 + 0.375, 0.5, -0.5],        # inside, 0.125 from the wall
           [0.25, 0.5, -0.0625]]             # inside, 0.0625 from the cap
    want = [1.0, 1.0, 0.75, np.sqrt(0.5 ** 2 + 0.375 ** 2), -0.5, -0.125, -0.0625]
    np.testing.assert_allclose(_one(pts, cyl=cyl), want, rtol=0, atol=1e-7)  # (0.9, 1.2, 0.8, 0.6 round as float32 inputs)
    np.testing.assert_allclose(_one(pts[2:3] + pts[4:], cyl=cyl), [0.75, -0.5, -0.125, -0.0625], rtol=0, atol=1e-15)
    # the minimum over both kinds, and the masks: any size |x| <= 1e-8 takes a primitive out; nothing live: +inf
    both = _one([[1.75, -0.25, 1.0]], cub=box, cyl=([[1.75, -0.25, 0.0]], [0.25], [1.5]))
    np.testing.assert_allclose(both, [0.25], rtol=0, atol=1e-15)  # the cylinder's cap is 0.25 below the point
    assert np.isposinf(_one([[0.3, 0.2, 0.1]], cub=([[0, 0, 0]], [[1.0, 1e-8, 1.0]]), cyl=([[0, 0, 0]], [1.0], [0.0]))).all()
    assert np.isfinite(_one([[0.3, 0.2, 0.1]], cub=([[0, 0, 0]], [[1.0, 2e-8, 1.0]]))).all()
    a = _one([[5.0, 0.0, 0.0]], cub=([[0, 0, 0], [4.5, 0, 0]], [[1.0, 1.0, 0.0], [0.5, 0.5, 0.5]]))
    np.testing.assert_allclose(a, [0.25], rtol=0, atol=1e-15)  # the masked box (nearer) does not count
    assert _one(pts, cyl=cyl, dtype=np.float32).dtype == np.float32


def test_cases_reach_every_route_at_both_ends_of_its_range():
    """``route`` is the launcher's own plan; over CASES it takes every value.  Every case runs in the full and in the
    flags-only form (the launcher does not look at ``min_sdf``), so both forms reach every route."""
    routes = {c: fc.case_route(c) for c in fc.CASES}
    for c, r in routes.items():
        print(fc.case_id(c), r)
    assert {r[0] for r in routes.values()} == set(fc.ROUTES)
    assert fc.FORMS == ("full", "flags_only")
    # an unaligned frame pointer sends every case to the general kernel (the bit-for-bit comparison of the GPU test)
    assert {fc.case_route(c, aligned=False)[0] for c in fc.CASES} == {"general"}
    env_block, col_tc = fc.env_form()
    assert (env_block, col_tc) == (256, 64)
    # S = 56 and S = 57: the lowest and the highest T of every form's range, found by walking the route query itself
    for S, table in ((56, "S56"), (57, "S57")):
        spans = {}
        for T in range(1, col_tc + 1):
            spans.setdefault(fc.route(2, T, S, 16, 16)[0], []).append(T)
        have = {(routes[c][0], c.T) for c in fc.CASES if c.table == table}
        for name, ts in spans.items():
            if S == 57 and name != "ppt16" and name != "wave":
                continue  # (the 57-sphere table is there for the 16-pairs form; 56 spheres cover the others)
            assert (name, ts[0]) in have and (name, ts[-1]) in have, (S, name, ts[0], ts[-1])
    assert fc.route(2, 62, 57, 16, 16)[0] == "ppt14" and fc.route(2, 63, 57, 16, 16)[0] == "ppt16"
    # each 256-thread form: once as a single chunk, once with a ragged last chunk of fewer than 256 pairs
    for p in range(2, 17, 2):
        mine = [r for r in routes.values() if r[0] == "ppt%d" % p]
        assert any(ch == 1 for _, ch, _ in mine), p
        assert any(ch > 1 and last < env_block for _, ch, last in mine), p
    # the shapes the issue names
    by_id = {fc.case_id(c): r for c, r in routes.items()}
    assert by_id["B3-T64-S64tile-M16x16"] == ("ppt16", 1, 16 * env_block)  # every thread 16 live pairs
    assert by_id["B4-T1-S64tile-M16x16"] == ("wave", 1, 64) and by_id["B3-T64-S1tile-M16x16"] == ("wave", 1, 64)
    assert by_id["B3-T65-S1tile-M16x16"] == ("ppt2", 2, 1)
    assert by_id["B3-T3-S65tile-M16x16"][0] == by_id["B3-T9-S56-M70x16"][0] == by_id["B2-T2-S56-M16x65"][0] == "general"
    assert by_id["B70-T50-S56-M40x16"] == ("ppt12", 1, 2800)
    # nothing to launch
    assert fc.route(0, 5, 56, 16, 16) is None and fc.route(3, 0, 56, 16, 16) is None and fc.route(3, 5, 0, 16, 16) is None


def test_scene_edges_are_what_they_claim(evaluated):
    case = next(c for c in fc.CASES if c.edge == "edges")
    args, radii, scn, ref64, _ = evaluated[case]
    live_c = ~(np.abs(scn["cuboid_dims"]) <= 1e-8).any(axis=2)
    live_y = ~((np.abs(scn["cylinder_radii"][..., 0]) <= 1e-8) | (np.abs(scn["cylinder_heights"][..., 0]) <= 1e-8))
    assert live_c[0].any() and not live_y[0].any() and (scn["cylinder_heights"][0] > 0).any()  # 0: no live cylinder
    assert not live_c[1].any() and live_y[1].all()                                               # 1: no live cuboid
    assert not live_c[2].any() and not live_y[2].any() and np.isposinf(ref64[2]).all()           # 2: nothing live
    assert live_c[3].sum() == 64 == case.M1                                                      # 3: exactly 64
    n = int(live_c[4].sum())                                                                     # 4: interleaved
    assert n >= 4 and not live_c[4, 0] and live_c[4, 1:2 * n:2].all() and not live_c[4, 0:2 * n:2].any()
    assert live_y[4, 1::2].all() and not live_y[4, 0::2].any()
    assert np.isfinite(ref64[[0, 1, 3, 4]]).all()
    hit, und = fc.decide(ref64, radii)
    assert not hit[2] and not und[2]


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_restatement_agrees_with_the_oracle(oracle, evaluated, case):
    args, radii, scn, ref64, ref32 = evaluated[case]
    oflags, omsdf = oracle.collision_flags(
        args[0], radii, (scn["cuboid_centers"], scn["cuboid_dims"], scn["cuboid_quats"]),
        (scn["cylinder_centers"], scn["cylinder_radii"], scn["cylinder_heights"], scn["cylinder_quats"]))
    bad, err = fc.offending_envs(omsdf, ref32)
    bad64, err64 = fc.offending_envs(omsdf, ref64)
    print(f"{fc.case_id(case)}: oracle vs restate32 {err:.2e}, vs restate64 {err64:.2e}, bar {fc.SDF_BAR:.1e}")
    assert not bad and not bad64
    hit, und = fc.decide(ref64, radii)
    assert np.array_equal(oflags[~und], hit[~und])


def test_sdf_bar_can_be_derived_again(evaluated):
    """Reference against reference: the bar is 4x the recorded gap; measured again it must lie between 2x and 8x of it."""
    gap = 0.0
    for case, (_, _, _, a, b) in evaluated.items():
        assert np.array_equal(np.isposinf(a), np.isposinf(b)) and not np.isnan(a).any()
        fin = np.isfinite(a)
        gap = max(gap, float(np.abs(a[fin] - b[fin].astype(np.float64)).max()) if fin.any() else 0.0)
    print(f"float32 vs float64 restatement: {gap:.3e}; recorded {fc.MEASURED_GAP:.3e}; SDF_BAR {fc.SDF_BAR:.3e}")
    assert fc.SDF_BAR == pytest.approx(4 * fc.MEASURED_GAP, rel=1e-2)
    assert 2.0 * gap <= fc.SDF_BAR <= 8.0 * gap
    assert gap == pytest.approx(fc.measure_reference_gap(fc.CASES[:3] + fc.CASES[-1:]), rel=1.0)  # (the helper runs)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_undecided_cap_holds_for_the_restatement_alone(evaluated, case):
    """With centres and frames from the oracle: the share of undecided environments of every GPU case is within the cap,
    so the GPU test's condition is satisfiable before anything runs on a GPU."""
    _, radii, _, ref64, _ = evaluated[case]
    hit, und = fc.decide(ref64, radii)
    print(f"{fc.case_id(case)}: {fc.case_route(case)}, hit {int(hit.sum())}/{case.B}, undecided {int(und.sum())}")
    assert und.mean() <= fc.UNDECIDED_CAP
    assert fc.UNDECIDED_CAP == 0.02


def test_cases_reach_both_outcomes_and_the_boundary_test_has_material(evaluated):
    hit = total = free = 0
    for case, (_, radii, _, ref64, _) in evaluated.items():
        h, _ = fc.decide(ref64, radii)
        hit, total = hit + int(h.sum()), total + case.B
        if fc.case_route(case)[0].startswith("ppt") and case.B <= 5:
            free += int((ref64.reshape(case.B, -1).min(axis=1) > 1e-3).sum())
    assert 0 < hit < total
    assert free >= 10  # environments with every distance > 1e-3 in the 256-thread forms


def test_comparator_sees_a_planted_row():
    """The sensitivity control of the GPU test, on the CPU: a chunk-tail row overwritten with its neighbour's values is
    flagged, in exactly that environment."""
    case = next(c for c in fc.CASES if fc.case_route(c)[1] > 1 and c.table == "S56")
    args, _, _ = fc.cpu_inputs(case)
    ref64 = fc.restate(*args)
    got = fc.restate(*args, dtype=np.float32)
    assert fc.offending_envs(got, ref64)[0] == set()
    got[1, case.T - 1] = got[1, case.T - 2]
    assert fc.offending_envs(got, ref64)[0] == {1}
    got[0, 0, 0] = np.inf
    assert fc.offending_envs(got, ref64)[0] == {0, 1}
