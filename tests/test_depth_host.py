"""The depth camera without a GPU: the float64 restatement (tests/float64_depth.py) against closed forms and the engine
SDF, the figures the tolerances of tests/test_gpu_depth_float64.py are made of, the leave-out caps of every GPU input, the
camera-inside rule through the CPU oracle (the kernel's statements in the kernel's order), and the host refusals of both
entries.

Each test prints its measured figures (``FIGURE ...`` lines, shown with ``pytest -s``): profiles/depth_float64.md.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_depth as fd  # noqa: E402
import float64_loss as fl  # noqa: E402
import float64_plan as fp  # noqa: E402

GENERATED = ("r1_scenes", "r1_robot", "r7_clip_scene")
OUTSIDE = ("r1_scenes", "r4_cylinders", "r5_loose_frames", "r6_masked", "r10_overlap")  # the camera is outside everything


def figure(*a):
    print("FIGURE", *a)


def plane_depth(z, intr=fd.CRAFTED, W=fd.W0, H=fd.H0):
    """Depth along the pixel rays of the identity camera to the plane at distance z in front of it: z sqrt(1 + x^2 + y^2)."""
    fx, fy, cx, cy = intr
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    x, y = (u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy
    return (z * np.sqrt(1 + x * x + y * y)).reshape(-1), x.reshape(-1), y.reshape(-1)


# ---------------------------------------------------------------- the restatement itself
def test_restatement_equals_closed_forms():
    scn = fd.empty_scene(3, 1, 1)
    fd.put_box(scn, 0, 0, (0, 0, -3), (4, 2, 2))  # front plane at 2 m over the whole image
    fd.put_cyl(scn, 1, 0, (0, 0, -3), 3.0, 2.0)  # near cap at 2 m, axis along the view
    fd.put_box(scn, 2, 0, (0, 0, -5.5), (12, 8, 1))  # a plate at 5 m behind a sphere on the view axis
    sph = (np.asarray([[(9, 9, 9)], [(9, 9, 9)], [(0, 0, -2)]], np.float32), np.asarray([0.5], np.float32))
    r = fd.render_pair(fd.inputs(fd.case("closed", scn, spheres=sph)))
    want2, x, y = plane_depth(2.0)
    want5, _, _ = plane_depth(5.0)
    d = r["depth"].numpy()
    assert np.abs(d[0] - want2).max() < 1e-12 and np.abs(d[1] - want2).max() < 1e-12
    # a ray meets the ball iff its distance from the centre, D sin(angle to the axis), is below the radius
    sin2 = 1 - 1 / (1 + x * x + y * y)
    hidden = 4.0 * sin2 < 0.25
    assert 10 < hidden.sum() < 200
    assert np.array_equal(d[2] < 0, hidden) and np.abs(d[2] - want5)[~hidden].max() < 1e-12
    assert r["left_out"] == 0 and r["flips32"] == 0 and r["e32"] < 4e-6
    figure("closed_forms", f"e32={r['e32']:.3g}")


@pytest.mark.parametrize("name", OUTSIDE)
def test_restatement_hits_are_first_hits_of_the_engine_sdf(name, oracle):
    """Hit points have |sdf| at rounding level in float64, every point in front of a hit is outside every primitive, and an
    empty pixel's ray is never deep inside one (float32 oracle SDF, sampled every centimetre)."""
    c, r = fd.cases()[name], fd.reference(name)
    inp = fd.inputs(c)
    o, d = fd.rays(c["poses"], c["intr"], c["W"], c["H"])
    depth = r["depth"]
    valid = depth >= 0
    sdf = lambda s: fp.sdf_min_grad(o[:, None, :] + s[..., None] * d, inp["scene"])[0]
    on = sdf(depth.clamp(min=0))[valid].abs().max().item()
    figure(name, f"largest |sdf| of a hit point {on:.3g}")
    assert on < 1e-9
    for frac in (0.05, 0.3, 0.6, 0.9, 0.99, 0.9999):
        assert bool((sdf(frac * depth.clamp(min=0))[valid] > 0).all()), frac
    s = c["scn"]
    if s["cylinder_radii"].shape[1] == 0 or s["cuboid_dims"].shape[1] == 0:
        return
    miss = (~valid).numpy()
    for dist in np.arange(0.05, 6.0, 0.01):
        p = (o[:, None, :] + float(dist) * d).numpy().astype(np.float32)
        sd = np.minimum(oracle.cuboid_sdf(s["cuboid_centers"], s["cuboid_dims"], oracle.repair_quaternions(s["cuboid_quats"]), p),
                        oracle.cylinder_sdf(s["cylinder_centers"], s["cylinder_radii"], s["cylinder_heights"],
                                            oracle.repair_quaternions(s["cylinder_quats"]), p))
        assert (sd[miss] > -6e-3).all(), dist


# ---------------------------------------------------------------- figures and caps of every GPU input
@pytest.mark.parametrize("name", fd.RENDER_CASES)
def test_case_figures_caps_and_the_float32_oracle(name, oracle):
    c, r = fd.cases()[name], fd.reference(name)
    got = fd.oracle_render(c)
    flips, err = fd.judge(got, r)
    e32 = fd.group_e32(c["group"])
    kept_valid = int((r["keep"] & (r["depth"] >= 0)).sum())
    figure(name, f"B={r['depth'].shape[0]} pixels={r['depth'].shape[1]} margin={c['margin']:.3g} e32={e32:.3g} "
                 f"atol={4 * e32:.3g} left_out={r['left_out']:.4f} kept_valid={kept_valid} flips32={r['flips32']} "
                 f"oracle_flips={flips} oracle_err={err:.3g}")
    if c["capped"]:
        assert r["left_out"] <= fd.LEAVE_OUT_CAP
    if name in GENERATED:
        assert kept_valid >= 100
    assert flips == 0 and r["flips32"] == 0  # the margin is wide enough: no kept pixel changes sides in float32
    assert err <= 4 * e32  # (else the kernel's order of operations loses digits the restatement's keeps)


def test_crafted_cases_are_what_they_claim(oracle):
    cs = fd.cases()
    o, d = fd.rays(fd.IDENTITY[None], fd.CRAFTED, fd.W0, fd.H0, dtype=torch.float32)
    centre = (fd.H0 // 2) * fd.W0 + fd.W0 // 2
    assert d[0, centre].tolist() == [0.0, 0.0, -1.0]  # exactly parallel to four faces of an axis-aligned box
    # the cylinder across the view: an identity frame seen by a camera whose pose is an exact permutation, so the axial
    # component ez of the direction is exactly 0 on the whole centre row
    f = fd.inputs(cs["r4_cylinders"])["scene"]["cyl_frames"][1, 0]
    assert np.array_equal(f[:3, :3], np.eye(3)) and np.array_equal(cs["r4_cylinders"]["poses"][1], fd.POSE_SIDE)
    _, side = fd.rays(fd.POSE_SIDE[None], fd.CRAFTED, fd.W0, fd.H0, dtype=torch.float32)
    row = side[0, (fd.H0 // 2) * fd.W0:(fd.H0 // 2 + 1) * fd.W0]
    assert (row[:, 2] == 0).all() and (row[:, 0] < -0.7).all()
    # the frames of R5 are no rotations
    s = fd.inputs(cs["r5_loose_frames"])["scene"]
    for frame in (s["cub_frames"][0, 0], s["cyl_frames"][1, 0], s["cub_frames"][2, 0], s["cyl_frames"][2, 0]):
        assert fl.frame_defect(frame) > 0.1
    # the face-plane box: the centre column is flagged wherever the ray runs in the plane of the face, and hit there
    r = fd.reference("r3_face_plane")
    col = np.arange(fd.H0) * fd.W0 + fd.W0 // 2
    in_face = np.abs((np.arange(fd.H0) + 0.5 - fd.CRAFTED[3]) / fd.CRAFTED[1]) * 2.0 < 0.35
    assert r["leave_out"][0, col][in_face].all() and in_face.sum() == 7
    # R6: read as live, the masked rows would change the image; and the 2e-8 plate is seen
    c = cs["r6_masked"]
    thick = {k: v.copy() for k, v in c["scn"].items()}
    for k in ("cuboid_dims", "cylinder_radii", "cylinder_heights"):
        thick[k][np.abs(thick[k]) <= 1e-8] = 1e-3
    a, b = fd.reference("r6_masked")["depth"], fd.render_pair(fd.inputs(dict(c, scn=thick)))["depth"]
    assert float(((a - b).abs() > 0.1).double().mean()) > 0.1
    assert int(((a - 2.0).abs() < 0.2).sum()) >= 30  # the plate at 2 m
    assert (fd.reference("r6_nothing")["depth"] == -1).all()
    # R7: one plate is partly kept, the other clipped everywhere; the cut scene loses pixels to the clip
    r = fd.reference("r7_plates")
    x = np.tile(np.arange(fd.W0), fd.H0)
    assert (r["depth"][0, x < 15] > 9.99).all() and (r["depth"][0, x > 17] == -1).all()
    assert (r["obstacle"][0, x > 17] > 10.0).all() and 100 < int((r["depth"][1] >= 0).sum()) < 561
    r = fd.reference("r7_clip_scene")
    cut = (r["obstacle"] >= 1.0) & torch.isfinite(r["obstacle"])
    assert int(cut.sum()) > 300 and (r["depth"][cut] == -1).all() and float(r["depth"].max()) < 1.0
    # R8: what each sphere does
    c, r = cs["r8_robot"], fd.reference("r8_robot")
    bare = fd.render_pair(fd.inputs(dict(c, spheres=None)))["depth"]
    removed = (bare >= 0) & (r["depth"] < 0)
    assert 20 < int(removed.sum()) < 150 and bool(((r["depth"] == bare) | removed).all())
    for keep_only, lo, hi in ((0, 10, 200), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 5, 100)):
        sc, sr = c["spheres"]
        one = fd.render_pair(fd.inputs(dict(c, spheres=(sc[:, keep_only:keep_only + 1], sr[keep_only:keep_only + 1]))))
        n = int(((bare >= 0) & (one["depth"] < 0)).sum())
        assert lo <= n <= hi, (keep_only, n)
    # R10: both environments hold the same primitives in another order; the cylinder list wins some pixels, the cuboids others
    r = fd.reference("r10_overlap")
    assert torch.equal(r["depth"][0], r["depth"][1])
    scene = fd.inputs(cs["r10_overlap"])
    only = lambda fam: fd.render_pair(dict(scene, scene=dict(scene["scene"], **{k: v[:, :0] for k, v in scene["scene"].items()
                                                                             if k.startswith(fam)})))["depth"]
    cubs, cyls = only("cyl"), only("cub")  # (what is left after dropping the other family)
    both = (cubs >= 0) & (cyls >= 0)
    assert int((both & (cubs < cyls)).sum()) >= 10 and int((both & (cyls < cubs)).sum()) >= 10


# ---------------------------------------------------------------- the camera-inside rule
@pytest.mark.parametrize("env,what", [(0, "cuboid"), (1, "cylinder along the view"), (2, "cylinder across the view"),
                                      (3, "robot sphere")])
def test_a_primitive_that_contains_the_camera_is_invisible(env, what, oracle):
    """The oracle (the kernel's statements) and the restatement: the containing object contributes nothing, the plate
    behind it is seen at its own depth in every pixel."""
    c, r = fd.cases()["r9_inside"], fd.reference("r9_inside")
    want, _, _ = plane_depth(3.0)
    got = fd.oracle_render(c)[env]
    figure(f"r9_inside[{env}]", what, f"oracle: empty pixels {int((got < 0).sum())}, largest |depth - plate| "
                                      f"{np.abs(got - want).max():.3g}")
    assert np.abs(r["depth"][env].numpy() - want).max() < 1e-12
    assert (got >= 0).all() and np.abs(got - want).max() <= 4 * r["e32"]
    # the origin is inside, by the engine's own SDF
    scene = fd.inputs(c)["scene"]
    if env < 3:
        assert fp.sdf_min_grad(torch.zeros(4, 1, 3, dtype=torch.float64), {k: (v[:, 1:] if k.startswith("cub") else v)
                                                                            for k, v in scene.items()})[0][env, 0] < -0.05
    else:
        assert np.linalg.norm(c["spheres"][0][3, 0]) < c["spheres"][1][0] - 0.1


# ---------------------------------------------------------------- the subset draw
def test_select_restatement_equals_oracle_and_validity_rule(oracle):
    W, H, n_out, seed = 33, 17, 100, 77
    depth = fd.populations(W, H, (561, 100, 99, 300), 5)
    depth[3, :8] = (0.0, -0.0, float("nan"), -1.0, float("nan"), 0.0, -0.0, -1.0)
    poses = fd.tilted_poses(4, 1)
    intr = fd.intrinsics(W, H)
    count, rows = fd.select_pixels(depth, n_out, seed, env_offset=7)
    opts, ocount = oracle.depth_select(depth, poses, intr, W, H, n_out, seed, env_offset=7)
    assert np.array_equal(count, ocount) and count[:3].tolist() == [561, 100, 99] and rows[2] is None
    valid3 = depth[3] >= 0
    assert count[3] == valid3.sum() and valid3[:8].tolist() == [True, True, False, False, False, True, True, False]
    for b in (0, 1, 3):
        want = fd.back_project(depth[b:b + 1], poses[b:b + 1], intr, W, H, rows[b][None])[0].numpy()
        assert len(set(rows[b].tolist())) == n_out and (depth[b, rows[b]] >= 0).all()
        assert np.abs(opts[b] - want).max() < 2e-6, b
    assert (opts[2] == 0).all()


# ---------------------------------------------------------------- host refusals (before any launch)
def test_both_entries_refuse_bad_arguments_on_the_host():
    from mpinets_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(256)  # any non-NULL "device pointer": validation fails before it is touched

    def render(fx=1.0, far=10.0, B=1):
        return lib.mpx_depth_render(one, fx, 1.0, 0.0, 0.0, 4, 4, B, one, one, 1, one, one, one, 1, None, None, 0, far, one, None)

    assert render(far=0.0) != 0 and b"intrinsics" in lib.mpx_last_error()
    assert render(far=-1.0) != 0
    assert render(fx=0.0) != 0 and b"intrinsics" in lib.mpx_last_error()
    assert render(fx=-2.0) != 0
    assert render(B=65536) != 0 and b"bad size" in lib.mpx_last_error()
    assert render(B=0) == 0  # (nothing to do: no launch)

    def select(n_out=4, stride=3, count=one, env=0, B=1):
        return lib.mpx_depth_select(one, one, 1.0, 1.0, 0.0, 0.0, 4, 4, B, n_out, 0, env, one, 12, stride, count, None)

    assert select(n_out=0) != 0 and b"n_out" in lib.mpx_last_error()
    assert select(n_out=4097) != 0 and b"n_out" in lib.mpx_last_error()
    assert select(stride=2) != 0 and b"bad output" in lib.mpx_last_error()
    assert select(count=None) != 0 and b"bad output" in lib.mpx_last_error()
    assert select(env=0xFFFFFFFF, B=0) == 0
    assert select(env=0x100000000, B=0) != 0 and b"env_offset" in lib.mpx_last_error()
    assert select(env=0xFFFFFFFF, B=1) != 0 and b"env_offset" in lib.mpx_last_error()
