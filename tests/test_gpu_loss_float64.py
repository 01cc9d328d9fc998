"""The three training-loss entries of csrc/loss.hip against their float64 restatement (tests/float64_loss.py), per point,
per element and per joint, called through ``_lib.call`` so that strides, NULL arguments and the margin are the test's.

Every tolerance is computed from the restatement alone on the case's own inputs (float32 evaluation against float64
evaluation of the same statements, times 4 because the kernel's fma order is not torch's); tests/test_loss_host.py holds
the same inputs to the leave-out caps without a GPU.  ``mpx_collision_hinge`` is the one entry that exposes the obstacle
gradient of sdf_grad_device.h per point, so these are also the device tests of what both planners descend on.

Each test prints its measured figures (``FIGURE ...`` lines, shown with ``pytest -s``): profiles/loss_float64.md.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_loss as fl  # noqa: E402
import float64_plan as fp  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LEAVE_OUT_CAP = 0.01
EPS32 = fl.EPS32
SENTINEL = 12345.678


def figure(*a):
    print("FIGURE", *a)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


# ---------------------------------------------------------------- collision hinge
def device_scene(scn):
    """scn arrays -> the tensors the entry reads, frames made by the library's own TorchCuboids / TorchCylinders, and the
    same float32 arrays on the host in the restatement's layout."""
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in scn.items()}
    cub = TorchCuboids(t["cuboid_centers"], t["cuboid_dims"], t["cuboid_quats"])
    cyl = TorchCylinders(t["cylinder_centers"], t["cylinder_radii"], t["cylinder_heights"], t["cylinder_quats"])
    d = {"cub_frames": cub.inv_frames, "cub_dims": t["cuboid_dims"].contiguous(), "cyl_frames": cyl.inv_frames,
         "cyl_radii": t["cylinder_radii"][..., 0].contiguous(), "cyl_heights": t["cylinder_heights"][..., 0].contiguous()}
    return d, {k: v.cpu().numpy() for k, v in d.items()}


def launch_hinge(points, d, margin, grad="new"):
    """points: device tensor [B,N,3] (a view with unit last stride is fine) -> loss_sum [B], grad.  ``grad``: "new" (a
    contiguous NaN-filled buffer), None (NULL) or a [B,N,3] view to write into."""
    from mpinets_amd import _lib

    B, N = points.shape[:2]
    M1, M2 = d["cub_dims"].shape[1], d["cyl_radii"].shape[1]
    sums = torch.full((B,), float("nan"), device=DEV)
    if isinstance(grad, str):
        grad = torch.full((B, N, 3), float("nan"), device=DEV)
    pbs, pps = (points.stride(0), points.stride(1)) if N else (0, 3)
    gbs, gps = (grad.stride(0), grad.stride(1)) if grad is not None and N else (0, 3)
    assert points.stride(2) == 1 or N == 0
    _lib.call("mpx_collision_hinge", ptr(points), pbs, pps, B, N, ptr(d["cub_frames"]), ptr(d["cub_dims"]), M1,
              ptr(d["cyl_frames"]), ptr(d["cyl_radii"]), ptr(d["cyl_heights"]), M2, float(margin), sums.data_ptr(),
              ptr(grad), gbs, gps)
    torch.cuda.synchronize()
    return sums, grad


def judge_hinge(name, pts, host_scene, margin, loss, grad, labels=None):
    """Device results against the restatement evaluated around the device's own frames."""
    B, N = pts.shape[:2]
    r = fl.hinge_pair(pts, host_scene, margin)
    keep = r["keep"].numpy() if labels is None else fl.h2_keep(labels, r["leave_out"].numpy())
    left = float((~keep).mean()) if keep.size else 0.0
    assert left <= LEAVE_OUT_CAP, (name, left)
    atol = 4 * r["e32"]
    assert atol <= 1e-3, (name, atol)  # (else the inputs are too ill-conditioned to test anything)
    got_loss, want_loss = loss.double().cpu(), r["loss_sum"]
    bound = fl.loss_sum_bound(r, N)
    loss_err = (got_loss - want_loss).abs()
    err = (grad.double().cpu() - r["grad"]).abs().amax(-1).numpy() if N else np.zeros((B, 0))
    worst = float(err[keep].max()) if keep.any() else 0.0
    figure(name, f"B={B} N={N} margin={margin} e32={r['e32']:.3g} atol={atol:.3g} left_out={left:.4f} "
                 f"active={float((r['h'] > 0).double().mean()) if N else 0:.2f} grad_err={worst:.3g} "
                 f"loss_err={float(loss_err.max()):.3g} loss_bound={float(bound.min()):.3g}")
    per_region = ""
    if labels is not None:
        worst_of = {}
        for b in range(B):
            for j, lab in enumerate(labels[b]):
                if keep[b, j]:
                    key = f"{fl.H2_KINDS[b]}{b}:{lab}"
                    worst_of[key] = max(worst_of.get(key, 0.0), float(err[b, j]))
        per_region = " ".join(f"{k}={v:.2g}" for k, v in sorted(worst_of.items()))
        figure(name + "_regions", per_region)
    assert bool((loss_err <= bound).all()), (name, got_loss, want_loss, bound)
    assert torch.isfinite(grad).all()
    assert worst <= atol, (name, worst, atol, per_region)
    return r


def hinge_case(name):
    scn, pts, margin = fl.hinge_cases()[name]
    d, host = device_scene(scn)
    return scn, pts, margin, d, host, torch.from_numpy(pts).to(DEV)


def test_hinge_scenes_per_point_and_bit_equal_relaunch():
    """H1 and H7: six mixed scenes, 1500 points each (1500 = 5 x 256 + 220)."""
    _, pts, margin, d, host, p = hinge_case("h1")
    loss, grad = launch_hinge(p, d, margin)
    r = judge_hinge("h1", pts, host, margin, loss, grad)
    assert float(r["active"].double().mean()) / pts.shape[1] > 0.5
    loss2, grad2 = launch_hinge(p, d, margin)
    assert same_bits(loss, loss2) and same_bits(grad, grad2)
    # the library's frames are the oracle's to rounding: the host test's caps were about these inputs (judge_hinge
    # asserts them again around the device's frames)
    oracle_scene = fp.scene_from_arrays(fl.hinge_cases()["h1"][0])
    for k in ("cub_frames", "cyl_frames"):
        assert np.abs(host[k] - oracle_scene[k]).max() <= 1e-6, k


def test_hinge_regions_by_construction_in_frames_that_are_no_rotations():
    """H2: one live primitive per environment, every region of its gradient, the stored 3x3 block not orthonormal."""
    d, host = device_scene(fl.h2_scene())
    for b in range(4):
        f = host["cub_frames"][b, 0] if b < 2 else host["cyl_frames"][b, 0]
        assert fl.frame_defect(f) > 0.1, (b, fl.frame_defect(f))
    pts, labels = fl.h2_case(host)
    loss, grad = launch_hinge(torch.from_numpy(pts).to(DEV), d, fl.H2_MARGIN)
    r = judge_hinge("h2", pts, host, fl.H2_MARGIN, loss, grad, labels)
    want = [fl.CUBOID_LABELS, fl.CUBOID_LABELS, fl.CYLINDER_LABELS, fl.CYLINDER_LABELS, fl.AXIS_LABELS]
    keep = fl.h2_keep(labels, r["leave_out"].numpy())
    for b, names in enumerate(want):
        kept = [lab for lab, k in zip(labels[b], keep[b]) if k]
        assert all(kept.count(n) >= 8 for n in names), b
    # on the axis: a finite gradient with a zero radial part (the frame of environment 4 is axis aligned)
    on_axis = torch.tensor([lab.startswith("axis_") for lab in labels[4]])
    g = grad[4].cpu()[on_axis]
    assert on_axis.sum() >= 40 and torch.isfinite(g).all() and (g[:, :2] == 0).all()
    assert set(g[:, 2].abs().tolist()) == {0.0, 1.0}  # radially nearest inside: zero; else the axial unit step
    far = torch.tensor([[lab == "far" for lab in row] for row in labels])
    assert (bits(grad.cpu()[far]) == 0).all()


@pytest.mark.parametrize("B,N", fl.LAUNCH_EDGES)
def test_hinge_launch_edges(B, N):
    """H3: N below, at and above the 256-thread stride, one and several environments."""
    name = f"h3_B{B}_N{N}"
    _, pts, margin, d, host, p = hinge_case(name)
    loss, grad = launch_hinge(p, d, margin)
    judge_hinge(name, pts, host, margin, loss, grad)
    if N == 0:
        assert (bits(loss) == 0).all()


@pytest.mark.parametrize("name", ["h3_no_cuboids", "h3_no_cylinders", "h3_masked"])
def test_hinge_empty_and_masked_primitive_sets(name):
    """H3: M1 = 0 with cylinders, M2 = 0 with cuboids; zero-volume rows at index 0 and between live ones -- the gradient
    is that of the nearest LIVE primitive's own frame (the restatement filters the rows, the kernel indexes them all)."""
    scn, pts, margin, d, host, p = hinge_case(name)
    if name == "h3_no_cuboids":
        assert host["cub_dims"].shape[1] == 0 and (host["cyl_radii"] > 0).any()
    elif name == "h3_no_cylinders":
        assert host["cyl_radii"].shape[1] == 0
    else:
        dims = host["cub_dims"]
        assert (np.abs(dims[:, 0]) <= 1e-8).any(-1).all() and (np.abs(dims[:, 3]) <= 1e-8).any(-1).all()
        assert (np.abs(dims[:, 1]) > 1e-8).all() and (np.abs(dims[:, 4]) > 1e-8).all()
        assert (np.abs(host["cyl_radii"][:, 0]) <= 1e-8).all() and (host["cyl_heights"][:, 2] == 0).all()
        # read as live (1 mm thick), the masked rows would be the nearest primitive of some of the points
        unmasked = {k: v.copy() for k, v in host.items()}
        unmasked["cub_dims"][np.abs(unmasked["cub_dims"]) <= 1e-8] = 1e-3
        a, b = fl.hinge(pts, host, margin), fl.hinge(pts, unmasked, margin)
        assert float(((a["grad"] - b["grad"]).abs().amax(-1) > 0.1).double().mean()) > 0.01
    loss, grad = launch_hinge(p, d, margin)
    judge_hinge(name, pts, host, margin, loss, grad)


def test_hinge_without_any_primitive_is_exactly_zero():
    scn, pts, margin, _, _, p = hinge_case("h3_B3_N257")
    d, _ = device_scene(fl.only_cuboids(fl.only_cylinders(scn)))
    loss, grad = launch_hinge(p, d, margin)
    assert (bits(loss) == 0).all() and (bits(grad) == 0).all()


def test_hinge_cuboid_listed_twice_gives_the_bits_of_listing_it_once():
    scn, pts, margin, d, _, p = hinge_case("h3_B3_N257")
    once = launch_hinge(p, d, margin)
    for which in (0, 1):
        d2, _ = device_scene(fl.with_repeated_cuboid(scn, which))
        twice = launch_hinge(p, d2, margin)
        assert same_bits(once[0], twice[0]) and same_bits(once[1], twice[1]), which


def test_hinge_exact_tie_inside_takes_the_first_largest():
    """Two or three equal largest d inside a cube or a cylinder (exact by construction: axis-aligned frames at the origin):
    the gradient steps along the FIRST of them, as box_grad documents and the restatement does."""
    scn, pts, want = fl.tie_case()
    d, host = device_scene(scn)
    assert np.array_equal(host["cub_frames"][0, 0], np.eye(4)) and np.array_equal(host["cyl_frames"][1, 0], np.eye(4))
    _, grad = launch_hinge(torch.from_numpy(pts).to(DEV), d, 0.03)
    assert np.array_equal(fl.hinge(pts, host, 0.03)["grad"].numpy(), want)
    assert np.array_equal(grad.cpu().numpy().astype(np.float64), want)


def test_hinge_strides_and_null_gradient():
    """H4: points as a window of a [B,N+200,4] slab, the gradient into columns 1..3 of a [B,N,5] buffer."""
    _, pts, margin, d, host, p = hinge_case("h3_B3_N257")
    B, N = pts.shape[:2]
    loss, grad = launch_hinge(p, d, margin)
    judge_hinge("h4_contiguous", pts, host, margin, loss, grad)
    slab = torch.full((B, N + 200, 4), SENTINEL, device=DEV)
    slab[:, 100:100 + N, :3] = p
    before = slab.clone()
    buf = torch.full((B, N, 5), SENTINEL, device=DEV)
    loss_s, _ = launch_hinge(slab[:, 100:100 + N, :3], d, margin, grad=buf[:, :, 1:4])
    assert same_bits(slab, before)
    assert same_bits(loss_s, loss) and same_bits(buf[:, :, 1:4], grad)
    assert same_bits(buf[:, :, [0, 4]], torch.full((B, N, 2), SENTINEL, device=DEV))
    loss_n, none = launch_hinge(slab[:, 100:100 + N, :3], d, margin, grad=None)
    assert none is None and same_bits(loss_n, loss) and same_bits(slab, before)


@pytest.mark.parametrize("name", ["h5_margin_0", "h5_margin_0.1"])
def test_hinge_margins(name):
    """H5: rows with h <= 0 have the gradient +0.0 exactly."""
    _, pts, margin, d, host, p = hinge_case(name)
    loss, grad = launch_hinge(p, d, margin)
    r = judge_hinge(name, pts, host, margin, loss, grad)
    off = (r["sdf"] > float(np.float32(margin)) + fl.FRAGILE)
    assert 0.05 < float(off.double().mean()) < 0.95
    assert (bits(grad.cpu()[off]) == 0).all()


def test_hinge_rows_that_are_not_finite_take_no_part():
    """H6: a row with a NaN or infinite coordinate adds nothing to loss_sum and gets a zero gradient (the reference would
    return NaN); every other row is as in the call where a far point stands in its place (whose hinge is +0, so the fixed
    order of the sum is the same and the bits are)."""
    _, pts, margin, d, _, _ = hinge_case("h3_B3_N257")
    n, i = float("nan"), float("inf")
    bad = [(n, n, n), (n, 0.3, 0.2), (0.5, n, 0.2), (0.5, 0.1, n), (i, 0.1, 0.2), (-i, 0.1, 0.2), (0.5, i, 0.2),
           (0.5, 0.1, -i), (i, -i, i), (n, i, 0.0)]
    rows = [(0, 0), (0, 1), (0, 100), (0, 255), (0, 256), (1, 7), (1, 8), (1, 200), (2, 64), (2, 256)]
    with_bad, with_far = pts.copy(), pts.copy()
    for (b, j), v in zip(rows, bad):
        with_bad[b, j], with_far[b, j] = v, fl.FAR_POINT
    loss_f, grad_f = launch_hinge(torch.from_numpy(with_far).to(DEV), d, margin)
    loss_b, grad_b = launch_hinge(torch.from_numpy(with_bad).to(DEV), d, margin)
    is_bad = torch.zeros(pts.shape[:2], dtype=torch.bool)
    for b, j in rows:
        is_bad[b, j] = True
    figure("h6", f"loss with far rows {loss_f.tolist()} with non-finite rows {loss_b.tolist()} "
                 f"gradients of the non-finite rows {grad_b.cpu()[is_bad].tolist()}")
    assert (bits(grad_f.cpu()[is_bad]) == 0).all()  # the stand-ins are outside the margin
    assert same_bits(loss_b, loss_f)
    assert (grad_b.cpu()[is_bad] == 0).all()
    assert same_bits(grad_b.cpu()[~is_bad], grad_f.cpu()[~is_bad])


# ---------------------------------------------------------------- point match
def launch_point_match(a, t, w_sq, w_abs, want_grad=True):
    from mpinets_amd import _lib

    B, n = a.shape
    sums = torch.full((B, 2), float("nan"), device=DEV)
    grad = torch.full((B, n), float("nan"), device=DEV) if want_grad else None
    _lib.call("mpx_point_match", ptr(a), ptr(t), B, n, float(w_sq), float(w_abs), sums.data_ptr(), ptr(grad))
    torch.cuda.synchronize()
    return sums, grad


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3072, 3073])
def test_point_match_per_element(n):
    """P1: equal and unequal weights, exact zeros where input == target, NULL gradient."""
    a, t = fl.point_match_case(n)
    B = a.shape[0]
    ad, td = torch.from_numpy(a).to(DEV), torch.from_numpy(t).to(DEV)
    w = 1.0 / max(B * n, 1)
    equal = torch.from_numpy(a == t)
    if n >= 255:
        assert 0.002 < float(equal.double().mean()) < 0.03
    worst = 0.0
    for w_sq, w_abs in ((w, w), (0.0, w), (w, 0.0)):
        want_sums, want_grad = fl.point_match(a, t, w_sq, w_abs)
        sums, grad = launch_point_match(ad, td, w_sq, w_abs)
        tol_s = (math.ceil(n / 256) + 16) * EPS32 * want_sums
        assert bool(((sums.double().cpu() - want_sums).abs() <= tol_s).all()), (n, w_sq, w_abs, sums, want_sums)
        d = torch.from_numpy(a.astype(np.float64) - t)
        ws, wa = float(np.float32(w_sq)), float(np.float32(w_abs))
        tol_g = 4 * EPS32 * ((2 * ws * d).abs() + abs(wa))
        err = (grad.double().cpu() - want_grad).abs()
        assert bool((err <= tol_g).all()), (n, w_sq, w_abs, float((err - tol_g).max()))
        if n:
            worst = max(worst, float((err / tol_g.clamp(min=1e-300)).max()))
        assert (bits(grad.cpu()[equal]) == 0).all()
        if w_sq == 0.0:  # +-w or 0, bit for bit
            expect = torch.from_numpy((np.float32(w_abs) * np.sign(a - t)).astype(np.float32))
            assert same_bits(grad.cpu(), expect)
        sums_n, _ = launch_point_match(ad, td, w_sq, w_abs, want_grad=False)
        assert same_bits(sums_n, sums)
    if n == 0:
        assert (bits(sums) == 0).all()
    figure("p1", f"n={n} largest gradient error / tolerance {worst:.3g}")


# ---------------------------------------------------------------- robot-cloud backward
def launch_cloud_grad(q, finger, tp, tl, sub, g):
    from mpinets_amd import _lib

    B = q.shape[0]
    n = g.shape[1]
    gq = torch.full((B, 7), float("nan"), device=DEV)
    gbs, gps = (g.stride(0), g.stride(1)) if n else (0, 3)
    _lib.call("mpx_franka_cloud_grad", q.data_ptr(), B, float(finger), tp.data_ptr(), tl.data_ptr(), ptr(sub), n, ptr(g),
              gbs, gps, gq.data_ptr())
    torch.cuda.synchronize()
    return gq


def run_cloud_case(group, name):
    """One input of a group against the restatement; the tolerance is stated with the group's c32."""
    members, c32 = fl.cloud_group(group)
    case, (q, tp, tl, sub, g), want, A = members[name]
    dev = lambda x: None if x is None else torch.from_numpy(x).to(DEV)
    got = launch_cloud_grad(dev(q), case.finger, dev(tp), dev(tl), dev(sub), dev(g)).double().cpu()
    assert 4 * c32 <= 64, (group, c32)  # (else: find out why the float32 restatement is that far off)
    tol = 4 * c32 * EPS32 * A
    err = (got - want).abs()
    on = A > 0
    figure(name, f"n={case.n} c32={c32:.3g} largest error / (2^-24 A) = "
                 f"{float((err[on] / (EPS32 * A[on])).max()) if bool(on.any()) else 0:.3g} of {4 * c32:.3g} allowed")
    assert bool((err <= tol).all()), (name, err / (EPS32 * A.clamp(min=1e-300)), 4 * c32)
    return got, want, A, (q, tp, tl, sub, g)


@pytest.mark.parametrize("with_base_link", [False, True])
def test_cloud_grad_random_subset(with_base_link):
    """G1: B = 4 (one row of zeros, one on the limits), n = 1024 through a seeded subset."""
    got, want, A, (q, *_) = run_cloud_case("g1", f"g1_base{int(with_base_link)}")
    lim = fp.limits32(ft.JOINT_LIMITS_REAL)
    assert (q[1] == 0).all() and ((q[2] == lim[:, 0]) | (q[2] == lim[:, 1])).all()
    assert float(want.abs().min()) > 0


@pytest.mark.parametrize("link", fl.LINKS)
def test_cloud_grad_one_link_at_a_time(link):
    """G2: a subset of one link's rows; the joints at and after min(link, 7) get exactly 0.0."""
    got, want, A, (_, tp, tl, sub, _) = run_cloud_case("g2", f"g2_link{link}")
    assert (tl[sub] == link).all()
    nj = min(link, 7)
    assert (bits(got.float()[:, nj:]) == 0).all()
    assert (want[:, :nj].abs() > 0).all()


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_cloud_grad_launch_edges(n):
    """G3: n below and above the 256-thread stride."""
    got, *_ = run_cloud_case("g3", f"g3_n{n}")
    if n == 0:
        assert (bits(got.float()) == 0).all()


def test_cloud_grad_null_subset_and_repeats():
    """G3: subset = NULL walks the whole table; a subset may name a row more than once."""
    _, _, _, (_, _, _, sub, _) = run_cloud_case("g3", "g3_null_subset")
    assert sub is None
    _, _, _, (_, _, _, sub, _) = run_cloud_case("g3", "g3_repeats")
    assert len(set(sub.tolist())) <= 64


def test_cloud_grad_strided_gradient_is_bit_equal():
    """G4: g as columns 0..2 of a [B,n,4] buffer."""
    q = fl.cloud_q()
    tp, tl, sub, g = fl.cloud_case(1024, False)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    args = (dev(q), 0.025, dev(tp), dev(tl), dev(sub))
    plain = launch_cloud_grad(*args, dev(g))
    wide = torch.full((q.shape[0], 1024, 4), SENTINEL, device=DEV)
    wide[:, :, :3] = dev(g)
    assert same_bits(launch_cloud_grad(*args, wide[:, :, :3]), plain)
    assert wide.stride(1) == 4 and same_bits(wide[:, :, 3], torch.full(wide.shape[:2], SENTINEL, device=DEV))


@pytest.mark.parametrize("finger", [0.0, 0.025, 0.04])
def test_cloud_grad_finger_openings(finger):
    """G5: the finger opening moves the fingertip rows only: the usual subset, and the rows of a fingertip alone."""
    run_cloud_case("g5", f"g5_finger{finger}")
    got, want, *_ = run_cloud_case("g5", f"g5_finger{finger}_tips")
    if finger != 0.025:
        other = fl.cloud_group("g5")[0]["g5_finger0.025_tips"][2]
        assert float((want - other).abs().max()) > 1e-3  # the opening matters to these rows
