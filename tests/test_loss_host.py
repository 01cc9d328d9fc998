"""CPU: the float64 restatement of the training-loss entries (tests/float64_loss.py) is right before any kernel is judged
by it -- against float64 autograd of the oracle's torch restatements, against the vectors the reference's loss.py made, the
joint mask per link -- and the inputs of tests/test_gpu_loss_float64.py (the same seeded builders) hold the leave-out caps."""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_loss as fl  # noqa: E402
import float64_plan as fp  # noqa: E402

from mpinets_amd import franka_tables as ft  # noqa: E402

LEAVE_OUT_CAP = 0.01
MIN_KEPT_PER_REGION = 8


def scene64(scene):
    t = lambda k: torch.from_numpy(scene[k]).double()
    return t("cub_frames"), t("cub_dims"), t("cyl_frames"), t("cyl_radii"), t("cyl_heights")


def autograd_hinge(oracle, pts, scene, margin):
    x = torch.from_numpy(pts).double().requires_grad_(True)
    B, N = pts.shape[:2]
    loss = oracle.collision_loss_torch(x, *scene64(scene), margin=float(np.float32(margin))) * (B * N)
    loss.backward()
    return float(loss.detach()), x.grad


@pytest.mark.parametrize("name", ["h1", "h3_masked", "h5_margin_0.1", "h3_no_cuboids"])
def test_hinge_equals_float64_autograd_of_the_oracle_on_the_kept_points(oracle, name):
    scn, pts, margin = fl.hinge_cases()[name]
    scene = fp.scene_from_arrays(scn)
    r = fl.hinge(pts, scene, margin)
    loss, grad = autograd_hinge(oracle, pts, scene, margin)
    assert abs(float(r["loss_sum"].sum()) - loss) < 1e-10 * max(loss, 1)
    keep = ~r["leave_out"]
    assert float((r["grad"] - grad)[keep].abs().max()) < 1e-12
    assert float((r["h"] > 0).double().mean()) > 0.3  # the comparison is about active hinges


def test_hinge_regions_equal_float64_autograd_where_the_frame_is_no_rotation(oracle):
    scene = fp.scene_from_arrays(fl.h2_scene())
    for b in range(4):
        f = scene["cub_frames"][b, 0] if b < 2 else scene["cyl_frames"][b, 0]
        assert fl.frame_defect(f) > 0.1, b
    pts, labels = fl.h2_case(scene)
    r = fl.hinge(pts, scene, fl.H2_MARGIN)
    _, grad = autograd_hinge(oracle, pts, scene, fl.H2_MARGIN)
    keep = torch.from_numpy(fl.h2_keep(labels, r["leave_out"].numpy()))
    # (on the axis autograd of the norm gives the zero radial part too, so the axis labels are compared as well)
    assert float((r["grad"] - grad)[keep].abs().max()) < 1e-12
    # the rolled frames' gradients are not unit vectors: M^T and M differ by more than a sign pattern
    norms = r["grad"][:4][keep[:4] & (r["h"][:4] > 0)].norm(dim=-1)
    assert float(norms.max()) > 1.05 or float(norms.min()) < 0.95


def test_hinge_takes_the_first_largest_at_an_exact_tie():
    scn, pts, want = fl.tie_case()
    for dtype in (torch.float64, torch.float32):
        r = fl.hinge(pts, fp.scene_from_arrays(scn), 0.03, dtype)
        assert r["leave_out"][0].all()  # every such point is ON a switch: the per-point comparisons leave them out
        assert np.array_equal(r["grad"].numpy(), want)


def test_hinge_matches_the_reference_vectors(loss_golden):
    g = loss_golden
    scn = {k: g["c_" + k] for k in fl.NAMES}
    r = fl.hinge(g["c_points"], fp.scene_from_arrays(scn), 0.03)
    B, N = g["c_points"].shape[:2]
    assert abs(float(r["loss_sum"].sum()) / (B * N) - float(g["c_loss"])) < 1e-6
    keep = (~r["leave_out"]).numpy()
    assert keep.mean() > 0.99
    scale = np.abs(g["c_grad"]).max()
    np.testing.assert_allclose((r["grad"].numpy() / (B * N))[keep], g["c_grad"][keep], atol=1e-5 * scale, rtol=1e-4)


def test_point_match_matches_the_reference_vectors_and_autograd(oracle, loss_golden):
    g = loss_golden
    a, t = g["p_input"].reshape(4, -1), g["p_target"].reshape(4, -1)
    w = 1.0 / a.size
    w32 = float(np.float32(w))
    sums, grad = fl.point_match(a, t, w, w)
    assert abs(float(sums.sum()) * w - float(g["p_loss"])) < 1e-7
    np.testing.assert_allclose(grad.numpy().reshape(g["p_grad"].shape), g["p_grad"], atol=1e-10, rtol=1e-5)
    x = torch.from_numpy(a).double().requires_grad_(True)
    oracle.point_match_loss_torch(x, torch.from_numpy(t).double()).backward()
    assert float((grad / (w32 / w) - x.grad).abs().max()) < 1e-15
    # unequal weights, and sign(0) = 0
    a2, t2 = fl.point_match_case(257)
    s2, g2 = fl.point_match(a2, t2, 0.0, 0.25)
    assert set(np.unique(g2.numpy())) == {-0.25, 0.0, 0.25} and ((g2 == 0).numpy() == (a2 == t2)).all()
    frac = (a2 == t2).mean()
    assert 0.002 < frac < 0.03
    s3, g3 = fl.point_match(a2, t2, 0.5, 0.0)
    np.testing.assert_allclose(g3.numpy(), a2.astype(np.float64) - t2, rtol=0, atol=0)
    np.testing.assert_allclose(s2.numpy(), s3.numpy(), rtol=0, atol=0)


@pytest.mark.parametrize("with_base_link", [False, True])
def test_cloud_grad_moves_each_link_with_its_upstream_joints_only(with_base_link):
    """Link L moves with joints 0 .. min(L, 7) - 1, link 0 with none; the fingers (9, 12, 13) with all seven."""
    q = fl.cloud_q()
    links = [l for l in fl.LINKS if l or with_base_link]
    pts, lnk = ft.link_point_table(4096, with_base_link)
    assert sorted(set(lnk.tolist())) == links
    for link in links:
        tp, tl, sub, g = fl.cloud_case(64, with_base_link, link=link)
        assert (tl[sub] == link).all()
        if link in (12, 13):
            own = np.nonzero(tl == link)[0]  # the fingertips own 7 or 8 rows each: all of them, repeated
            assert len(own) <= 8 and set(sub.tolist()) == set(own.tolist())
        gq, A = fl.cloud_grad(q, 0.025, tp, tl, sub, g)
        nj = min(link, 7)
        assert (gq[:, nj:] == 0).all() and (A[:, nj:] == 0).all(), link
        assert (gq[:, :nj].abs() > 1e-6).all() and (A[:, :nj] >= gq[:, :nj].abs()).all(), link


def test_cloud_grad_float32_restatement_is_within_its_own_scale():
    for group in fl.CLOUD_GROUPS:
        members, c32 = fl.cloud_group(group)
        assert 0 < 4 * c32 <= 64, (group, c32)
        for name, (case, _, gq, A) in members.items():
            assert gq.shape == A.shape == (4, 7) and ((A > 0).any() or case.n == 0 or case.link == 0), name


def test_leave_out_cap_holds_for_every_gpu_input():
    for name, (scn, pts, margin) in fl.hinge_cases().items():
        r = fl.hinge_pair(pts, fp.scene_from_arrays(scn), margin)
        assert r["left_out"] <= LEAVE_OUT_CAP, (name, r["left_out"])
        assert 4 * r["e32"] <= 1e-3, (name, r["e32"])  # (else: the inputs are too ill-conditioned to test anything)
        if pts.shape[1] >= 255:
            assert float((r["h"] > 0).double().mean()) > 0.2, name


def test_every_region_keeps_enough_points():
    scene = fp.scene_from_arrays(fl.h2_scene())
    pts, labels = fl.h2_case(scene)
    r = fl.hinge_pair(pts, scene, fl.H2_MARGIN)
    keep = fl.h2_keep(labels, r["leave_out"].numpy())
    assert (~keep).mean() <= LEAVE_OUT_CAP and 4 * r["e32"] <= 1e-3
    want = [fl.CUBOID_LABELS, fl.CUBOID_LABELS, fl.CYLINDER_LABELS, fl.CYLINDER_LABELS, fl.AXIS_LABELS]
    for b, names in enumerate(want):
        kept = Counter(lab for lab, k in zip(labels[b], keep[b]) if k)
        assert set(kept) - {"far"} == set(names), (b, set(names) ^ (set(kept) - {"far"}))
        assert min(kept[n] for n in names) >= MIN_KEPT_PER_REGION, (b, kept)
        active = (r["h"][b] > 0).numpy()
        assert all(active[j] for j, lab in enumerate(labels[b]) if lab != "far"), b
    # the axis points project back to rho == 0 exactly, in float64 and in the device's float32 statement order alike
    f = scene["cyl_frames"][4, 0]
    x = pts[4][[lab.startswith("axis_") for lab in labels[4]]]
    for dt in (np.float64, np.float32):
        p = ((f[:2, 0].astype(dt) * x[:, :1].astype(dt) + f[:2, 1].astype(dt) * x[:, 1:2].astype(dt))
             + f[:2, 2].astype(dt) * x[:, 2:3].astype(dt)) + f[:2, 3].astype(dt)
        assert (p == 0).all()
    g = r["grad"][4][[lab.startswith("axis_") for lab in labels[4]]]
    assert torch.isfinite(g).all() and (g[:, :2] == 0).all()
