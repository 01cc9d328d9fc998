"""GPU: ``mpx_cloud_clean`` (csrc/cloud_clean.hip) through ``mpinets_amd.capture``: the four stages against their
float64 restatement, the exact edge of both radius tests, duplicates, a far-away row without a crop box, the draw
against the NumPy restatement of its keys, uniformity, layouts, the error path, the reference's signature, and the
capture -> clean -> slab -> policy / ``check_cloud`` chain.

Bands (tests/float64_cloud_clean.py): the device's squared distance is within ``BAND = 4 * 2^-24`` relative of the float64
one, so a row whose every test is outside the band must get exactly the restatement's reason, a row with a test inside
it may get either candidate, and at most 1 % of an environment's rows may be such rows
(tests/test_cloud_clean_host.py shows the restatement alone gives 0).  Everything else here is exact.
"""
import functools

import numpy as np
import pytest
import torch

import float64_cloud_clean as f64
from mpinets_amd import _lib
from mpinets_amd.capture import REFERENCE_WORKSPACE, clean_point_cloud, clean_point_clouds
from mpinets_amd.robot import FrankaCollisionSampler

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def sampler():
    return FrankaCollisionSampler(DEV, with_base_link=True)


def device_arguments(case):
    """-> (cloud tensor, keyword arguments of clean_point_clouds) of a case."""
    B, N, crop, robot, outlier, ragged, n_out = case
    data, kw = f64.make_case(case), dict(f64.case_arguments(case))
    if robot:
        kw["q"], kw["collision_sampler"] = torch.from_numpy(data["q"]).to(DEV), sampler()
    if ragged:
        kw["counts"] = torch.from_numpy(data["counts"]).to(DEV)
    return torch.from_numpy(data["cloud"]).to(DEV), kw


@functools.lru_cache(maxsize=None)
def run_case(case):
    """One filter-only device run plus the restatement from the device's own sphere centres, shared by the tests below
    (inputs and results are not modified)."""
    B, N, crop, robot, outlier, ragged, n_out = case
    cloud, kw = device_arguments(case)
    reason, count = clean_point_clouds(cloud, 0, **kw)
    centres = sampler().sphere_centers(kw["q"]).cpu().numpy() if robot else None
    return reason.cpu().numpy(), count.cpu().numpy(), f64.restate_case(case, centres)


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_stages_against_float64(case):
    B, N, crop, robot, outlier, ragged, n_out = case
    reason, count, ref = run_case(case)
    assert reason.shape == (B, N) and reason.dtype == np.uint8 and count.shape == (B,)
    for b in range(B):
        und = ref[b]["undecided"]
        ok = (ref[b]["allowed"] >> reason[b].astype(np.int64)) & 1
        print(f"{f64.case_id(case)} env {b}: kept {int(count[b])}, reasons {np.bincount(reason[b], minlength=5).tolist()}, "
              f"undecided {int(und.sum())}, wrong {int((ok == 0).sum())}")
        assert und.sum() <= f64.UNDECIDED_CAP * N
        assert (reason[b] <= 4).all() and ok.all(), np.flatnonzero(ok == 0)[:10]
        assert count[b] == (reason[b] == 0).sum()
    if ragged:
        for b, n in enumerate(f64.RAGGED[:B]):
            assert (reason[b, n:] == 1).all()


class OneSphere:
    """The three members ``clean_point_clouds`` uses of a collision sampler, for one sphere at a fixed place."""

    def __init__(self, centre, radius):
        self.centre = torch.tensor(centre, dtype=torch.float32, device=DEV)
        self.radii = torch.tensor([radius], dtype=torch.float32, device=DEV)
        self.num_spheres = 1

    def sphere_centers(self, q):
        return self.centre.expand(q.size(0), 1, 3).contiguous()


def lattice():
    """9 x 8 x 7 points at multiples of 2^-5 below 2 m, shuffled: every difference, square and sum is exact in float32."""
    g = np.stack(np.meshgrid(np.arange(9), np.arange(8), np.arange(7), indexing="ij"), -1).reshape(-1, 3)
    order = np.random.default_rng(0).permutation(len(g))
    g = g[order]
    pts = ((g + np.array([20, 3, 40])) * 2.0 ** -5).astype(np.float32)
    interior = ((g > 0) & (g < np.array([8, 7, 6]))).all(axis=1)
    return g, pts, interior


def test_exact_edge_of_the_neighbour_radius():
    """Every interior lattice point has exactly 6 neighbours, all at d2 == r^2: the test is <=, and the cell walk finds
    neighbours that sit exactly one radius away in the next cell."""
    g, pts, interior = lattice()
    cloud = torch.from_numpy(pts).to(DEV)[None]
    r6, c6 = clean_point_clouds(cloud, 0, boxes=None, outlier_radius=2.0 ** -5, min_neighbors=6)
    assert np.array_equal(r6[0].cpu().numpy() == 0, interior) and (r6[0].cpu().numpy()[~interior] == 4).all()
    assert int(c6[0]) == int(interior.sum()) == 7 * 6 * 5
    r7, c7 = clean_point_clouds(cloud, 0, boxes=None, outlier_radius=2.0 ** -5, min_neighbors=7)
    assert (r7 == 4).all() and int(c7[0]) == 0
    # 5 of the 6: faces keep their points, edges and corners do not
    on_faces = ((g == 0) | (g == np.array([8, 7, 6]))).sum(axis=1)
    r5, _ = clean_point_clouds(cloud, 0, boxes=None, outlier_radius=2.0 ** -5, min_neighbors=5)
    assert np.array_equal(r5[0].cpu().numpy() == 0, on_faces <= 1)


def test_exact_edge_of_the_robot_radius():
    """One sphere of radius 2^-4 centred on a lattice point: the 33 points with |offset|^2 <= 4 steps^2 are robot, the six
    at exactly two steps included."""
    g, pts, _ = lattice()
    centre = np.array([4, 4, 3])
    off2 = ((g - centre) ** 2).sum(axis=1)
    cloud = torch.from_numpy(pts).to(DEV)[None]
    one = OneSphere(((centre + np.array([20, 3, 40])) * 2.0 ** -5).tolist(), 2.0 ** -4)
    reason, count = clean_point_clouds(cloud, 0, boxes=None, q=torch.zeros(1, 7, device=DEV), collision_sampler=one)
    assert np.array_equal(reason[0].cpu().numpy() == 3, off2 <= 4) and int((off2 <= 4).sum()) == 33
    assert int((off2 == 4).sum()) == 6 and int(count[0]) == len(g) - 33
    # a margin of one more step: |offset|^2 <= 9
    reason, _ = clean_point_clouds(cloud, 0, boxes=None, q=torch.zeros(1, 7, device=DEV), collision_sampler=one,
                                   robot_margin=2.0 ** -5)
    assert np.array_equal(reason[0].cpu().numpy() == 3, off2 <= 9)


def test_duplicates_are_neighbours_of_each_other():
    cloud = torch.tensor([0.4, 0.1, 0.2], device=DEV).expand(1, 64, 3).contiguous()
    r, c = clean_point_clouds(cloud, 0, boxes=None, outlier_radius=0.01, min_neighbors=63)
    assert (r == 0).all() and int(c[0]) == 64
    r, c = clean_point_clouds(cloud, 0, boxes=None, outlier_radius=0.01, min_neighbors=64)
    assert (r == 4).all() and int(c[0]) == 0


def test_far_rows_without_a_crop_box_only_coarsen_the_cells():
    case = (1, 4097, False, False, True, False, 128)
    cloud, kw = device_arguments(case)
    base, _ = clean_point_clouds(cloud, 0, **kw)
    far = torch.tensor([[50.0, -30.0, 20.0], [1e6, 1e6, 1e6]], device=DEV)
    huge = torch.tensor([[3e38, -3e38, 3e38], [-3e38, 3e38, -3e38]], device=DEV)
    for rows in (far, huge):  # (the second: an extent that overflows float32 on every axis -- one cell, still right)
        both = torch.cat([cloud, rows[None]], dim=1)
        reason, count = clean_point_clouds(both, 0, **kw)
        assert torch.equal(reason[:, :4097], base)
        assert (reason[:, 4097:] == 4).all() and int(count[0]) == int((base == 0).sum())


DRAW_CASES = [c for c in f64.CASES if c[6] > 0]


@pytest.mark.parametrize("case", DRAW_CASES, ids=f64.case_id)
def test_draw_given_the_device_mask(case):
    B, N, crop, robot, outlier, ragged, n_out = case
    cloud, kw = device_arguments(case)
    seed, env = (0xC0FFEE << 32) | 12345, 7
    out, index, reason = clean_point_clouds(cloud, n_out, seed=seed, env_offset=env, return_index=True, return_reason=True, **kw)
    filter_only, count = run_case(case)[:2]
    assert np.array_equal(reason.cpu().numpy(), filter_only)  # the same mask with and without the draw
    assert np.array_equal(clean_point_clouds.last_counts.cpu().numpy(), count)
    assert out.shape == (B, n_out, 3) and index.shape == (B, n_out) and index.dtype == torch.int32
    idx = index.cpu().numpy()
    for b in range(B):
        want = f64.draw(filter_only[b] == 0, n_out, seed, env + b)
        assert np.array_equal(idx[b], want), (b, np.flatnonzero(idx[b] != want)[:5])
    gathered = torch.gather(cloud, 1, index.long()[..., None].expand(-1, -1, 3))
    assert torch.equal(out.view(torch.int32), gathered.view(torch.int32))  # bit for bit
    # another seed: another subset (not for the one-row draws of the smallest clouds)
    if n_out >= 128:
        other = clean_point_clouds(cloud, n_out, seed=seed + 1, env_offset=env, return_index=True, **kw)[1]
        assert not torch.equal(torch.sort(other, dim=1).values, torch.sort(index, dim=1).values)
    # row b of a batch at env_offset e == a one-environment call at e + b
    for b in range(B):
        kw1 = {k: (v[b:b + 1] if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        o1, i1 = clean_point_clouds(cloud[b:b + 1], n_out, seed=seed, env_offset=env + b, return_index=True, **kw1)
        assert torch.equal(i1[0], index[b]) and torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32))
    # two identical calls: identical bytes
    out2, index2, reason2 = clean_point_clouds(cloud, n_out, seed=seed, env_offset=env, return_index=True, return_reason=True, **kw)
    assert torch.equal(index2, index) and torch.equal(reason2, reason) and torch.equal(out2.view(torch.int32), out.view(torch.int32))
    assert np.array_equal(clean_point_clouds.last_counts.cpu().numpy(), count)


def test_draw_sizes_on_one_mask():
    """n_out in {1, 128, 4096} over the same survivors: each is the head of the same (key, row) order."""
    case = (1, 12289, False, False, False, False, 4096)
    cloud, kw = device_arguments(case)
    heads = [clean_point_clouds(cloud, n, seed=5, return_index=True, **kw)[1][0] for n in (1, 128, 4096)]
    assert torch.equal(heads[0], heads[2][:1]) and torch.equal(heads[1], heads[2][:128])
    assert len(set(heads[2].tolist())) == 4096


def test_draw_is_uniform_without_replacement():
    """As tests/test_gpu_depth.py does it: 40 seeds, 1000 of 1536 survivors; every survivor is chosen with probability
    1000 / 1536 (a binomial frequency over 40 draws has a spread of sqrt(p (1 - p) / 40) = 0.075)."""
    rng = np.random.default_rng(1)
    n, inside = 3072, np.zeros(3072, bool)
    inside[rng.permutation(3072)[:1536]] = True
    pts = rng.random((n, 3)).astype(np.float32) * 0.5 + np.where(inside, 0.0, 2.0)[:, None].astype(np.float32)
    cloud = torch.from_numpy(pts).to(DEV)[None]
    box = np.array([[-0.1, -0.1, -0.1, 0.6, 0.6, 0.6]], np.float32)
    seen = np.zeros(n, np.int64)
    for seed in range(40):
        _, index = clean_point_clouds(cloud, 1000, boxes=box, seed=seed, return_index=True)
        idx = index[0].cpu().numpy()
        assert len(set(idx.tolist())) == 1000 and inside[idx].all()
        seen[idx] += 1
    freq = seen[inside] / 40.0
    assert abs(freq.mean() - 1000 / 1536) < 1e-9 and freq.std() < 0.12


def test_layouts_four_columns_in_and_slab_rows_out():
    case = (3, 12289, True, True, True, False, 4096)
    cloud, kw = device_arguments(case)
    want, want_index = clean_point_clouds(cloud, 4096, seed=3, return_index=True, **kw)
    wide = torch.full((3, 12289, 4), float("nan"), device=DEV)
    wide[..., :3] = cloud
    xyz = torch.full((3, 6272, 4), -7.0, device=DEV)
    xyz[..., 3] = torch.arange(6272, device=DEV)
    before = xyz.clone()
    got, index = clean_point_clouds(wide[..., :3], 4096, seed=3, return_index=True, out=xyz[:, 2048:6144], **kw)
    assert torch.equal(index, want_index) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert got.data_ptr() == xyz[:, 2048:6144].data_ptr() and torch.equal(xyz[:, 2048:6144, :3], want)
    assert torch.equal(xyz[..., 3], before[..., 3])  # the label column stays
    assert torch.equal(xyz[:, :2048], before[:, :2048]) and torch.equal(xyz[:, 6144:], before[:, 6144:])
    # the four-column tensor itself, too
    got4 = clean_point_clouds(wide, 4096, seed=3, **kw)
    assert torch.equal(got4.view(torch.int32), want.view(torch.int32))


def test_too_few_survivors_raises_like_numpy_and_filter_only_returns_masks():
    case = (3, 65, True, True, True, True, 0)  # counts = [0, 17, 65]
    cloud, kw = device_arguments(case)
    reason, count = clean_point_clouds(cloud, 0, **kw)
    kept = count.cpu().numpy()
    assert kept[0] == 0 and kept[1] < kept[2] and reason.shape == (3, 65) and reason.dtype == torch.uint8
    n_out = int(kept[2])  # environment 2 can draw, 0 and 1 cannot
    out = torch.full((3, n_out, 3), 123.0, device=DEV)
    with pytest.raises(ValueError, match=r"larger sample than population.*environment 0 keeps 0 of its rows"):
        clean_point_clouds(cloud, n_out, out=out, **kw)
    assert (out[:2] == 123.0).all() and not (out[2] == 123.0).any()
    assert np.array_equal(clean_point_clouds.last_counts.cpu().numpy(), kept)
    with pytest.raises(_lib.MpxError):
        clean_point_clouds(cloud, 4097, **kw)


def test_reference_signature_crops_and_draws():
    data = f64.make_case((3, 12289, True, True, True, False, 4096))
    xyz = data["cloud"][0]
    i = np.arange(len(xyz))
    rgba = np.stack([i & 255, (i >> 8) & 255, (i >> 16) & 255, np.full_like(i, 255)], axis=1).astype(np.uint8)
    pts, colours = clean_point_cloud(xyz, rgba)
    assert pts.shape == (4096, 3) and pts.dtype == np.float32 and colours.shape == (4096, 4) and colours.dtype == np.uint8
    src = colours[:, 0].astype(np.int64) | (colours[:, 1].astype(np.int64) << 8) | (colours[:, 2].astype(np.int64) << 16)
    assert len(set(src.tolist())) == 4096  # without replacement
    assert np.array_equal(pts.view(np.int32), xyz[src].view(np.int32))  # the colours still belong to their points
    inside = np.zeros(4096, bool)
    for b in REFERENCE_WORKSPACE:
        inside |= ((pts > b[:3]) & (pts < b[3:])).all(axis=1)
    assert inside.all()
    # the reference's own mask (planning_node.py:201-222), and the draw is from all of it
    mask = np.zeros(len(xyz), bool)
    with np.errstate(invalid="ignore"):
        for b in REFERENCE_WORKSPACE:
            mask |= ((xyz > b[:3]) & (xyz < b[3:])).all(axis=1)
    assert np.array_equal(src, f64.draw(mask, 4096, 0, 0))
    assert not np.array_equal(clean_point_cloud(xyz, rgba, seed=1)[0], pts)


def test_capture_to_policy_and_cloud_check():
    """capture -> clean (robot margin 2 cm) -> slab -> policy forward, and check_cloud at the capture configuration with
    point_radius + clearance = 1.5 cm < margin: no environment may hit (both kernels use the same centres and the same
    squared distance), while the uncleaned capture hits in every environment."""
    from mpinets_amd.model import MotionPolicyNetwork
    from mpinets_amd.scenes import make_problem_batch

    case = (3, 12289, True, True, True, False, 4096)
    cloud, kw = device_arguments(case)
    q0, s = kw["q"], sampler()
    prob = make_problem_batch(3, seed=3, device=DEV)
    xyz = prob["xyz"]
    cleaned = clean_point_clouds(cloud, 4096, seed=11, out=xyz[:, 2048:6144], **kw)
    assert kw["robot_margin"] == 0.02 and (clean_point_clouds.last_counts >= 4096).all()
    torch.manual_seed(0)
    mdl = MotionPolicyNetwork().to(DEV).eval()
    with torch.no_grad():
        dq = mdl(xyz, prob["q_norm"])
    assert dq.shape == (3, 7) and torch.isfinite(dq).all()
    assert not s.check_cloud(q0, cleaned, point_radius=0.01, clearance=0.005).any()
    assert s.check_cloud(q0, cloud, point_radius=0.01, clearance=0.005).all()
