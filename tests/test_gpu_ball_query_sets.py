"""GPU: ``mpx_ball_query_set`` -- the hit slots of a neighbourhood as a SET, in no particular order -- and the proof that
its consumers do not care.

The engine's forward hands the neighbour rows only to the fused grouped-MLP kernels with their counts, and those max-pool
over the listed neighbours: a max over a set does not depend on the order of its members.  So the first module's bucketed
search may skip its per-row sort.  Pinned here: (1) counts and per-row sets equal ``mpx_ball_query_hits`` on each of the
three search kernels, slots past ``max(cnt, 1)`` untouched; (2) the grouped-MLP kernels give the same bits for permuted
rows, at the small and at the persistent launch shape, fp32 and bf16x3 (needs none of the new code); (3) the forward and
the rollout give the same bits with the ordered search forced, and the native loop equals ``step()``.  Reference
semantics: pointnet2_ops ball_query, "first nsample hits in index order" (oracle/oracle.py ``ball_query``)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7


def dev():
    return torch.device("cuda:0")


def crafted_cloud(seed, N, npoint, nsample, radius, stride):
    """One environment: a random cloud in [0.01, 0.99]^2 x [0, 0.5] plus, two units above it, a cluster of EXACTLY
    ``nsample`` points and one of ``nsample + 20`` points around their own queries; the cloud's (x, y) bounding-box corners
    are points of it.  The point order is shuffled (cluster indices are scattered over [0, N), so "the nsample smallest"
    is not "the first found").  Queries: 0 = no hit, 1 = exactly nsample hits, 2 = overflow, 3 / 4 = the lower / upper
    corner of the bounding box, the rest = points of the cloud.  -> (points [N, stride], queries [npoint, 3], overflow
    cluster's point ids)."""
    rng = np.random.RandomState(seed)
    n_over = nsample + 20
    n_rand = N - nsample - n_over - 2
    assert n_rand >= npoint
    box = np.concatenate([rng.uniform(0.01, 0.99, (n_rand, 2)), rng.uniform(0.0, 0.5, (n_rand, 1))], axis=1)
    corners = np.array([[0.0, 0.0, 0.25], [1.0, 1.0, 0.25]])
    c_exact, c_over = np.array([0.3, 0.6, 2.0]), np.array([0.7, 0.2, 2.0])

    def ball(c, n):  # n points strictly inside 0.4 * radius of c
        d = rng.normal(size=(n, 3))
        d *= (0.4 * radius * rng.uniform(0.1, 1.0, (n, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
        return c + d

    pts = np.concatenate([box, corners, ball(c_exact, nsample), ball(c_over, n_over)]).astype(np.float32)
    perm = rng.permutation(N)
    pts = pts[perm]
    over_ids = np.sort(np.nonzero(perm >= N - n_over)[0])  # (shuffled index i holds original row perm[i])
    q = np.empty((npoint, 3), np.float32)
    q[0] = (0.5, 0.5, 5.0)
    q[1], q[2] = c_exact, c_over
    q[3], q[4] = corners
    q[5:] = pts[rng.choice(np.nonzero(perm < n_rand)[0], npoint - 5, replace=False)]
    full = np.zeros((N, stride), np.float32)
    full[:, :3] = pts
    if stride > 3:
        full[:, 3:] = rng.uniform(0, 1, (N, stride - 3))
    return full, q, over_ids


def crafted_batch(B, seed, N, npoint, nsample, radius, stride):
    parts = [crafted_cloud(seed + b, N, npoint, nsample, radius, stride) for b in range(B)]
    x = torch.from_numpy(np.stack([p[0] for p in parts])).to(dev())
    q = torch.from_numpy(np.stack([p[1] for p in parts])).to(dev())
    return x, q, [p[2] for p in parts]


def search(entry, x, q, radius, nsample):
    from mpinets_amd import _lib

    B, N, stride = x.shape
    npoint = q.size(1)
    idx = torch.full((B, npoint, nsample), SENTINEL, dtype=torch.int32, device=x.device)
    cnt = torch.full((B, npoint), SENTINEL, dtype=torch.int32, device=x.device)
    _lib.call(entry, _lib.ptr(q), 3, _lib.ptr(x), stride, B, N, npoint, float(radius), nsample, _lib.ptr(idx), _lib.ptr(cnt))
    return idx, cnt


def sorted_sets(idx, cnt):
    """Rows with the slots at or beyond max(cnt, 1) replaced by a key above every index, sorted."""
    live = torch.arange(idx.size(2), device=idx.device)[None, None, :] < cnt.clamp(min=1)[:, :, None]
    return torch.where(live, idx, torch.full_like(idx, 1 << 30)).sort(dim=2).values, live


# (grid path: N = 2048 is its smallest cloud, nsample = 64 > the 40 hits the ordered kernel parks in LDS, 64 queries on 16
# waves; wave path: the second module's shape class, N <= 512; brute force: a cloud size neither of them takes)
@pytest.mark.parametrize("path,B,N,npoint,nsample,radius,stride", [
    ("grid", 3, 2048, 64, 64, 0.05, 4), ("wave", 3, 512, 128, 128, 0.3, 3), ("brute", 3, 1000, 64, 64, 0.1, 4)])
def test_set_rows_equal_the_ordered_hit_rows_as_sets(path, B, N, npoint, nsample, radius, stride):
    x, q, over_ids = crafted_batch(B, 100, N, npoint, nsample, radius, stride)
    ref_idx, ref_cnt = search("mpx_ball_query_hits", x, q, radius, nsample)
    idx, cnt = search("mpx_ball_query_set", x, q, radius, nsample)
    # the inputs hold the cases they were built for
    assert (ref_cnt[:, 0] == 0).all() and (ref_idx[:, 0, 0] == 0).all(), "query 0 must have no hit"
    assert (ref_cnt[:, 1] == nsample).all() and (ref_cnt[:, 2] == nsample).all()
    assert (ref_cnt[:, 3:5] >= 1).all(), "the bounding-box corners are points of the cloud"
    for b in range(B):  # overflow: the nsample SMALLEST indices of the cluster
        assert ref_idx[b, 2].cpu().numpy().tolist() == over_ids[b][:nsample].tolist()
        assert over_ids[b].size == nsample + 20
    assert int(ref_cnt[:, 5:].max()) < nsample and int(ref_cnt[:, 5:].min()) >= 1
    # the contract
    assert torch.equal(cnt, ref_cnt)
    got, live = sorted_sets(idx, cnt)
    want, _ = sorted_sets(ref_idx, ref_cnt)
    assert torch.equal(got, want)
    assert (idx[~live] == SENTINEL).all(), "slots at or beyond max(cnt, 1) must be left untouched"
    assert (ref_idx[~live] == SENTINEL).all()


def test_set_entry_point_requires_counts_and_short_rows():
    from mpinets_amd import _lib

    x = torch.zeros((1, 600, 3), device=dev())
    idx = torch.zeros((1, 4, 288), dtype=torch.int32, device=dev())
    cnt = torch.zeros((1, 4), dtype=torch.int32, device=dev())
    with pytest.raises(_lib.MpxError, match="nsample = 288 > 256"):
        _lib.call("mpx_ball_query_set", _lib.ptr(x), 3, _lib.ptr(x), 3, 1, 600, 4, 0.1, 288, _lib.ptr(idx), _lib.ptr(cnt))
    with pytest.raises(_lib.MpxError, match="hit counts are required"):
        _lib.call("mpx_ball_query_set", _lib.ptr(x), 3, _lib.ptr(x), 3, 1, 600, 4, 0.1, 128, _lib.ptr(idx), None)


# ---- the consumers: permuting slots [0, cnt) of every row changes no output bit ------------------------------------------
def permute_hits(nbr, cnt, seed):
    """Slots [0, cnt) of every row in a seeded random order; the padding slots stay where they are."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    key = torch.rand(nbr.shape, generator=g).to(nbr.device)
    slot = torch.arange(nbr.size(2), device=nbr.device)[None, None, :]
    key = torch.where(slot < cnt[:, :, None], key, 2.0 + slot.float())  # padding keeps its place
    out = torch.gather(nbr, 2, key.argsort(dim=2))
    assert not torch.equal(out, nbr)
    return out


# (B = 2: a few queries per wave; B = 64: 32 x 1024 queries of the first module / 8 x 1024 of the second -- where the launch
# plan turns to the persistent grid fed from the unit queue)
@pytest.mark.parametrize("B", [2, 64])
def test_grouped_mlp_kernels_ignore_the_order_of_the_hits(B):
    from mpinets_amd import _lib
    from mpinets_amd.pointnet2 import PointnetSAModule, ball_query, launch_sa, sa_mlp_factored

    torch.manual_seed(3)
    sa1 = PointnetSAModule(npoint=512, radius=0.05, nsample=128, mlp=[1, 64, 64, 64], bn=False).to(dev())
    sa2 = PointnetSAModule(npoint=128, radius=0.3, nsample=128, mlp=[64, 128, 128, 256], bn=False).to(dev())

    # -- first module's shape: mpx_sa_mlp / mpx_sa_mlp_bf16x3 over [p - c ; label] rows
    one = crafted_batch(2, 300, 2048, 512, 128, 0.05, 4)
    pc = one[0].repeat(B // 2, 1, 1).contiguous()
    ctr = one[1].repeat(B // 2, 1, 1).contiguous()
    nbr, cnt = ball_query(0.05, 128, pc[:, :, :3].contiguous(), ctr, return_counts=True)
    assert int(cnt.min()) == 0 and int(cnt.max()) == 128
    shuffled = permute_hits(nbr, cnt, 11)
    c1 = sa1.convs()
    for precision in ("fp32", "bf16x3"):
        w = sa1._packed.get(c1, 1, precision)

        def run(rows):
            out = torch.full((B, 512, 68), float("nan"), dtype=torch.float32, device=dev())
            launch_sa(precision, _lib.ptr(pc), 4, _lib.ptr(ctr), 3, _lib.ptr(pc) + 12, 4, 1, rows, cnt, B, 2048, 512, 128, w,
                      (64, 64, 64), _lib.ptr(out), 68)
            return out[:, :, :64].clone()

        a, b = run(nbr), run(shuffled)
        assert torch.isfinite(a).all() and torch.equal(a, b), f"SA1 {precision}"

    # -- second module's shape: mpx_sa_mlp_factored / mpx_sa_mlp_bf16x3_factored over [f | xyz | 0] point rows
    one = crafted_batch(2, 400, 512, 128, 128, 0.3, 3)
    x1 = one[0].repeat(B // 2, 1, 1).contiguous()
    x2 = one[1].repeat(B // 2, 1, 1).contiguous()
    nbr, cnt = ball_query(0.3, 128, x1, x2, return_counts=True)
    assert int(cnt.min()) == 0 and int(cnt.max()) == 128
    shuffled = permute_hits(nbr, cnt, 12)
    g = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.zeros((B, 512, 68), device=dev())
    rows[:, :, :64] = torch.rand((B, 512, 64), generator=g).to(dev())
    rows[:, :, 64:67] = x1
    centre = torch.zeros((B, 128, 4), device=dev())
    centre[:, :, :3] = x2
    c2 = sa2.convs()
    for precision in ("fp32", "bf16x3"):
        def run(r):
            out = torch.full((B, 128, 256), float("nan"), dtype=torch.float32, device=dev())
            sa_mlp_factored(rows.view(B * 512, 68), centre.view(B * 128, 4), r, cnt, sa2._packed, c2, 64, 512, _lib.ptr(out),
                            256, precision=precision)
            return out

        a, b = run(nbr), run(shuffled)
        assert torch.isfinite(a).all() and torch.equal(a, b), f"SA2 {precision}"


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_forward_is_bit_identical_with_the_ordered_search_forced(precision):
    from mpinets_amd.model import MotionPolicyNetwork
    from mpinets_amd.scenes import make_problem_batch

    torch.manual_seed(8)
    mdl = MotionPolicyNetwork().to(dev()).eval().set_precision(precision)
    prob = make_problem_batch(4, seed=21, device=dev(), kinds=("tabletop", "cubby", "dresser"), M1=40, device_clouds=True)
    enc = mdl.point_cloud_encoder
    assert enc.ordered_ball_query is False
    with torch.no_grad():
        dq_set = mdl(prob["xyz"], prob["q_norm"])
        cnt_set = [c.clone() for c in enc.last_counts]
        enc.ordered_ball_query = True
        dq_ord = mdl(prob["xyz"], prob["q_norm"])
        enc.ordered_ball_query = False
    assert torch.equal(dq_set, dq_ord)
    assert all(torch.equal(a, b) for a, b in zip(cnt_set, enc.last_counts))


def test_rollout_is_bit_identical_with_the_ordered_search_forced_and_native_equals_step():
    from mpinets_amd.model import MotionPolicyNetwork
    from mpinets_amd.rollout import RolloutEngine
    from mpinets_amd.scenes import make_problem_batch

    torch.manual_seed(12)
    mdl = MotionPolicyNetwork().to(dev()).eval()
    enc = mdl.point_cloud_encoder
    sets, ordered, native = (RolloutEngine(mdl, make_problem_batch(4, seed=31, device=dev(), kinds=("tabletop", "cubby", "dresser"),
                                                                   M1=40, M2=16, device_clouds=True),
                                           rerender_scene=True, scene_seed=77) for _ in range(3))
    for _ in range(3):
        sets.step()
    enc.ordered_ball_query = True
    try:
        for _ in range(3):
            ordered.step()
    finally:
        enc.ordered_ball_query = False
    native.run_native(3)
    for other in (ordered, native):
        assert torch.equal(sets.q, other.q) and torch.equal(sets.q_norm, other.q_norm)
        assert torch.equal(sets.flags, other.flags) and torch.equal(sets.xyz, other.xyz)
