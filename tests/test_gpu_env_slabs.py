"""The entries that walk more environments than one launch's gridDim.y (65 535) in slabs, each re-offsetting its operands by
hand per slab, given 65 535 + 3 environments: a full slab and a slab of three.

For the entries whose result does not depend on the environment's index the data is PERIODIC with period 7:
``operand[b] = base[b % 7]``.  65 535 = 7 * 9362 + 1, so the phase of an environment's data differs from the phase of its
position in its slab: a slab offset that is missing, off by a slab, off by a row or scaled by another operand's row length
hands some environment of the second slab the data of another phase, and its output differs from its base's.  Environments
0..6 are held to an independent reference; EVERY other environment must equal environment ``b % 7`` bit for bit (the whole
tensor is compared, nothing is sampled).  With the three-environment second slab a wrong multiplier stays inside the
operand (the operands hold 65 538 environments; a multiplier that is too small reads earlier rows).

``mpx_scene_cloud`` draws by environment id, so it is held to its own contract instead: a shard of a larger batch draws
exactly what the unsharded batch draws.

Each test names the launcher lines it enters."""
import numpy as np
import pytest
import torch

import float64_collision as fc

pytestmark = pytest.mark.gpu

GRID_Y = 65535  # MPX_GRID_Y of csrc/common.h
B = GRID_Y + 3
PERIOD = 7
U = 2.0 ** -24


def dev():
    return torch.device("cuda:0")


def phase():
    return torch.arange(B, device=dev()) % PERIOD


def tiled(base):
    """numpy [7, ...] -> device [B, ...] with row b = base[b % 7]."""
    assert base.shape[0] == PERIOD
    return torch.from_numpy(np.ascontiguousarray(base)).to(dev())[phase()].contiguous()


def _bits(t):
    t = t.reshape(t.shape[0], -1)
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_periodic(out, what):
    """Every environment of ``out`` [B, ...] equals environment b % 7, bit for bit."""
    assert out.shape[0] == B
    flat = _bits(out)
    same = (flat == flat[:PERIOD][phase()]).all(dim=1)
    bad = torch.nonzero(~same).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} environments differ from their base, the first at {bad[:8].tolist()}"
    print(f"ENVSLABS {what}: environments 7..{B - 1} vs environment b % 7 bit-equal")


@pytest.fixture
def free_device_memory():
    yield
    torch.cuda.empty_cache()  # (the bucketed ball query case holds about 1.7 GB)


def test_the_batch_crosses_one_slab_edge_out_of_phase():
    """CPU arithmetic the construction rests on."""
    assert GRID_Y % PERIOD == 1 and GRID_Y < B < 2 * GRID_Y and B - GRID_Y == 3
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "constexpr int MPX_GRID_Y = %d;" % GRID_Y in open(os.path.join(root, "motion-policy-networks_amd", "csrc", "common.h")).read()


# ---- point-vs-primitive distances -------------------------------------------------------------------------------------
def _quats(rng, n):
    q = rng.standard_normal((n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _device_frames(centers, quats):
    """float32 [7,M,16]: the inverse frames ``mpx_prim_frames`` makes of the bases -- what the distance kernels work from."""
    from mpinets_amd import _lib

    c, q = torch.from_numpy(centers).to(dev()), torch.from_numpy(quats).to(dev())
    f = torch.empty(centers.shape[:2] + (16,), dtype=torch.float32, device=dev())
    _lib.call("mpx_prim_frames", c.data_ptr(), q.data_ptr(), centers.shape[0] * centers.shape[1], f.data_ptr())
    return f


@pytest.mark.parametrize("kind", ["cuboid", "cylinder", "sphere"])
def test_primitive_sdf_past_one_slab(kind):
    """``launch_sdf`` (csrc/geometry.hip), the loop ``for (b0 = 0; b0 < B; b0 += 65535)``: frames + (sphere ? 3 : 16) po,
    pa + (cuboid ? 3 : 1) po, pb + po (cylinder), points + b0 P 3, out + b0 P -- a different set of multipliers per kind."""
    from mpinets_amd import _lib

    M, P = 2, 5
    rng = np.random.default_rng({"cuboid": 11, "cylinder": 12, "sphere": 13}[kind])
    centers = rng.uniform(-0.3, 0.3, (PERIOD, M, 3)).astype(np.float32)
    quats = _quats(rng, PERIOD * M).reshape(PERIOD, M, 4)
    dims = rng.uniform(0.1, 0.4, (PERIOD, M, 3)).astype(np.float32)   # cuboid: dims; cylinder: [..., 0] radius, [..., 1] height
    points = rng.uniform(-0.6, 0.6, (PERIOD, P, 3)).astype(np.float32)
    dims[3, 0, 0 if kind != "cuboid" else 1] = 0.0                    # base 3: one zero-volume primitive
    dims[5, :, 0 if kind != "cylinder" else 1] = 0.0                  # base 5: both -> +inf
    pts = tiled(points)
    out = torch.full((B, P), -7.0, dtype=torch.float32, device=dev())
    if kind == "sphere":
        radii = np.ascontiguousarray(dims[..., 0])
        cd, rd = tiled(centers), tiled(radii)
        _lib.call("mpx_sphere_sdf", cd.data_ptr(), rd.data_ptr(), B, M, pts.data_ptr(), P, out.data_ptr())
        d = np.linalg.norm(points.astype(np.float64)[:, None] - centers.astype(np.float64)[:, :, None], axis=-1) - radii.astype(np.float64)[..., None]
        d[np.abs(radii) <= np.float32(1e-8)] = np.inf
        ref = d.min(axis=1)[:, None]                                  # [7,1,P]
    else:
        frames = _device_frames(centers, quats)
        f44 = frames.cpu().numpy().reshape(PERIOD, M, 4, 4)
        none44, none = np.zeros((PERIOD, 0, 4, 4), np.float32), np.zeros((PERIOD, 0), np.float32)
        fr = tiled(frames.cpu().numpy())
        if kind == "cuboid":
            dd = tiled(dims)
            _lib.call("mpx_cuboid_sdf", fr.data_ptr(), dd.data_ptr(), B, M, pts.data_ptr(), P, out.data_ptr())
            ref = fc.restate(points[:, None], f44, dims, none44, none, none)
        else:
            rad, hgt = np.ascontiguousarray(dims[..., 0]), np.ascontiguousarray(dims[..., 1])
            rd, hd = tiled(rad), tiled(hgt)
            _lib.call("mpx_cylinder_sdf", fr.data_ptr(), rd.data_ptr(), hd.data_ptr(), B, M, pts.data_ptr(), P, out.data_ptr())
            ref = fc.restate(points[:, None], none44, np.zeros((PERIOD, 0, 3), np.float32), f44, rad, hgt)
    torch.cuda.synchronize()
    got = out[:PERIOD].cpu().numpy()[:, None]
    assert np.isposinf(ref[5]).all() and np.isfinite(ref[[0, 1, 2, 3, 4, 6]]).all()
    bad, worst = fc.offending_envs(got, ref)
    print(f"ENVSLABS {kind} sdf: environments 0..6 vs float64, largest err / bar = {worst / fc.SDF_BAR:.4f}")
    assert bad == set()
    assert_periodic(out, f"{kind} sdf")


# ---- table points moved by one pose per environment --------------------------------------------------------------------
def test_pose_cloud_past_one_slab():
    """``mpx_pose_cloud`` (csrc/franka.hip), ``if (B > MPX_GRID_Y)``: poses + b0 16, out + b0 out_batch_stride."""
    from mpinets_amd import _lib

    rng = np.random.default_rng(21)
    n_table, n_out, ops = 10, 6, 4
    poses = np.zeros((PERIOD, 4, 4), np.float32)
    q = _quats(rng, PERIOD).astype(np.float64)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(PERIOD, 3, 3)
    poses[:, :3, :3], poses[:, :3, 3], poses[:, 3, 3] = R, rng.uniform(-1, 1, (PERIOD, 3)), 1.0
    table = rng.uniform(-0.5, 0.5, (n_table, 3)).astype(np.float32)
    subset = rng.permutation(n_table)[:n_out].astype(np.int32)
    td, sd = torch.from_numpy(table).to(dev()), torch.from_numpy(subset).to(dev())
    out = torch.full((B, n_out, ops), -7.0, dtype=torch.float32, device=dev())
    pd = tiled(poses)
    _lib.call("mpx_pose_cloud", pd.data_ptr(), B, td.data_ptr(), sd.data_ptr(), n_out, out.data_ptr(), n_out * ops, ops)
    torch.cuda.synchronize()
    assert (out[..., 3] == -7.0).all(), "the fourth column of a point was written"
    P64, p = poses.astype(np.float64), table[subset].astype(np.float64)
    ref = np.einsum("bij,nj->bni", P64[:, :3, :3], p) + P64[:, None, :3, 3]
    bar = 4 * U / (1 - 4 * U) * (np.einsum("bij,nj->bni", np.abs(P64[:, :3, :3]), np.abs(p)) + np.abs(P64[:, None, :3, 3]))
    err = np.abs(out[:PERIOD, :, :3].cpu().numpy().astype(np.float64) - ref)
    print(f"ENVSLABS pose cloud: environments 0..6 vs float64, largest err / bar = {(err / bar).max():.4f}")
    assert (err <= bar).all()
    assert_periodic(out, "pose cloud")


# ---- max over groups of rows ---------------------------------------------------------------------------------------------
def test_rowmax_past_one_slab():
    """``mpx_rowmax`` (csrc/dense.hip), ``if (G > MPX_GRID_Y)``: x + g0 rows ldx, y + g0 ldy."""
    from mpinets_amd import _lib

    rows, C, ldx, ldy = 3, 70, 72, 71
    rng = np.random.default_rng(31)
    base = np.full((PERIOD, rows, ldx), 1e30, np.float32)  # (a padding column that is read wins the max)
    base[..., :C] = rng.standard_normal((PERIOD, rows, C)).astype(np.float32)
    x = tiled(base)
    y = torch.full((B, ldy), -7.0, dtype=torch.float32, device=dev())
    _lib.call("mpx_rowmax", x.data_ptr(), ldx, B, rows, C, y.data_ptr(), ldy)
    torch.cuda.synchronize()
    assert (y[:, C:] == -7.0).all(), "a column past C was written"
    np.testing.assert_array_equal(y[:PERIOD, :C].cpu().numpy(), base[..., :C].max(axis=1))
    print("ENVSLABS rowmax: environments 0..6 vs the float32 maximum bit-equal")
    assert_periodic(y, "rowmax")


# ---- ball query -----------------------------------------------------------------------------------------------------------
# (N, npoint, nsample, radius, stride) and the kernel family ball_query_impl's conditions give the shape
BALL_SHAPES = {"wave": (40, 5, 8, 0.25, 3),          # N <= 512: a wave per query
               "brute-force": (600, 5, 8, 0.1, 4),    # 512 < N < 2048: a thread per query (stride 4, 64-byte aligned rows)
               "bucketed": (2048, 8, 64, 0.05, 3)}    # N >= 2048, 40 < nsample <= 128, 48 radius < 4: the column buckets
IDX_SENTINEL = -7


def _ball_bases(N, npoint, nsample, radius, seed):
    """Seven clouds in the unit cube with a cluster of nsample + 4 points, and queries: 0 at the cluster (overflows), 1 far
    away (no hit), the others at cloud points outside the cluster (a few hits, themselves among them)."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.5, 0.5, (PERIOD, N, 3)).astype(np.float32)
    centre = np.float32([0.1, 0.2, -0.1])
    xyz[:, 4:4 + nsample + 4] = centre + rng.normal(scale=radius * 0.2, size=(PERIOD, nsample + 4, 3)).astype(np.float32)
    new = np.empty((PERIOD, npoint, 3), np.float32)
    for b in range(PERIOD):
        new[b] = xyz[b, (4 + nsample + 4) + rng.permutation(N - (4 + nsample + 4))[:npoint]]
    new[:, 0], new[:, 1] = centre, 50.0
    return xyz, new


@pytest.mark.parametrize("family", list(BALL_SHAPES))
def test_ball_query_past_one_slab(oracle, family, free_device_memory):
    """``ball_query_impl`` (csrc/pointnet.hip), ``if (B > MPX_GRID_Y)``: new_xyz + b0 npoint new_stride, xyz + b0 N stride,
    idx + b0 npoint nsample, cnt + b0 npoint -- through ``mpx_ball_query``, ``mpx_ball_query_hits`` and
    ``mpx_ball_query_set``, each recursing into the small-cloud wave kernel, the brute-force kernel or the bucketed kernel."""
    from mpinets_amd import _lib

    N, npoint, nsample, radius, stride = BALL_SHAPES[family]
    xyz3, new3 = _ball_bases(N, npoint, nsample, radius, 41 + N)
    ref, rcnt = oracle.ball_query(new3, xyz3, radius, nsample, return_counts=True)
    # the mix: query 0 has more hits than slots, query 1 none, most of the others a few
    d2 = ((new3[:, :, None].astype(np.float64) - xyz3[:, None].astype(np.float64)) ** 2).sum(-1)
    assert ((d2[:, 0] < (0.99 * radius) ** 2).sum(-1) > nsample).all() and (rcnt[:, 0] == nsample).all() and (rcnt[:, 1] == 0).all()
    few = (rcnt[:, 2:] >= 1) & (rcnt[:, 2:] < nsample)
    assert few.mean() > 0.5 and len(np.unique(rcnt[:, 2:])) > 1, rcnt
    base = np.full((PERIOD, N, stride), np.nan, np.float32)
    base[..., :3] = xyz3
    xd, nd = tiled(base), tiled(new3)
    assert stride != 4 or (xd.data_ptr() % 64 == 0 and N % 4 == 0)
    slots = np.arange(nsample)[None, None, :] < np.maximum(rcnt, 1)[..., None]  # what _hits / _set write
    for entry in ("mpx_ball_query", "mpx_ball_query_hits", "mpx_ball_query_set"):
        idx = torch.full((B, npoint, nsample), IDX_SENTINEL, dtype=torch.int32, device=dev())
        cnt = torch.full((B, npoint), IDX_SENTINEL, dtype=torch.int32, device=dev())
        _lib.call(entry, nd.data_ptr(), 3, xd.data_ptr(), stride, B, N, npoint, float(radius), nsample, idx.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        got, gcnt = idx[:PERIOD].cpu().numpy(), cnt[:PERIOD].cpu().numpy()
        np.testing.assert_array_equal(gcnt, rcnt, err_msg=entry)
        if entry == "mpx_ball_query":
            np.testing.assert_array_equal(got, ref, err_msg=entry)                      # padded rows, exactly
        else:
            assert (got[~slots] == IDX_SENTINEL).all(), f"{entry}: a slot past the hits was written"
            if entry == "mpx_ball_query_set":                                           # the hits as sorted sets
                got, idx = np.sort(np.where(slots, got, np.iinfo(np.int32).max), axis=-1), torch.sort(idx, dim=-1).values
                np.testing.assert_array_equal(got, np.sort(np.where(slots, ref, np.iinfo(np.int32).max), axis=-1), err_msg=entry)
            else:
                np.testing.assert_array_equal(got[slots], ref[slots], err_msg=entry)    # the hit slots, exactly
        print(f"ENVSLABS {entry} ({family}): environments 0..6 vs the oracle bit-equal")
        assert_periodic(cnt, f"{entry} ({family}) counts")
        assert_periodic(idx, f"{entry} ({family}) rows" + (" (each row sorted: a set)" if entry.endswith("_set") else ""))
        del idx, cnt


# ---- scene clouds ---------------------------------------------------------------------------------------------------------
def test_scene_cloud_past_one_slab_equals_its_shards(oracle):
    """``mpx_scene_cloud`` (csrc/scene.hip), ``if (B > MPX_GRID_Y)``: cub_centers + b0 M1 3, cub_dims + b0 M1 3, cub_quats +
    b0 M1 4, cyl_centers + b0 M2 3, cyl_radii + b0 M2, cyl_heights + b0 M2, cyl_quats + b0 M2 4, env_offset + b0, assign + b0
    num_points, labels + b0 (M1 + M2), n_obstacles + b0, out + b0 out_batch_stride.  The draws are keyed by the environment's
    id, so the data is not periodic: the one call must equal, bit for bit, the call on environments [0, 65 535) and the call
    on [65 535, B) with env_offset = 65 535 (the header: a shard of a larger batch draws exactly what the unsharded batch
    draws), and environments 65 533..65 537 must equal the oracle's restatement on the ids."""
    from mpinets_amd import _lib

    M1, M2, NP, seed = 2, 1, 64, 20261021
    rng = np.random.default_rng(51)
    scn = {"cuboid_centers": rng.uniform(-0.5, 0.5, (B, M1, 3)).astype(np.float32),
           "cuboid_dims": rng.uniform(0.05, 0.4, (B, M1, 3)).astype(np.float32),
           "cuboid_quats": _quats(rng, B * M1).reshape(B, M1, 4),
           "cylinder_centers": rng.uniform(-0.5, 0.5, (B, M2, 3)).astype(np.float32),
           "cylinder_radii": rng.uniform(0.05, 0.2, (B, M2, 1)).astype(np.float32),
           "cylinder_heights": rng.uniform(0.05, 0.4, (B, M2, 1)).astype(np.float32),
           "cylinder_quats": _quats(rng, B * M2).reshape(B, M2, 4)}
    scn["cuboid_dims"][GRID_Y - 1, 1, 2] = 0.0     # a zero-volume primitive on each side of the slab edge ...
    scn["cuboid_dims"][GRID_Y, 0, 0] = 0.0
    scn["cylinder_radii"][GRID_Y + 2] = 0.0
    scn["cuboid_dims"][GRID_Y + 1] = 0.0           # ... and nothing alive in one environment of the second slab
    scn["cylinder_heights"][GRID_Y + 1] = 0.0
    keys = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights", "cylinder_quats")
    d = {k: torch.from_numpy(scn[k]).to(dev()) for k in keys}

    def outputs():
        return (torch.full((B, NP, 4), -3.0, dtype=torch.float32, device=dev()), torch.full((B, NP), -3, dtype=torch.int16, device=dev()),
                torch.full((B, M1 + M2), 77, dtype=torch.uint8, device=dev()), torch.full((B,), -3, dtype=torch.int32, device=dev()))

    def draw(o, lo, hi):
        out, assign, labels, nobs = o
        _lib.call("mpx_scene_cloud", d[keys[0]][lo:].data_ptr(), d[keys[1]][lo:].data_ptr(), d[keys[2]][lo:].data_ptr(), M1,
                  d[keys[3]][lo:].data_ptr(), d[keys[4]][lo:].data_ptr(), d[keys[5]][lo:].data_ptr(), d[keys[6]][lo:].data_ptr(), M2,
                  hi - lo, NP, seed, lo, assign[lo:].data_ptr(), labels[lo:].data_ptr(), nobs[lo:].data_ptr(), out[lo:].data_ptr(),
                  NP * 4, 4, 1)

    whole, shards = outputs(), outputs()
    draw(whole, 0, B)
    draw(shards, 0, GRID_Y)
    draw(shards, GRID_Y, B)
    torch.cuda.synchronize()
    for name, a, b in zip(("points and labels", "assign", "labels", "n_obstacles"), whole, shards):
        assert not (a == (77 if a.dtype == torch.uint8 else -3)).any(), f"{name}: an element was left unwritten"
        bad = torch.nonzero(~(_bits(a) == _bits(b)).all(dim=1)).flatten()
        assert bad.numel() == 0, f"{name}: {bad.numel()} environments differ from the shards, the first at {bad[:8].tolist()}"
        print(f"ENVSLABS scene cloud {name}: one call vs its two shards bit-equal")
    lo, hi = GRID_Y - 2, GRID_Y + 3
    opts, oassign, olabels, onobs = oracle.scene_cloud({k: scn[k][lo:hi] for k in keys}, NP, seed, env_offset=lo)
    out, assign, labels, nobs = (t[lo:hi].cpu().numpy() for t in whole)
    assert onobs.tolist() == [3, 2, 2, 0, 2]
    np.testing.assert_array_equal(assign.view(np.uint16), oassign)
    np.testing.assert_array_equal(labels, olabels)
    np.testing.assert_array_equal(nobs, onobs)
    np.testing.assert_allclose(out[..., :3], opts, rtol=0, atol=1e-6)  # (the bar tests/test_scene_cloud.py holds the points to)
    want = np.take_along_axis(olabels.astype(np.float32), np.minimum(oassign, M1 + M2 - 1).astype(np.int64), 1)
    want[oassign == 0xFFFF] = 0
    np.testing.assert_array_equal(out[..., 3], want)
    print("ENVSLABS scene cloud: environments 65533..65537 vs the oracle on the ids bit-equal")
