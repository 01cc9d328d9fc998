"""Restatement of ``mpx_cloud_field_build`` and ``mpx_cloud_field_sample`` on the CPU, written from the contracts in
include/mpinets_hip.h (not from csrc/cloud_field.hip).

Build.  Node coordinates are formed as the device rounds them: the float64 ``i * h + lo`` of float32 operands, rounded once
to float32 (an fma; ``float64_plan.line`` emulates its fma the same way).  ``dx = node.x - p.x`` (likewise y, z) is the
device's own float32 subtraction; the squares and their sum are float64.  What is left between this and the device is the
three roundings of ``mpx_sqdist``: the device's d2 is within ``3 * 2^-24`` relative of the float64 value, the bands use
``BAND = 4 * 2^-24`` on d2 as tests/float64_cloud_collision.py does.  The field must be the correctly rounded square
root of a number within BAND of the float64 minimum wherever that is below ``trunc^2 (1 - BAND)``, exactly ``trunc``
wherever it is above ``trunc^2 (1 + BAND)``, and either in between (``check_field``).

Sample.  ``sample`` runs the header's statements in the dtype it is given: float64 (the reference) or float32 with every
lerp an emulated fma (the reference-against-reference measurement that sets the bars of the GPU test).

Also here: the cases and seeded inputs of tests/test_gpu_cloud_field.py, so that tests/test_cloud_field_host.py can run
the same cases on the CPU.
"""
import numpy as np
import torch

BAND = 4.0 * 2.0 ** -24
TILE = 256  # MPX_CLOUD_TILE: points per LDS tile of the build
BRICK = 8   # MPX_FIELD_BRICK
FACE = 1e-5  # samples within this many cells of a cell face are left out of the gradient comparison
FACE_CAP = 0.01

REACH_LO = np.array([-0.9, -0.9, -0.3], np.float32)
REACH_HI = np.array([0.9, 0.9, 1.2], np.float32)

# (nx, ny, nz): no side a multiple of the brick but one 8; one brick, several bricks along x, y and z
GRIDS = [(2, 2, 2), (9, 8, 5), (17, 3, 2), (33, 9, 6)]

# (B, N, grid index, trunc: "small" (below the grid's diagonal) | "large" (above it), extras)
# extras: "counts" (below 0, above N, in between), "bad" (NaN / inf rows), "empty" (environment 0 has no usable row),
# "slab" (the [B,6272,4][:, 2048:2048+N, :3] view), "far" (a fifth of the points far outside the grid)
BUILD_CASES = [
    (1, 0, 0, "small", ()),
    (1, 1, 0, "large", ()),
    (3, 1, 1, "small", ("counts",)),
    (1, TILE - 1, 1, "small", ("bad",)),
    (3, TILE, 2, "large", ("far",)),
    (1, TILE + 1, 3, "small", ("slab",)),
    (3, 2 * TILE + 3, 3, "small", ("counts", "bad", "far", "slab")),
    (3, 2 * TILE + 3, 1, "large", ("empty", "bad")),
    (1, 2 * TILE + 3, 2, "small", ()),
    (3, TILE + 1, 0, "small", ("empty", "counts")),
    (1, TILE, 3, "large", ("bad", "far")),
    (3, 0, 2, "small", ("counts",)),
]


def case_id(case):
    B, N, g, tr, extras = case
    return f"B{B}-N{N}-grid{'x'.join(map(str, GRIDS[g]))}-{tr}" + "".join("-" + e for e in extras)


def make_grid(shape, lo=(-0.25, -0.125, 0.0), h=0.0625, trunc=0.1):
    nx, ny, nz = shape
    return {"lo": np.asarray(lo, np.float32), "h": np.float32(h), "nx": int(nx), "ny": int(ny), "nz": int(nz),
            "trunc": np.float32(trunc)}


def node_coordinates(grid):
    """-> (x [nx], y [ny], z [nz]) float32: fma((float)i, h, lo) as the device rounds it."""
    h = np.float64(grid["h"])
    return tuple((np.arange(n, dtype=np.float64) * h + np.float64(grid["lo"][a])).astype(np.float32)
                 for a, n in enumerate((grid["nx"], grid["ny"], grid["nz"])))


def make_build_case(case):
    """-> cloud float32 [B,N,3] (or its slab [B,6272,4] with ``view`` = the slice to pass), counts int32 [B] or None, grid."""
    B, N, g, tr, extras = case
    rng = np.random.default_rng(4000 + BUILD_CASES.index(case))
    shape = GRIDS[g]
    h = 0.0625 if g != 3 else 0.03
    grid = make_grid(shape, h=h)
    x, y, z = node_coordinates(grid)
    lo = np.array([x[0], y[0], z[0]], np.float32)
    hi = np.array([x[-1], y[-1], z[-1]], np.float32)
    diag = float(np.linalg.norm((hi - lo).astype(np.float64)))
    grid["trunc"] = np.float32(0.15 * diag if tr == "small" else 1.5 * diag + 0.1)
    pad = np.float32(0.5 * float(grid["trunc"]) if tr == "small" else 0.1)
    cloud = (lo - pad + rng.random((B, N, 3), dtype=np.float32) * (hi - lo + 2 * pad)).astype(np.float32)
    if "far" in extras and N:
        far = rng.random((B, N)) < 0.2
        cloud[far] += np.float32(50.0) * np.sign(rng.standard_normal((int(far.sum()), 3))).astype(np.float32)
    if "bad" in extras and N:
        rows = rng.integers(0, N, size=(B, max(1, N // 16)))
        for b in range(B):
            for i, r in enumerate(rows[b]):
                cloud[b, r, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    counts = None
    if "counts" in extras:
        counts = np.array([(-3, N + 5, N // 2)[b % 3] for b in range(B)], np.int32)
    if "empty" in extras:
        if counts is not None:
            counts[0] = 0
        elif N:
            cloud[0, :, 1] = np.nan
    return cloud, counts, grid


def usable(cloud_b, n):
    p = np.asarray(cloud_b[:n], np.float32)
    return p[np.isfinite(p).all(axis=1)]


def build_restate(cloud, counts, grid, chunk=1 << 15):
    """-> d2min float64 [B,nz,ny,nx]: float32 differences, float64 squares and sum; +inf without a usable row."""
    cloud = np.asarray(cloud, np.float32)
    B, N = cloud.shape[:2]
    x, y, z = node_coordinates(grid)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    nodes = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1).astype(np.float32)  # [n,3], x fastest
    out = np.full((B, nodes.shape[0]), np.inf)
    for b in range(B):
        n = N if counts is None else int(min(max(int(counts[b]), 0), N))
        p = usable(cloud[b], n)
        if p.shape[0] == 0:
            continue
        for s in range(0, nodes.shape[0], chunk):
            d = (nodes[s:s + chunk, None, :] - p[None, :, :]).astype(np.float64)  # (the subtraction itself is float32)
            out[b, s:s + chunk] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).min(axis=1)
    return out.reshape(B, grid["nz"], grid["ny"], grid["nx"])


def nearest_distance(points, queries, upper=None, chunk=1 << 12):
    """float64 distance from every query [Q,3] to its nearest of points [n,3] (n > 0): a k-d tree where scipy is
    installed, chunked brute force where it is not.  ``upper``: distances above it may come back as +inf."""
    points, queries = np.asarray(points, np.float64), np.asarray(queries, np.float64)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        out = np.empty(queries.shape[0])
        for s in range(0, queries.shape[0], chunk):
            d = queries[s:s + chunk, None, :] - points[None, :, :]
            out[s:s + chunk] = np.sqrt((d * d).sum(-1).min(1))
        return out
    return cKDTree(points).query(queries, distance_upper_bound=np.inf if upper is None else upper * 1.001)[0]


def build_fast(cloud, counts, grid):
    """The field itself, float32 [B,nz,ny,nx], through a k-d tree in float64: the same values up to the rounding of the
    coordinate differences (not bit for bit; for the restatement of the PLANNER on grids too large for ``build_restate``)."""
    cloud = np.asarray(cloud, np.float32)
    B, N = cloud.shape[:2]
    x, y, z = node_coordinates(grid)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    nodes = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1).astype(np.float64)
    trunc = float(grid["trunc"])
    out = np.full((B, nodes.shape[0]), np.float32(trunc), np.float32)
    for b in range(B):
        n = N if counts is None else int(min(max(int(counts[b]), 0), N))
        p = usable(cloud[b], n)
        if p.shape[0]:
            out[b] = np.minimum(nearest_distance(p, nodes, trunc), trunc).astype(np.float32)
    return out.reshape(B, grid["nz"], grid["ny"], grid["nx"])


def check_field(field, d2min, trunc):
    """The banded rule, BAND on d2.  ``field`` float32 [B,nz,ny,nx].  The device returns fminf(sqrtf(best), trunc) with
    ``best`` within BAND of the float64 d2 and a correctly rounded, hence monotone, square root: so where d2 is below
    trunc^2 (1 - BAND) the value lies between float32(sqrt(d2 (1 - BAND))) and float32(sqrt(d2 (1 + BAND))), both cut at
    trunc -- "field^2 within BAND of the minimum" said without charging the square root's own half ulp to the band;
    where d2 is above trunc^2 (1 + BAND) it is exactly trunc; in between either.  -> how many nodes fell in each class."""
    f = np.asarray(field, np.float32)
    t = np.float32(trunc)
    t2 = float(t) ** 2
    below, above = d2min < t2 * (1 - BAND), d2min > t2 * (1 + BAND)
    assert np.isfinite(f).all() and (f <= t).all() and (f >= 0).all()
    assert (f[above] == t).all()
    with np.errstate(invalid="ignore"):
        lo = np.minimum(np.sqrt(d2min * (1 - BAND)).astype(np.float32), t)
        hi = np.minimum(np.sqrt(d2min * (1 + BAND)).astype(np.float32), t)
    inside = (f >= lo) & (f <= hi)
    assert inside[below].all(), float(np.abs(f.astype(np.float64)[below] ** 2 / d2min[below] - 1).max())
    mid = ~below & ~above
    assert (inside[mid] | (f[mid] == t)).all()
    return int(below.sum()), int(above.sum()), int(mid.sum())


# ---- the sampler ---------------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """a * b + c with one rounding in the dtype of a (float64: the plain expression)."""
    if a.dtype == torch.float32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def sample(field, grid, points, dtype=torch.float64, want_face=False):
    """field float32 [B,nz,ny,nx] (numpy or torch), points float32 [B,P,3] -> dist [B,P], grad [B,P,3] (torch, ``dtype``),
    inside bool [B,P] and, with ``want_face``, near_face bool [B,P]: a coordinate within FACE cells of a cell face (where
    the gradient is discontinuous and the two sides may pick different cells)."""
    f = torch.as_tensor(np.asarray(field, np.float32)).to(dtype)
    p = torch.as_tensor(np.asarray(points, np.float32)).to(dtype)
    B, P = p.shape[:2]
    n = torch.tensor([grid["nx"], grid["ny"], grid["nz"]])
    lo = torch.as_tensor(np.asarray(grid["lo"], np.float32)).to(dtype)
    inv_h = torch.tensor(float(np.float32(1.0) / np.float32(grid["h"]))).to(dtype)  # (float32 on the host, then widened)
    u = (p - lo) * inv_h  # [B,P,3]
    with np.errstate(invalid="ignore"):
        inside = (torch.isfinite(p).all(-1) & (u >= 0).all(-1) & (u <= (n - 1).to(dtype)).all(-1))
    us = torch.where(inside[..., None], u, torch.zeros_like(u))
    i0 = torch.minimum(torch.floor(us).long(), n - 2)
    fr = us - i0.to(dtype)
    fx, fy, fz = fr[..., 0], fr[..., 1], fr[..., 2]
    nx, ny, nz = grid["nx"], grid["ny"], grid["nz"]
    flat = f.reshape(B, -1)
    base = (i0[..., 2] * ny + i0[..., 1]) * nx + i0[..., 0]

    def corner(zz, yy, xx):
        return torch.gather(flat, 1, base + (zz * ny + yy) * nx + xx)

    c = [[[corner(zz, yy, xx) for xx in (0, 1)] for yy in (0, 1)] for zz in (0, 1)]
    X = [[c[zz][yy][1] - c[zz][yy][0] for yy in (0, 1)] for zz in (0, 1)]
    a = [[_fma(fx, X[zz][yy], c[zz][yy][0]) for yy in (0, 1)] for zz in (0, 1)]
    Y = [a[zz][1] - a[zz][0] for zz in (0, 1)]
    e = [_fma(fy, Y[zz], a[zz][0]) for zz in (0, 1)]
    Z = e[1] - e[0]
    dist = _fma(fz, Z, e[0])
    x0 = _fma(fy, X[0][1] - X[0][0], X[0][0])
    x1 = _fma(fy, X[1][1] - X[1][0], X[1][0])
    gx = inv_h * _fma(fz, x1 - x0, x0)
    gy = inv_h * _fma(fz, Y[1] - Y[0], Y[0])
    gz = inv_h * Z
    trunc = torch.tensor(float(np.float32(grid["trunc"]))).to(dtype)
    dist = torch.where(inside, dist, trunc)
    grad = torch.where(inside[..., None], torch.stack([gx, gy, gz], -1), torch.zeros_like(p))
    if not want_face:
        return dist, grad, inside
    ud = ((p.double() - lo.double()) * inv_h.double())
    near = ((ud - torch.round(ud)).abs() < FACE).any(-1) & inside
    return dist, grad, inside, near


def make_sample_points(grid, B, P, seed):
    """Seeded float32 [B,P,3]: uniform over the grid's box inflated by a tenth (so a share falls outside), then a NaN
    row, an infinite row, one point per axis exactly on the last node (u == n - 1) and one far away."""
    rng = np.random.default_rng(seed)
    x, y, z = node_coordinates(grid)
    lo = np.array([x[0], y[0], z[0]], np.float32)
    hi = np.array([x[-1], y[-1], z[-1]], np.float32)
    pad = np.float32(0.1) * (hi - lo)
    pts = (lo - pad + rng.random((B, P, 3), dtype=np.float32) * (hi - lo + 2 * pad)).astype(np.float32)
    pts[:, 0, 0] = np.nan
    pts[:, 1, 1] = np.inf
    pts[:, 2] = hi
    pts[:, 3] = (hi[0], lo[1], lo[2])
    pts[:, 4] = lo + np.float32(1000.0)
    return pts


# the grid and cloud of the sample tests: power-of-two spacing and lo on multiples of it, so that u is exact on nodes
SAMPLE_GRID = dict(shape=(19, 12, 9), lo=(-0.5, -0.25, 0.0), h=0.0625, trunc=0.3)
SAMPLE_B, SAMPLE_N, SAMPLE_P, SAMPLE_SEED = 2, 300, 4096, 77


def make_sample_case():
    grid = make_grid(SAMPLE_GRID["shape"], SAMPLE_GRID["lo"], SAMPLE_GRID["h"], SAMPLE_GRID["trunc"])
    rng = np.random.default_rng(SAMPLE_SEED)
    x, y, z = node_coordinates(grid)
    lo, hi = np.array([x[0], y[0], z[0]], np.float32), np.array([x[-1], y[-1], z[-1]], np.float32)
    cloud = (lo + rng.random((SAMPLE_B, SAMPLE_N, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    return grid, cloud, make_sample_points(grid, SAMPLE_B, SAMPLE_P, SAMPLE_SEED + 1)


def field_from_d2(d2min, trunc):
    """The field a correctly rounded device returns for the float64 minimum: float32(sqrt(d2)) cut at trunc."""
    with np.errstate(invalid="ignore"):
        return np.minimum(np.sqrt(d2min).astype(np.float32), np.float32(trunc))
