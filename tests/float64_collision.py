"""Restatement of the primitive collision sweep (csrc/franka.hip, ``mpx_franka_collision``) on the CPU in float64, its
launcher's routing as the library reports it, and the shapes and seeded inputs of tests/test_gpu_collision_forms.py.

``restate`` works from what the kernel itself works from: FLOAT32 sphere centres (``FrankaCollisionSampler.sphere_centers``,
which the sweep reproduces bit for bit) and the float32 inverse frames the device produced (``TorchCuboids.inv_frames``);
on a machine without a GPU the oracle's FK centres and the oracle's frames stand in (``cpu_inputs``).  Rows 0..2 of a
frame ([R | Rt]) take the centre into the primitive's frame; a cuboid's distance is the norm of the positive parts of
``|p| - d/2`` plus the clamped largest component, a cylinder's the same over ``(rho - r, |z| - h/2)``; a primitive with
any size ``|x| <= 1e-8`` is masked to +inf; the result is the minimum over all primitives.  Nothing here shares code
with the kernel or with oracle/mpn_oracle.c.

``SDF_BAR`` is the reference against itself: 4 x the largest |float32 run - float64 run| of ``restate`` over every finite
entry of every case below (the factor follows tests/float64_metrics.py).  tests/test_collision_host.py measures the gap
again and holds the constant inside a 2x..8x window of it.

  measured gap (oracle frames and centres, all 36 CASES): 2.25e-07 m     SDF_BAR = 9.0e-07 m

Decisions: with ``m = sdf64 - radius[s]`` an environment is a definite hit when some pair has ``m < -SDF_BAR``, undecided
when it has no definite hit and some pair has ``|m| <= SDF_BAR``, else a definite miss.  Undecided environments are left
out of the flag comparison; ``UNDECIDED_CAP`` bounds their share per case (a condition, not a measurement).
"""
from collections import namedtuple

import numpy as np

from launch_routes import collision_fields, collision_route as route  # noqa: F401  (the launcher's own routing)

MEASURED_GAP = 2.25e-07   # largest |restate32 - restate64| over the finite entries of all CASES (see the module docstring)
SDF_BAR = 9.0e-07         # = 4 x MEASURED_GAP, metres
UNDECIDED_CAP = 0.02      # share of a case's environments that may be undecided


def env_form():
    """-> (threads, waypoints per chunk) of the per-environment 256-thread form, as the library reports them."""
    form, _, threads, tc, _, _ = collision_fields(2, 64, 56, 16, 16)
    assert form == 3
    return threads, tc


ROUTES = ("general", "wave") + tuple("ppt%d" % p for p in range(2, 17, 2))
FORMS = ("full", "flags_only")  # min_sdf given / NULL: every case runs in both (tests/test_gpu_collision_forms.py)

# table: "S56" / "S57" = the robot's own table without / with the base link (FrankaCollisionSampler); ("tile", S) = S rows of
# the 56-sphere table (spread over it for S < 56, repeated for S > 56), each moved by a small seeded offset -- through
# the raw entry point.  edge: a scene edit applied to the generated scene (see ``_edit_scene``).
Case = namedtuple("Case", "B T table kinds M1 M2 edge", defaults=(None,))
_TC, _TCD = ("tabletop", "cubby"), ("tabletop", "cubby", "dresser")

CASES = (
    # S = 56: both ends of the T range of every pairs-per-thread form, then two and three chunks
    [Case(3, 1, "S56", _TC, 16, 16)]
    + [Case(2 + i % 4, T, "S56", _TCD if i % 2 else _TC, 40 if i % 2 else 16, 16)
       for i, T in enumerate((2, 9, 10, 18, 19, 27, 28, 36, 37, 45, 46, 54, 55, 64, 65, 130))]
    # S = 57: the 16-pairs form from 63 waypoints on; 129 = two full chunks and one waypoint
    + [Case(3, T, "S57", _TCD, 40, 16) for T in (1, 63, 64, 129)]
    # custom tables
    + [Case(3, 64, ("tile", 64), _TC, 16, 16),   # every thread holds 16 live pairs, dr = 0
       Case(4, 1, ("tile", 64), _TC, 16, 16),    # one full wave
       Case(3, 64, ("tile", 1), _TC, 16, 16),    # 64 FK lanes, one pair each
       Case(3, 65, ("tile", 1), _TC, 16, 16),    # the second chunk holds one pair
       Case(4, 8, ("tile", 33), _TCD, 40, 16),
       Case(3, 3, ("tile", 65), _TC, 16, 16),    # general: S > 64
       # two chunks with a ragged last one (< 256 pairs) in the forms S = 56 / 57 cannot reach with T > 64
       Case(3, 66, ("tile", 16), _TC, 16, 16),   # ppt4, last chunk 32 pairs
       Case(3, 67, ("tile", 24), _TCD, 40, 16),  # ppt6, 72
       Case(3, 65, ("tile", 32), _TC, 16, 16),   # ppt8, 32
       Case(3, 69, ("tile", 40), _TCD, 40, 16),  # ppt10, 200
       Case(3, 66, ("tile", 48), _TC, 16, 16)]   # ppt12, 96
    + [Case(70, 50, "S56", _TCD, 40, 16),
       Case(3, 9, "S56", _TCD, 70, 16),          # general: M1 > 64
       Case(2, 2, "S56", _TC, 16, 65),           # general: M2 > 64
       Case(5, 19, "S56", _TCD, 64, 16, "edges")]
)


def case_id(case):
    S = {"S56": 56, "S57": 57}.get(case.table) or case.table[1]
    tag = "" if case.table in ("S56", "S57") else "tile"
    return f"B{case.B}-T{case.T}-S{S}{tag}-M{case.M1}x{case.M2}" + (f"-{case.edge}" if case.edge else "")


def num_spheres(case):
    return {"S56": 56, "S57": 57}.get(case.table) or case.table[1]


def case_route(case, aligned=True):
    return route(case.B, case.T, num_spheres(case), case.M1, case.M2, aligned)


def case_seed(case):
    return 2000 + CASES.index(case)


def sphere_table(case):
    """-> centres float32 [S,3] (link frame), radii float32 [S], links int32 [S]."""
    from mpinets_amd import franka_tables as ft

    if case.table in ("S56", "S57"):
        c, r, l, _ = ft.collision_sphere_table(case.table == "S57")
        return c.copy(), r.copy(), l.copy()
    S = case.table[1]
    c, r, l, _ = ft.collision_sphere_table(False)
    rows = np.arange(S) * 56 // S if S < 56 else np.arange(S) % 56
    rng = np.random.default_rng(7000 + S)
    off = rng.uniform(-0.01, 0.01, (S, 3)).astype(np.float32)
    return (c[rows] + off).astype(np.float32), r[rows].copy(), l[rows].copy()


def _edit_scene(scn, seed):
    """The scene edges (5 environments, M1 = 64): 0 no live cylinder, 1 no live cuboid, 2 nothing live, 3 exactly 64 live
    cuboids, 4 live and zero-size rows interleaved (compaction moves every live row: a zero-size row comes first)."""
    rng = np.random.default_rng(seed)
    cc, cd, cq = scn["cuboid_centers"], scn["cuboid_dims"], scn["cuboid_quats"]
    yc, yr, yh, yq = scn["cylinder_centers"], scn["cylinder_radii"], scn["cylinder_heights"], scn["cylinder_quats"]
    M1, M2 = cd.shape[1], yr.shape[1]

    def boxes(n):
        c = rng.uniform([0.2, -0.7, 0.0], [0.9, 0.7, 0.9], (n, 3))
        d = rng.uniform(0.03, 0.12, (n, 3))
        yaw = rng.uniform(0, np.pi, n)
        q = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1)
        return c.astype(np.float32), d.astype(np.float32), q.astype(np.float32)

    yr[0] = 0.0                                  # 0: cylinders with a height but no radius
    cd[1, :, 1] = 0.0                            # 1: every cuboid flat along y
    c, d, q = boxes(M2)
    yc[1], yr[1, :, 0], yh[1, :, 0], yq[1] = c, d[:, 0], d[:, 1] * 3, q   # ... and 16 live cylinders
    cd[2], yh[2] = 0.0, 0.0                      # 2: nothing live
    dead = np.abs(cd[3]).min(axis=1) <= 1e-8     # 3: every dead row becomes a small box
    c, d, q = boxes(int(dead.sum()))
    cc[3, dead], cd[3, dead], cq[3, dead] = c, d, q
    live = np.flatnonzero(np.abs(cd[4]).min(axis=1) > 1e-8)[: M1 // 2]    # 4: live rows at 1, 3, 5, ..., zero rows between
    c4, d4, q4 = cc[4, live].copy(), cd[4, live].copy(), cq[4, live].copy()
    cd[4] = 0.0
    cc[4, 1:2 * len(live):2], cd[4, 1:2 * len(live):2], cq[4, 1:2 * len(live):2] = c4, d4, q4
    c, d, q = boxes(M2 // 2)
    yr[4], yh[4] = 0.0, 0.0
    yc[4, 1::2], yr[4, 1::2, 0], yh[4, 1::2, 0], yq[4, 1::2] = c, d[:, 0], d[:, 1] * 3, q
    return scn


def make_case(case):
    """-> q float32 [B,T,7] (straight joint-space lines), the scene (numpy dict of ``scenes.make_scenes``) and the sphere
    table (centres, radii, links); seeded by the case's position in CASES."""
    from mpinets_amd import scenes

    seed = case_seed(case)
    scn = scenes.make_scenes(case.B, seed, case.kinds, case.M1, case.M2)
    if case.edge == "edges":
        assert case.B == 5 and case.M1 == 64
        scn = _edit_scene(scn, seed)
    q = scenes.linear_trajectories(case.B, case.T, seed + 1)
    return q, scn, sphere_table(case)


def cpu_inputs(case):
    """Everything ``restate`` needs, made without a GPU: (centres [B,T,S,3], cub_frames [B,M1,4,4], cub_dims, cyl_frames,
    cyl_radii, cyl_heights), radii [S] and the scene."""
    from oracle import oracle as orc

    q, scn, (c, r, l) = make_case(case)
    fr = orc.franka_fk(q.reshape(-1, 7))
    centres = orc.transform_table(fr, c, l).reshape(case.B, case.T, -1, 3)
    args = (centres, orc.inv_frames_4x4(scn["cuboid_centers"], scn["cuboid_quats"]), scn["cuboid_dims"],
            orc.inv_frames_4x4(scn["cylinder_centers"], scn["cylinder_quats"]), scn["cylinder_radii"], scn["cylinder_heights"])
    return args, r, scn


def _is_zero(x):
    return np.abs(np.asarray(x, np.float32)) <= np.float32(1e-8)  # the float32 test of the kernel (torch.isclose(x, 0))


def restate(centres, cub_frames, cub_dims, cyl_frames, cyl_radii, cyl_heights, dtype=np.float64):
    """centres float32 [B,T,S,3]; frames float32 [B,M,4,4]; dims [B,M1,3]; radii, heights [B,M2] or [B,M2,1]
    -> min over all primitives of the signed distance, ``dtype`` [B,T,S] (+inf where the environment has no live one)."""
    centres = np.asarray(centres, np.float32)
    B, T, S, _ = centres.shape
    out = np.full((B, T, S), np.inf, dtype)
    zero = dtype(0)

    def local(frames, p):  # rows 0..2 of [M,4,4] applied to p [P,3] -> [M,P,3]
        f = np.asarray(frames, np.float32).astype(dtype)
        return np.einsum("mij,pj->mpi", f[:, :3, :3], p) + f[:, None, :3, 3]

    for b in range(B):
        p = centres[b].reshape(-1, 3).astype(dtype)
        best = np.full(p.shape[0], np.inf, dtype)
        dims = np.asarray(cub_dims[b], np.float32).reshape(-1, 3)
        live = ~_is_zero(dims).any(axis=1)
        if live.any():
            d = np.abs(local(cub_frames[b][live], p)) - (dims[live].astype(dtype) / dtype(2))[:, None, :]
            sdf = np.sqrt((np.maximum(d, zero) ** 2).sum(axis=2)) + np.minimum(d.max(axis=2), zero)
            best = np.minimum(best, sdf.min(axis=0))
        rad = np.asarray(cyl_radii[b], np.float32).reshape(-1)
        hgt = np.asarray(cyl_heights[b], np.float32).reshape(-1)
        live = ~(_is_zero(rad) | _is_zero(hgt))
        if live.any():
            x = local(cyl_frames[b][live], p)
            rho = np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2)
            d = np.stack([rho - rad[live].astype(dtype)[:, None], np.abs(x[..., 2]) - (hgt[live].astype(dtype) / dtype(2))[:, None]], -1)
            sdf = np.sqrt((np.maximum(d, zero) ** 2).sum(axis=2)) + np.minimum(d.max(axis=2), zero)
            best = np.minimum(best, sdf.min(axis=0))
        out[b] = best.reshape(T, S)
    return out


def decide(sdf64, radii, bar=SDF_BAR):
    """-> (hit, undecided) bool [B] from the float64 distances [B,T,S] and the sphere radii [S]."""
    m = (np.asarray(sdf64, np.float64) - np.asarray(radii, np.float64)[None, None, :]).reshape(sdf64.shape[0], -1)
    hit = (m < -bar).any(axis=1)
    return hit, ~hit & (np.abs(m) <= bar).any(axis=1)


def offending_envs(got, ref64, bar=SDF_BAR):
    """The comparator of the GPU test: environments where ``got`` [B,T,S] has another +inf pattern than the float64
    reference or a finite entry further than ``bar`` from it; also the worst finite error."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    inf_g, inf_r = np.isposinf(got), np.isposinf(ref64)
    both = np.isfinite(got) & np.isfinite(ref64)
    err = np.where(both, np.abs(np.where(both, got, 0.0) - np.where(both, ref64, 0.0)), 0.0)
    bad = (inf_g != inf_r) | (~both & ~(inf_g & inf_r)) | (err > bar)
    return set(np.flatnonzero(bad.reshape(got.shape[0], -1).any(axis=1)).tolist()), float(err.max()) if err.size else 0.0


def measure_reference_gap(cases=None):
    """Largest |float32 run - float64 run| of ``restate`` over the finite entries of every case, oracle frames and centres."""
    gap = 0.0
    for case in CASES if cases is None else cases:
        args, _, _ = cpu_inputs(case)
        a, b = restate(*args, dtype=np.float64), restate(*args, dtype=np.float32)
        assert np.array_equal(np.isposinf(a), np.isposinf(b))
        fin = np.isfinite(a)
        if fin.any():
            gap = max(gap, float(np.abs(a[fin] - b[fin].astype(np.float64)).max()))
    return gap
