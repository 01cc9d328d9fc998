"""What the launchers themselves say they launch: thin wrappers over the library's route queries (mpx_*_route,
include/mpinets_hip.h; the launchers plan with the same functions, csrc/launch_routes.h).  No GPU is needed and nothing is
launched.  A plain module, imported by the tests: it holds no test of its own."""
import ctypes
from collections import namedtuple

MPX_VARIANT_FPS, MPX_VARIANT_BALL_QUERY = 0, 1  # selectors of mpx_set_variant
FPS_MAX_N = 8192                                # "N <= 8192" of mpx_fps in the header
SaRoute = namedtuple("SaRoute", "packed Q lpool units per_env persistent slots resident one_env xcd_aware")
WgradRoute = namedtuple("WgradRoute", "tile splits rows_per_split")


def _query(name, n, *args):
    from mpinets_amd import _lib

    out = (ctypes.c_int32 * n)()
    assert getattr(_lib.load(), name)(*args, out) == 0
    return list(out)


def fps_fields(B, N, variant=1):
    """-> [family, points per lane, threads, LDS bytes] of ``mpx_fps`` with the MPX_VARIANT_FPS switch at ``variant`` (put
    back to what it was)."""
    from mpinets_amd import _lib

    lib = _lib.load()
    was = lib.mpx_get_variant(MPX_VARIANT_FPS)
    assert lib.mpx_set_variant(MPX_VARIANT_FPS, variant) == 0
    try:
        return _query("mpx_fps_route", 4, B, N)
    finally:
        assert lib.mpx_set_variant(MPX_VARIANT_FPS, was) == 0


def fps_route(B, N, variant=1):
    """-> ("wave" | "cull8" | "cull4" | "plain", P): the kernel family and the points-per-lane instantiation of ``mpx_fps``."""
    family, pts, _, _ = fps_fields(B, N, variant)
    return ("plain", "wave", "cull8", "cull4")[family], pts


def collision_fields(B, T, S, M1, M2, aligned=True):
    """-> [form, pairs per thread, threads, waypoints per chunk, chunks (general: workgroups), pairs of the last one]."""
    return _query("mpx_franka_collision_route", 6, B, T, S, M1, M2, int(aligned))


def collision_route(B, T, S, M1, M2, aligned=True):
    """-> (name, chunks, last): the kernel ``mpx_franka_collision`` launches for this shape -- "general", "wave" or
    "ppt2" .. "ppt16" -- the number of waypoint chunks per environment and the (waypoint, sphere) pairs of the last
    chunk.  For the general kernel: the number of workgroups and the pairs of the last one.  None where nothing is
    launched.  The flags-only form (``min_sdf == NULL``) takes the same route."""
    form, ppt, _, _, chunks, last = collision_fields(B, T, S, M1, M2, aligned)
    return None if form == 0 else (("general", "wave", "ppt%d" % ppt)[form - 1], chunks, last)


def linear_route(M, N, K):
    """"gemv" | "tile" | "split-K": the kernel ``pointnet2.linear`` (mpx_linear / mpx_linear_ws) runs."""
    return ("gemv", "tile", "split-K")[_query("mpx_linear_route", 3, M, N, K)[0]]


def linear_form(x, ldx, w, bias, M, N, K, act, y, ldy):
    """-> (route, rowlane, dma) of ``mpx_linear`` for exactly these operands (addresses as integers, None = NULL): the
    ``linear_route`` name, whether the row-per-lane kernel is launched, whether the first slab's tile kernel stages by DMA."""
    form, rowlane, dma = _query("mpx_linear_form", 3, x, ldx, w, bias, M, N, K, act, y, ldy)
    return ("gemv", "tile", "split-K")[form], bool(rowlane), bool(dma)


def wgrad_route(M, N, K):
    return WgradRoute(*_query("mpx_linear_wgrad_route", 3, M, N, K))


def pool_wgrad_splits(Q, C, K):
    return _query("mpx_pool_wgrad_route", 1, Q, C, K)[0]


def sa_route(cus, B, npoint, nsample, counts, C, precision, factored, out_aligned=True):
    return SaRoute(*_query("mpx_sa_mlp_route", 10, cus, B, npoint, nsample, int(counts), C, int(precision == "bf16x3"),
                           int(factored), int(out_aligned)))
