"""Operand rules of the robot-geometry wrappers (``robot``, ``solvers``, ``capture``, ``field``), each stated once: single
operands (cloud, counts, limits, scratch), the argument blocks the Franka entries share (sphere table and primitives, cloud,
options / seed / env_offset) and the merge of keyword options into a C options struct.  C side: csrc/franka_host.h."""
from __future__ import annotations

import ctypes
from operator import itemgetter
from typing import Dict, Optional

import torch

from . import _lib
from . import franka_tables as ft

_scratch: Dict[Optional[int], torch.Tensor] = {}
_sphere_tables: dict = {}


def cloud_operand(who: str, cloud: torch.Tensor, B: Optional[int] = None, empty_batch_any_stride: bool = True):
    """A ``[B,N,3]`` / ``[B,N,4]`` float32 view whose last stride is 1 -> (N, batch stride, point stride) in floats, read
    in place.  A one-row view may carry any row stride, and so may an empty batch: the rule, and what a new entry gets.
    ``empty_batch_any_stride=False`` is only for ``check_cloud``, ``check_cloud_each`` and ``clean_point_clouds``: they have
    always handed a row stride below 3 (an ``expand`` view) to C at B = 0 too, where it is refused, and still do."""
    shape = cloud.shape  # (one call each for the shape and the strides: this runs in front of every launch)
    if len(shape) != 3 or shape[2] not in (3, 4) or cloud.dtype != torch.float32 or (B is not None and shape[0] != B):
        raise _lib.MpxError(f"{who}: cloud must be float32 [B{'' if B is None else '=' + str(B)},N,3] or [B,N,4], "
                            f"got {cloud.dtype} {tuple(shape)}")
    nb, N, _ = shape
    bs, ps, last = cloud.stride()
    if N > 0 and nb > 0 and last != 1:
        raise _lib.MpxError(f"{who}: the cloud's last dimension must have stride 1")
    as_is = N > 1 and (nb > 0 or not empty_batch_any_stride)
    return N, bs, ps if as_is else max(ps, 3)


def counts_operand(counts: Optional[torch.Tensor], B: int) -> Optional[torch.Tensor]:
    """``counts`` -> contiguous int32 [B], or None."""
    if counts is None:
        return None
    assert counts.shape == (B,)
    return _lib.i32c(counts)


def limits_operand(limits, device: torch.device) -> torch.Tensor:
    """[7,2] limits -> float32 on ``device``, rounded INWARD: a joint clamped onto a limit is inside the limits as passed."""
    lim = torch.from_numpy(ft.limits_float32_inward(limits.detach().cpu().numpy() if torch.is_tensor(limits) else limits)).to(device)
    assert lim.shape == (7, 2)
    return lim


def scratch_for(device: torch.device, nbytes: int) -> torch.Tensor:
    """The one growing scratch buffer of a GPU, at least ``nbytes`` (and 16: the entries want an aligned pointer even when
    they need nothing).  Every entry's work is ordered on the stream, so they share it; fetch it right before the call that
    uses it: a later fetch may replace it by a larger one."""
    buf = _scratch.get(device.index)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch[device.index] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    return buf


def sphere_table(device: torch.device, with_base_link: bool):
    """The collision-sphere table of ``franka_tables`` on ``device`` -> (centres, radii, links), made once per device."""
    key = (device, bool(with_base_link))
    if key not in _sphere_tables:
        c, r, l, _ = ft.collision_sphere_table(with_base_link)
        _sphere_tables[key] = tuple(torch.from_numpy(a).to(device) for a in (c, r, l))
    return _sphere_tables[key]


# The blocks below return call ARGUMENTS (pointers as plain integers) and, second, the tensors behind those that may be
# copies made here: the caller keeps that second value in a local until its ``_lib.call`` returns.


def sphere_primitive_args(cuboids, cylinders, B: Optional[int] = None, device: Optional[torch.device] = None,
                          with_base_link: bool = False, table=None):
    """-> the eleven arguments ``sph_centers, sph_radii, sph_link, S, cub_inv_frames, cub_dims, M1, cyl_inv_frames,
    cyl_radii, cyl_heights, M2`` of an entry that tests spheres against ``geometry.TorchCuboids`` / ``TorchCylinders`` (batch
    ``B`` where given, or None), and what to hold.  ``table``: a sampler's own (centres, radii, links), always passed;
    without one the cached table of ``device`` is passed where there is a primitive to test, and S = 0 where there is none."""
    cub, cyl, held = (None, None, 0), (None, None, None, 0), ()
    if cuboids is not None:
        assert B is None or cuboids.centers.size(0) == B
        cf, cd = held = cuboids.inv_frames, _lib.f32c(cuboids.dims)
        cub = cf.data_ptr(), cd.data_ptr(), cuboids.centers.size(1)
    if cylinders is not None:
        assert B is None or cylinders.centers.size(0) == B
        yf, yr, yh = cylinders.inv_frames, _lib.f32c(cylinders.radii), _lib.f32c(cylinders.heights)
        cyl, held = (yf.data_ptr(), yr.data_ptr(), yh.data_ptr(), cylinders.centers.size(1)), held + (yf, yr, yh)
    if table is None:
        if cub[2] + cyl[3] == 0:
            return (None, None, None, 0) + cub + cyl, held
        table = sphere_table(device, with_base_link)
    c, r, l = table
    return (c.data_ptr(), r.data_ptr(), l.data_ptr(), c.size(0)) + cub + cyl, (table, held)


def cloud_args(who: str, cloud: torch.Tensor, counts: Optional[torch.Tensor], B: int, point_radius: float,
               empty_batch_any_stride: bool = True, row: int = 0, null_without_points: bool = False):
    """-> the six arguments ``cloud, cloud_batch_stride, cloud_point_stride, N, counts, point_radius`` of an entry that reads
    one cloud per environment (``cloud_operand``'s and ``counts_operand``'s rules), from environment ``row`` on, and what to
    hold.  ``null_without_points``: ``mpx_franka_ik_cloud`` is handed NULL for a cloud of no rows."""
    N, bs, ps = cloud_operand(who, cloud, B, empty_batch_any_stride)
    cn = counts_operand(counts, B)
    return (None if null_without_points and N == 0 else cloud.data_ptr() + 4 * row * bs, bs, ps, N,
            None if cn is None else cn.data_ptr() + 4 * row, float(point_radius)), cn


def options_tail(copt: ctypes.Structure, seed: int, env_offset: int):
    """-> the three arguments ``options, seed, env_offset`` of a solver entry (the seed as the uint64 the draws are keyed by)."""
    return ctypes.byref(copt), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_offset)


def _self_flag(v) -> int:
    return int(bool(v))


# struct -> (the values of its fields out of an options dict, the cast of each), in field order: the option names are the
# struct's field names, but ``damping`` (C: ``lambda``) where the struct has no ``damping`` of its own (the follower has:
# its ``lambda_`` keeps its name)
_OPTION_FIELDS = {
    s: (itemgetter(*("damping" if n == "lambda_" and "damping" not in dict(s._fields_) else n for n, _ in s._fields_)),
        tuple(_self_flag if n in ("check_self", "test_self") else float if t is ctypes.c_float else int for n, t in s._fields_))
    for s in (_lib.IkOptions, _lib.PlanOptions, _lib.RoadmapOptions, _lib.ShortcutOptions, _lib.GripperRoadmapOptions,
              _lib.GripperShortcutOptions, _lib.FollowOptions, _lib.TaskCandidatesOptions)}


def merge_options(who: str, struct, defaults: dict, options: dict):
    """Keyword ``options`` over ``defaults`` (one value per field of ``struct``, of the field's type; never written) -> the
    filled ctypes struct and the merged dict, read-only: its values as the caller gave them, not yet float32.  Without
    options that dict is ``defaults`` itself (most calls pass none: nothing to merge, nothing to cast)."""
    values, casts = _OPTION_FIELDS[struct]
    if not options:
        return struct(*values(defaults)), defaults
    if not options.keys() <= defaults.keys():
        raise TypeError(f"{who}: unknown option(s) {sorted(options.keys() - defaults.keys())}")
    o = dict(defaults, **options)
    return struct(*[cast(v) for cast, v in zip(casts, values(o))]), o
