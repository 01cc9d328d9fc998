"""Operand rules of the robot-geometry wrappers (``robot``, ``capture``, ``field``), each stated once; C side: csrc/franka_host.h."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib
from . import franka_tables as ft

_scratch: Dict[Optional[int], torch.Tensor] = {}


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
