"""Truncated distance fields of point clouds on the GPU (csrc/cloud_field.hip): what ``robot.franka_plan_cloud`` steers by.

``CloudField.build`` turns one cloud per environment into a ``[B,nz,ny,nx]`` grid of distances to the nearest point, cut
at ``truncation``; ``.sample`` returns the trilinear interpolant and its gradient at arbitrary points.  The field is a
SURFACE field -- unsigned, with no inside -- and it only steers an optimiser: whether a configuration is free is
``FrankaCollisionSampler.check_cloud``'s question, asked of the cloud itself.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._operands import cloud_operand, counts_operand  # (cloud_operand: also this module's public name)

FIELD_MAX_SIDE = 1024  # MPX_FIELD_MAX_SIDE
FIELD_MAX_NODES = 1 << 24  # MPX_FIELD_MAX_NODES
# the reach box of the arm: what the cloud-collision tests crop to
DEFAULT_LO, DEFAULT_HI, DEFAULT_VOXEL = (-0.9, -0.9, -0.3), (0.9, 0.9, 1.2), 0.03


def make_grid(lo: Sequence[float], hi: Sequence[float], voxel: float, truncation: float) -> _lib.FieldGrid:
    """The grid that covers [lo, hi] with nodes ``voxel`` apart: node 0 on ``lo``, the last node on or past ``hi`` (to 1e-4 of
    a cell: the float32 images of the default box are 60 and 50 cells wide to 3e-6)."""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    if lo32.shape != (3,) or hi32.shape != (3,) or not (voxel > 0):
        raise _lib.MpxError("CloudField: lo and hi must have 3 entries and voxel must be > 0")
    h = float(np.float32(voxel))
    n = [max(2, int(math.ceil((float(hi32[a]) - float(lo32[a])) / h - 1e-4)) + 1) for a in range(3)]
    return _lib.FieldGrid((ctypes.c_float * 3)(*[float(v) for v in lo32]), h, n[0], n[1], n[2], float(truncation))


class CloudField:
    """``values`` float32 [B,nz,ny,nx] (x fastest) on the GPU and the ``grid`` (``_lib.FieldGrid``) they sit on."""

    def __init__(self, values: torch.Tensor, grid: _lib.FieldGrid):
        self.values, self.grid = values, grid

    @property
    def shape(self):
        return (self.grid.nz, self.grid.ny, self.grid.nx)

    @property
    def truncation(self) -> float:
        return float(self.grid.trunc)

    def node_coordinates(self):
        """-> (x [nx], y [ny], z [nz]) float32 numpy: the node positions as the device rounds them (one fma each)."""
        g = self.grid
        return tuple((np.arange(n, dtype=np.float64) * np.float64(np.float32(g.h)) + np.float64(np.float32(g.lo[a]))).astype(np.float32)
                     for a, n in enumerate((g.nx, g.ny, g.nz)))

    @classmethod
    def build(cls, cloud: torch.Tensor, counts: Optional[torch.Tensor] = None, lo: Sequence[float] = DEFAULT_LO,
              hi: Sequence[float] = DEFAULT_HI, voxel: float = DEFAULT_VOXEL, truncation: float = 0.25,
              grid: Optional[_lib.FieldGrid] = None, out: Optional[torch.Tensor] = None) -> "CloudField":
        """Distance of every grid node to the nearest point of its environment's cloud, cut at ``truncation``.

        :param cloud: [B,N,3] or [B,N,4] float32 on the GPU, any view whose last stride is 1 (``xyz[:, 2048:6144, :3]`` of
            the slab is read in place); rows with a NaN or infinite coordinate are ignored
        :param counts: optional int [B]: only the first ``counts[b]`` rows of environment b exist (clamped to [0, N])
        :param lo, hi, voxel: the box the grid covers and its node spacing [m]; ``grid`` (a ``_lib.FieldGrid``) replaces them
        :param truncation: the field saturates here [m]; an environment without usable points is ``truncation`` everywhere
        :param out: optional float32 [B,nz,ny,nx] contiguous tensor to fill
        """
        _lib.require_cuda(cloud, counts, out)
        N, bs, ps = cloud_operand("CloudField.build", cloud)
        B = cloud.size(0)
        g = grid if grid is not None else make_grid(lo, hi, voxel, truncation)
        cn = counts_operand(counts, B)
        shape = (B, max(g.nz, 0), max(g.ny, 0), max(g.nx, 0))
        if out is None:
            nodes = shape[1] * shape[2] * shape[3]
            out = torch.empty(shape if 0 < nodes <= FIELD_MAX_NODES else (B, 0, 0, 0), dtype=torch.float32, device=cloud.device)
        elif out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise _lib.MpxError(f"CloudField.build: out must be contiguous float32 {shape}")
        _lib.call("mpx_cloud_field_build", _lib.ptr(cloud), bs, ps, N, _lib.ptr(cn), B, ctypes.byref(g), _lib.ptr(out))
        return cls(out, g)

    def sample(self, points: torch.Tensor, return_grad: bool = False):
        """Trilinear interpolant of the field at ``points`` [B,P,3] (or [B,P,4], last stride 1) -> ``dist`` [B,P], and with
        ``return_grad`` its analytic gradient [B,P,3].  Outside the grid, or at a non-finite point: ``truncation`` and 0."""
        _lib.require_cuda(points, self.values)
        B = self.values.size(0)
        P, bs, ps = cloud_operand("CloudField.sample", points, B)
        dist = torch.empty((B, P), dtype=torch.float32, device=points.device)
        grad = torch.empty((B, P, 3), dtype=torch.float32, device=points.device) if return_grad else None
        _lib.call("mpx_cloud_field_sample", _lib.ptr(self.values), ctypes.byref(self.grid), B, _lib.ptr(points), bs, ps, P,
                  _lib.ptr(dist), _lib.ptr(grad))
        return (dist, grad) if return_grad else dist
