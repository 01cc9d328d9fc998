"""PointNet++ op seam: drop-in for ``pointnet2_ops`` as the reference uses it.

Reference call sites: ``from pointnet2_ops.pointnet2_modules import PointnetSAModule``
(mpinets/model.py:27), constructed at model.py:366-383, called at model.py:423-424 with
``xyz [B,N,3]`` contiguous and ``features [B,C,N]`` contiguous; returns
``(new_xyz [B,npoint,3] | None, new_features [B,mlp[-1],npoint])``.  xyz is concatenated before
the features (3 extra input channels), ``bn=False`` gives Conv2d(bias=True)+ReLU per layer, and the
state-dict keys are ``mlps.0.{0,2,4}.{weight,bias}`` ([EXT-RECALL]).

All compute runs in ``libmpinets_hip.so``; CPU tensors are rejected like in the reference
(model.py:417 "CPU tensors not supported").
"""
from __future__ import annotations

from typing import Any, Callable, List, Optional, Tuple

import torch
from torch import nn

from . import _lib


# ---- functional ops (pointnet2_utils equivalents) --------------------------------------------------
def furthest_point_sample(xyz: torch.Tensor, npoint: int, return_xyz: bool = False):
    """xyz [B,N,3|4] float32 (rows may be slab rows: only the first three columns are read)
    -> idx int32 [B,npoint] (and new_xyz [B,npoint,3])."""
    _lib.require_cuda(xyz)
    assert xyz.ndim == 3 and xyz.size(2) >= 3 and xyz.dtype == torch.float32 and xyz.is_contiguous()
    B, N, S = xyz.shape
    idx = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device)
    new_xyz = torch.empty((B, npoint, 3), dtype=torch.float32, device=xyz.device) if return_xyz else None
    _lib.call("mpx_fps", _lib.ptr(xyz), B, N, S, npoint, _lib.ptr(idx), _lib.ptr(new_xyz), 3)
    return (idx, new_xyz) if return_xyz else idx


def gather_operation(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """features [B,C,N], idx [B,npoint] -> [B,C,npoint] (index plumbing, torch)."""
    return torch.gather(features, 2, idx.long().unsqueeze(1).expand(-1, features.size(1), -1))


def ball_query(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor, return_counts: bool = False):
    """-> idx int32 [B,npoint,nsample] (argument order of pointnet2_utils.ball_query); with
    ``return_counts`` also the number of real hits per query (slots beyond it are padding)."""
    _lib.require_cuda(xyz, new_xyz)
    assert xyz.is_contiguous() and new_xyz.is_contiguous()
    B, N, S = xyz.shape
    npoint = new_xyz.size(1)
    idx = torch.empty((B, npoint, nsample), dtype=torch.int32, device=xyz.device)
    cnt = torch.empty((B, npoint), dtype=torch.int32, device=xyz.device) if return_counts else None
    _lib.call("mpx_ball_query", _lib.ptr(new_xyz), new_xyz.size(2), _lib.ptr(xyz), S, B, N, npoint,
              float(radius), nsample, _lib.ptr(idx), _lib.ptr(cnt))
    return (idx, cnt) if return_counts else idx


def query_and_group(xyz: torch.Tensor, new_xyz: torch.Tensor, features_pm: Optional[torch.Tensor],
                    idx: torch.Tensor) -> torch.Tensor:
    """Materialised QueryAndGroup(use_xyz=True): -> [B,3+C,npoint,nsample].
    ``features_pm`` is point-major [B,N,C]."""
    B, N, S = xyz.shape
    npoint, nsample = idx.shape[1:]
    C = 0 if features_pm is None else features_pm.size(2)
    out = torch.empty((B, 3 + C, npoint, nsample), dtype=torch.float32, device=xyz.device)
    _lib.call("mpx_group_points", _lib.ptr(xyz), S, _lib.ptr(new_xyz), new_xyz.size(2), _lib.ptr(features_pm),
              C if features_pm is None else features_pm.stride(1), C, _lib.ptr(idx), B, N, npoint, nsample,
              _lib.ptr(out))
    return out


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = act(x @ weight.T + bias) on the fp32 matrix cores.  x [M,K] (row stride may exceed K),
    weight [N,K].  ``out`` may be a column slice of a wider row-major buffer."""
    assert x.ndim == 2 and weight.ndim == 2 and x.size(1) == weight.size(1)
    assert x.stride(1) == 1 and weight.is_contiguous()
    M, K = x.shape
    N = weight.size(0)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    need = _lib.load().mpx_linear_workspace(M, N, K)
    if need == 0:
        _lib.call("mpx_linear", _lib.ptr(x), x.stride(0), _lib.ptr(weight), _lib.ptr(bias), M, N, K, act,
                  _lib.ptr(out), out.stride(0))
    else:  # skinny problem: split K over the CUs through a per-(device, stream) workspace (stream-ordered reuse)
        key = (x.device, _lib.stream_ptr())
        ws = _WORKSPACE.get(key)
        if ws is None or ws.numel() < need:
            ws = _WORKSPACE[key] = torch.empty(max(need, 16 << 20), dtype=torch.uint8, device=x.device)
        _lib.call("mpx_linear_ws", _lib.ptr(x), x.stride(0), _lib.ptr(weight), _lib.ptr(bias), M, N, K, act,
                  _lib.ptr(out), out.stride(0), _lib.ptr(ws), ws.numel())
    return out


_WORKSPACE = {}


def split_pairs(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 rows [R, K] -> the ``bf16x3`` kernels' PAIRS form [R, 2 * roundup(K, 16)] bf16: per group of 16 k-values
    [hi x 16 | lo x 16], hi = bf16(v), lo = bf16(v - hi), zero padded."""
    assert x.ndim == 2 and x.stride(1) == 1 and x.dtype == torch.float32
    R, K = x.shape
    Kp = (K + 15) // 16 * 16
    if out is None:
        out = torch.empty((R, 2 * Kp), dtype=torch.bfloat16, device=x.device)
    assert out.shape == (R, 2 * Kp) and out.stride(1) == 1
    _lib.call("mpx_split_bf16", _lib.ptr(x), x.stride(0), R, K, _lib.ptr(out), out.stride(0))
    return out


class DerivedWeights:
    """Tensors derived from parameters (kernel weight packs, ``bf16x3`` pairs, padded copies), one entry per derived
    tensor under a name saying what it is.  An entry is rebuilt when the (data_ptr, _version, shape) of any tensor it
    was made from has changed.  It keeps those tensors referenced, so their memory cannot pass to another tensor that
    would match the key.  Writes through ``param.data`` do not bump the version: ``clear()`` after them."""

    def __init__(self):
        self._entries = {}

    def entry(self, name, sources, make: Callable[[], Any]):
        """The entry ``name``, made by ``make()`` from ``sources`` unless it was made from them as they are now."""
        key = [(t.data_ptr(), t._version, t.shape) for t in sources]
        hit = self._entries.get(name)
        if hit is None or hit[0] != key:
            hit = self._entries[name] = (key, sources, make())
        return hit[2]

    def __contains__(self, name) -> bool:
        return name in self._entries

    def clear(self) -> None:
        self._entries.clear()


class SplitWeights(DerivedWeights):
    """Dense weight matrices in the pairs form for the ``bf16x3`` mode."""

    def get(self, weight: torch.Tensor, source: Optional[torch.Tensor] = None, name=None) -> torch.Tensor:
        """``weight`` [N, K] in the pairs form.  ``source``: the parameter a derived matrix (padded / reshaped copy) was
        made from (default: ``weight``); ``name``: what the matrix is, e.g. its layer (default: ``source``)."""
        src = weight if source is None else source
        return self.entry(src if name is None else name, (src,), lambda: split_pairs(_lib.f32c(weight.detach())))


def linear_x3(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int, split: SplitWeights,
              out: Optional[torch.Tensor] = None, source: Optional[torch.Tensor] = None, name=None) -> torch.Tensor:
    """``linear`` on the bf16 matrix cores (three split products per fp32 product, fp32 accumulate); ``source``,
    ``name``: see ``SplitWeights.get``."""
    assert x.ndim == 2 and weight.ndim == 2 and x.size(1) == weight.size(1) and x.stride(1) == 1
    M, K = x.shape
    N = weight.size(0)
    wp = split.get(weight, source, name)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    assert out.shape == (M, N) and out.stride(1) == 1
    _lib.call("mpx_linear_bf16x3", _lib.ptr(x), x.stride(0), _lib.ptr(wp), _lib.ptr(bias), M, N, K, act, _lib.ptr(out),
              out.stride(0))
    return out


def groupnorm_leaky(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int, eps: float = 1e-5,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    assert x.ndim == 2 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    _lib.call("mpx_groupnorm_leaky", _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), x.size(0), x.size(1), groups,
              float(eps), _lib.ptr(out))
    return out


PRECISIONS = ("fp32", "bf16x3")


class SAWeights(DerivedWeights):
    """Packed (MFMA-stream order) weights of one shared MLP: one pack per precision mode, ``fp32`` (exact fp32 MFMA,
    the parity default) or ``bf16x3`` (split-bf16: hi/lo bf16 operand blocks for the bf16 matrix cores), and the first
    layer split for the factored kernels."""

    def factored(self, convs: List[nn.Conv2d], C: int):
        """First layer split for ``mpx_sa_mlp_factored``: (w_point [c1, Kp] over rows [feat | xyz | 0],
        w_centre [c1, 4] over rows [xyz | 0], -b1)."""
        c0 = convs[0]

        def make():
            w = c0.weight.detach().reshape(c0.out_channels, -1).float()
            assert w.size(1) == 3 + C
            z = lambda n: torch.zeros((w.size(0), n), dtype=torch.float32, device=w.device)
            wp = torch.cat((w[:, 3:], w[:, :3], z((-(3 + C)) % 4)), dim=1).contiguous()
            wc = torch.cat((w[:, :3], z(1)), dim=1).contiguous()
            return wp, wc, (-c0.bias.detach().float()).contiguous()

        return self.entry("factored", (c0.weight, c0.bias), make)

    def get(self, convs: List[nn.Conv2d], C: int, precision: str = "fp32") -> torch.Tensor:
        assert precision in PRECISIONS, precision

        def make():
            c1, c2, c3 = (c.out_channels for c in convs)
            lib = _lib.load()
            dev = convs[0].weight.device
            w = [_lib.f32c(c.weight.detach().reshape(c.out_channels, -1)) for c in convs]
            b = [_lib.f32c(c.bias.detach()) for c in convs]
            if precision == "fp32":
                n = lib.mpx_sa_pack_size(C, c1, c2, c3)
                pack = torch.empty(max(n, 0), dtype=torch.float32, device=dev)
                fn = "mpx_sa_pack_weights"
            else:
                n = lib.mpx_sa_pack_bf16x3_size(C, c1, c2, c3)
                pack = torch.empty(max(n, 0), dtype=torch.uint8, device=dev)
                fn = "mpx_sa_pack_bf16x3"
            if n < 0:
                raise _lib.MpxError(f"unsupported shared-MLP shape C={C} mlp=({c1},{c2},{c3})")
            _lib.call(fn, _lib.ptr(w[0]), _lib.ptr(b[0]), _lib.ptr(w[1]), _lib.ptr(b[1]), _lib.ptr(w[2]),
                      _lib.ptr(b[2]), C, c1, c2, c3, _lib.ptr(pack))
            return pack

        return self.entry(("pack", precision), [p for c in convs for p in (c.weight, c.bias)], make)


def launch_sa(precision: str, xyz_ptr: int, stride: int, new_xyz_ptr: int, new_stride: int, feat_ptr: int,
              feat_stride: int, C: int, idx: torch.Tensor, cnt: Optional[torch.Tensor], B: int, N: int, npoint: int,
              nsample: int, wpack: torch.Tensor, widths: Tuple[int, int, int], out_ptr: int, out_stride: int,
              append_centre: bool = False) -> bool:
    """One fused group + MLP + max-pool launch in either precision (raw pointers: slab views welcome).
    ``cnt`` (from the ball query) lets the kernel skip neighbourhood tiles that hold only padding --
    bit-identical output; for the lockstep bf16x3 kernel the queries are first ordered by tile count.
    ``append_centre``: also write [query xyz | 0] into columns [c3, c3+4) of the output rows (the fp32 kernel with
    counts and the weight-resident bf16x3 kernel); returns whether that was done (False: the caller appends them with ``mpx_append_columns``)."""
    c1, c2, c3 = widths
    if precision == "fp32":
        fused = bool(append_centre and cnt is not None)
        _lib.call("mpx_sa_mlp", xyz_ptr, stride, new_xyz_ptr, new_stride, feat_ptr, feat_stride, C, _lib.ptr(idx),
                  _lib.ptr(cnt), B, N, npoint, nsample, _lib.ptr(wpack), c1, c2, c3, out_ptr, out_stride, int(fused))
        return fused
    order = None
    wants_order = bool(_lib.load().mpx_sa_mlp_bf16x3_wants_order(C, c1, c2, c3, nsample))
    if cnt is not None and wants_order:
        order = torch.empty(B * npoint, dtype=torch.int32, device=idx.device)
        scratch = torch.empty(128, dtype=torch.int32, device=idx.device)
        _lib.call("mpx_sort_queries", _lib.ptr(cnt), B * npoint, nsample, _lib.ptr(order), _lib.ptr(scratch))
    fused = bool(append_centre and not wants_order)  # (the weight-resident kernel completes the rows itself)
    _lib.call("mpx_sa_mlp_bf16x3", xyz_ptr, stride, new_xyz_ptr, new_stride, feat_ptr, feat_stride, C, _lib.ptr(idx),
              _lib.ptr(cnt), _lib.ptr(order), B, N, npoint, nsample, _lib.ptr(wpack), c1, c2, c3, out_ptr, out_stride,
              int(fused))
    return fused


def sa_mlp_fused(xyz: torch.Tensor, new_xyz: torch.Tensor, feat: torch.Tensor, feat_stride: int, C: int,
                 idx: torch.Tensor, wpack: torch.Tensor, widths: Tuple[int, int, int],
                 out: Optional[torch.Tensor] = None, precision: str = "fp32",
                 cnt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused group + MLP + max-pool.  xyz [B,N,S]; new_xyz [B,npoint,S']; feat: tensor whose
    ``data_ptr`` is the first feature of point 0 with ``feat_stride`` floats between points;
    -> out [B,npoint,c3] point-major (``out`` may be a column slice of a wider buffer)."""
    B, N, S = xyz.shape
    npoint, nsample = idx.shape[1:]
    c1, c2, c3 = widths
    if out is None:
        out = torch.empty((B, npoint, c3), dtype=torch.float32, device=xyz.device)
    assert out.stride(2) == 1 and out.stride(0) == npoint * out.stride(1)
    launch_sa(precision, _lib.ptr(xyz), S, _lib.ptr(new_xyz), new_xyz.stride(1), _lib.ptr(feat), feat_stride, C, idx, cnt,
              B, N, npoint, nsample, wpack, widths, _lib.ptr(out), out.stride(1))
    return out


def sa_mlp_factored(point_rows: torch.Tensor, centre_rows: torch.Tensor, idx: torch.Tensor, cnt: torch.Tensor,
                    packed: SAWeights, convs: List[nn.Conv2d], C: int, N: int, out_ptr: int, out_stride: int,
                    precision: str = "fp32") -> None:
    """The (64+3,128,128,256) module with its first layer evaluated per point / per query instead of per
    (query, neighbour) row (``mpx_sa_mlp_factored`` / ``mpx_sa_mlp_bf16x3_factored``).  ``point_rows`` [B*N, Kp] =
    [feat | xyz | 0] rows, ``centre_rows`` [B*npoint, 4] = [xyz | anything finite] rows (row strides free)."""
    B, npoint, nsample = idx.shape
    wp, wc, nb1 = packed.factored(convs, C)
    c1, c2, c3 = (c.out_channels for c in convs)
    # (bf16x3 too: K = 68 is HBM-bound either way -- the fp32 row-per-lane kernel is the faster one, 0.71 vs 0.79 ms, and exact)
    pre = linear(point_rows, wp, None)
    ctr = linear(centre_rows, wc, nb1)  # K = 4: not worth the matrix cores
    x3 = precision == "bf16x3"
    # (the bf16x3 kernel is persistent and takes its units from a device-side queue: no sorting pass, order = NULL)
    order = (None,) if x3 else ()
    _lib.call("mpx_sa_mlp_bf16x3_factored" if x3 else "mpx_sa_mlp_factored", _lib.ptr(pre), _lib.ptr(ctr), _lib.ptr(idx),
              _lib.ptr(cnt), *order, B, N, npoint, nsample, _lib.ptr(packed.get(convs, C, precision)), C, c1, c2, c3, out_ptr,
              out_stride)


FACTORED_SHAPE = (64, 128, 128, 256)
FACTORED_BF16X3_MAX_NSAMPLE = 128  # (= csrc/sa_mlp_bf16.hip v2::MAX_NSAMPLE: the persistent kernel's row -> query table)


def use_factored(module: "PointnetSAModule", C: int, convs) -> bool:
    """Does this module run with its first layer factored per point / per query?  Only the (64+3, 128, 128, 256) shape has
    the kernels, and the ``bf16x3`` one is built for <= 128 slots per neighbourhood (larger ones take the unfactored
    kernel, which has no such limit)."""
    if not module.factored or (C,) + tuple(c.out_channels for c in convs) != FACTORED_SHAPE:
        return False
    return module.precision != "bf16x3" or module.nsample <= FACTORED_BF16X3_MAX_NSAMPLE


# ---- module -------------------------------------------------------------------------------------------
class PointnetSAModule(nn.Module):
    """``PointnetSAModule(npoint=None, radius=None, nsample=None, mlp=[...], bn=False, use_xyz=True)``.

    ``forward(xyz [B,N,3], features [B,C,N]) -> (new_xyz [B,npoint,3] | None, [B,mlp[-1],npoint])``.
    """

    def __init__(self, *, mlp: List[int], npoint: Optional[int] = None, radius: Optional[float] = None,
                 nsample: Optional[int] = None, bn: bool = False, use_xyz: bool = True, precision: str = "fp32"):
        super().__init__()
        assert precision in PRECISIONS
        self.precision = precision  # "fp32" (exact) | "bf16x3" (split-bf16 matrix cores, ~3e-7 on the policy output)
        # skip neighbourhood tiles that hold only ball-query padding (bit-identical output, see launch_sa)
        self.elide_padding = True
        # evaluate the first layer per point / per query where the kernel supports it (fp32, SA2 shape)
        self.factored = True
        if bn:
            raise NotImplementedError("bn=True is not used by the reference (model.py:366-383)")
        assert use_xyz, "the reference relies on use_xyz=True (3 extra input channels)"
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        spec = list(mlp)
        spec[0] += 3
        layers: List[nn.Module] = []
        for i in range(len(spec) - 1):
            layers.append(nn.Conv2d(spec[i], spec[i + 1], kernel_size=1, bias=True))
            layers.append(nn.ReLU(inplace=True))
        # same container shape as pointnet2_ops: self.mlps = ModuleList([Sequential(conv, relu, ...)])
        self.mlps = nn.ModuleList([nn.Sequential(*layers)])
        self._packed = SAWeights()

    def convs(self) -> List[nn.Conv2d]:
        return [m for m in self.mlps[0] if isinstance(m, nn.Conv2d)]

    def forward(self, xyz: torch.Tensor, features: Optional[torch.Tensor] = None):
        if not xyz.is_cuda:
            raise _lib.MpxError("CPU tensors not supported (reference: model.py:417)")
        xyz = _lib.f32c(xyz)
        B, N, _ = xyz.shape
        convs = self.convs()
        if self.npoint is not None:
            assert features is not None
            C = features.size(1)
            feat_pm = _lib.f32c(features).transpose(1, 2).contiguous()  # [B,N,C] point-major
            idx, new_xyz = furthest_point_sample(xyz, self.npoint, return_xyz=True)
            nbr, cnt = ball_query(self.radius, self.nsample, xyz, new_xyz, return_counts=True)
            if self.training and torch.is_grad_enabled():
                from .train_ops import sa_module_train

                fpm = features.transpose(1, 2).contiguous() if features.requires_grad else feat_pm
                out = sa_module_train(convs, xyz, 3, new_xyz, 3, fpm, C, C, nbr, cnt, (B, N, self.npoint, self.nsample))
                return new_xyz, out.transpose(1, 2).contiguous()
            if use_factored(self, C, convs):
                full = cnt if self.elide_padding else torch.full_like(cnt, self.nsample)
                rows = torch.cat((feat_pm, xyz, torch.zeros_like(xyz[:, :, :1])), dim=2).view(B * N, C + 4)
                ctr_rows = torch.nn.functional.pad(new_xyz, (0, 1)).view(B * self.npoint, 4)
                out = torch.empty((B, self.npoint, convs[-1].out_channels), dtype=torch.float32, device=xyz.device)
                sa_mlp_factored(rows, ctr_rows, nbr, full, self._packed, convs, C, N, _lib.ptr(out), out.stride(1),
                                precision=self.precision)
                return new_xyz, out.transpose(1, 2).contiguous()
            wpack = self._packed.get(convs, C, self.precision)
            out = sa_mlp_fused(xyz, new_xyz, feat_pm, C, C, nbr, wpack, tuple(c.out_channels for c in convs),
                               precision=self.precision, cnt=cnt if self.elide_padding else None)
            return new_xyz, out.transpose(1, 2).contiguous()
        # group-all: one "neighbourhood" holding every point, xyz NOT re-centred
        if self.training and torch.is_grad_enabled():
            from .train_ops import linear_train

            h = torch.cat([xyz] + ([features.transpose(1, 2)] if features is not None else []), dim=2)
            for conv in convs:
                h = linear_train(h, conv.weight.view(conv.out_channels, -1), conv.bias, 1)
            return None, h.max(dim=1).values.unsqueeze(-1)
        parts = [xyz]
        if features is not None:
            parts.append(_lib.f32c(features).transpose(1, 2))
        x = torch.cat(parts, dim=2)  # [B,N,3+C]
        K = x.size(2)
        Kp = (K + 3) // 4 * 4
        if Kp != K:
            x = torch.nn.functional.pad(x, (0, Kp - K))
        h = x.reshape(B * N, Kp).contiguous()
        for conv in convs:
            w = conv.weight.detach().reshape(conv.out_channels, -1)
            if w.size(1) != h.size(1):
                w = torch.nn.functional.pad(w, (0, h.size(1) - w.size(1)))
            h = linear(h, _lib.f32c(w), _lib.f32c(conv.bias.detach()), act=1)
        pooled = torch.empty((B, h.size(1)), dtype=torch.float32, device=xyz.device)
        _lib.call("mpx_rowmax", _lib.ptr(h), h.stride(0), B, N, h.size(1), _lib.ptr(pooled), pooled.stride(0))
        return None, pooled.unsqueeze(-1)
