"""Training path (row N1), the Python face of ``csrc/train_ops.hip`` and ``csrc/dense_grad.hip``: dense layers, GroupNorm +
LeakyReLU, grouping and the segment max-pool as autograd nodes whose forward AND backward are this engine's kernels.
Imports go one way: from ``pointnet2`` to here (``PointnetSAModule`` imports from here inside its training branches)."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from .pointnet2 import PRECISIONS, groupnorm_leaky, linear, split_pairs

# the backward of [last dense layer + ReLU + max-pool] walks the pool's Q * C non-zero gradients (mpx_pool_wgrad /
# mpx_pool_dgrad) instead of forming the [rows, C] gradient and running two dense GEMMs over its zeros;
# False = the dense route (mpx_segment_max_grad_act + mpx_linear_wgrad / mpx_linear_dact), kept for A/B tests
SPARSE_POOL_BACKWARD = True


def _pad4(t: torch.Tensor, rows: bool = False) -> torch.Tensor:
    """Zero-pad the last (or with ``rows`` the first) dimension of a matrix to a multiple of 4."""
    n = t.size(0 if rows else 1)
    n4 = (n + 3) // 4 * 4
    if n4 == n:
        return t
    return torch.nn.functional.pad(t, (0, 0, 0, n4 - n) if rows else (0, n4 - n))


def _transposed(wp: torch.Tensor) -> torch.Tensor:
    """Column-padded weight [N, Kp] -> [Kp, Np] contiguous: the weight operand of the input-gradient GEMMs."""
    return _pad4(wp, rows=True).t().contiguous()


def _dense_wgrad(dz: torch.Tensor, x: torch.Tensor, N: int, K: int, has_bias: bool, x3: bool):
    """Weight / bias gradient of a dense layer from ``dz`` [M, Np] and its saved input ``x`` [M, Kp] (zero-padded to multiples
    of 4) -> (dw [N, K], db [N] or None): ``dw | db`` is one buffer, one fixed-order reduction launch; ``x3``: split bf16."""
    M, Np = dz.shape
    Kp = x.size(1)
    both = torch.empty(Np * Kp + Np, dtype=torch.float32, device=dz.device)
    dw = both[:Np * Kp].view(Np, Kp)
    db = both[Np * Kp:] if has_bias else None
    scratch = torch.empty(_lib.load().mpx_linear_wgrad_scratch(M, Np, Kp), dtype=torch.float32, device=dz.device)
    _lib.call("mpx_linear_wgrad_bf16x3" if x3 else "mpx_linear_wgrad", _lib.ptr(dz), dz.stride(0), _lib.ptr(x), x.stride(0),
              M, Np, Kp, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch))
    return dw[:N, :K], (db[:N] if has_bias else None)


def _pool_wgrad(g: torch.Tensor, arg: torch.Tensor, pooled: torch.Tensor, act: int, x: torch.Tensor, K: int, has_bias: bool):
    """``_dense_wgrad`` of a layer whose output was max-pooled to ``pooled`` [Q, N] (arg-max rows ``arg``), from the pool's
    gradient ``g`` [Q, N]: the kernel applies the activation backward and walks the Q * N non-zeros of dz.  Always fp32."""
    Q, N = pooled.shape
    Kp = x.size(1)
    both = torch.empty(N * Kp + N, dtype=torch.float32, device=g.device)
    dw, db = both[:N * Kp].view(N, Kp), both[N * Kp:]
    scratch = torch.empty(_lib.load().mpx_pool_wgrad_scratch(Q, N, Kp), dtype=torch.float32, device=g.device)
    _lib.call("mpx_pool_wgrad", _lib.ptr(g), g.stride(0), _lib.ptr(arg), _lib.ptr(pooled), N, Q, N, act, _lib.ptr(x),
              x.stride(0), Kp, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch))
    return dw[:, :K], (db if has_bias else None)


def _act_backward(g: torch.Tensor, y: torch.Tensor, act: int) -> torch.Tensor:
    """g * act'(y) elementwise (``y``: the activation's output, laid out like ``g``); ``act`` 0: g itself."""
    if not act:
        return g
    dz = torch.empty_like(g)
    _lib.call("mpx_act_backward", _lib.ptr(g), _lib.ptr(y), g.numel(), act, _lib.ptr(dz))
    return dz


# ---- dense layer, GroupNorm + LeakyReLU: one node per layer ------------------------------------------------------------
class _LinearFn(torch.autograd.Function):
    """y = act(x @ W.T + b) with ``mpx_linear`` forward; backward = ``mpx_act_backward`` + ``mpx_linear`` on W^T
    (input gradient) + ``mpx_linear_wgrad`` (weight / bias gradients, deterministic split reduction)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        assert x.ndim == 2 and weight.ndim == 2 and x.size(1) == weight.size(1)
        N, K = weight.shape
        # first layers (4, 67, 259, 7 inputs): zero columns change nothing
        xp, wp = _pad4(_lib.f32c(x.detach())), _pad4(_lib.f32c(weight.detach()))
        y = linear(xp, wp, None if bias is None else _lib.f32c(bias.detach()), act)
        ctx.save_for_backward(xp, wp, y if act else None)
        ctx.meta = (act, N, K, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        xp, wp, y = ctx.saved_tensors
        act, N, K, has_bias = ctx.meta
        dz = _pad4(_act_backward(_lib.f32c(g), y, act))  # (pads the 7-wide output layer)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = linear(dz, _transposed(wp), None, 0)[:, :K]  # [M, Kp] -> [M, K]
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            gw, gb = _dense_wgrad(dz, xp, N, K, has_bias, False)
        return gx, gw, gb, None


class _GroupNormLeakyFn(torch.autograd.Function):
    """GroupNorm(groups) + LeakyReLU(0.01) on [M, C]: ``mpx_groupnorm_leaky`` forward, ``mpx_groupnorm_leaky_grad`` back."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups, eps):
        xc, w, b = _lib.f32c(x.detach()), _lib.f32c(weight.detach()), _lib.f32c(bias.detach())
        y = groupnorm_leaky(xc, w, b, groups, eps)
        ctx.save_for_backward(xc, w, b)
        ctx.meta = (groups, eps)
        return y

    @staticmethod
    def backward(ctx, g):
        xc, w, b = ctx.saved_tensors
        groups, eps = ctx.meta
        g = _lib.f32c(g)
        M, C = xc.shape
        dx, dw, db = torch.empty_like(xc), torch.empty_like(w), torch.empty_like(b)
        stats = torch.empty(2 * M * groups, dtype=torch.float32, device=xc.device)
        _lib.call("mpx_groupnorm_leaky_grad", _lib.ptr(xc), _lib.ptr(w), _lib.ptr(b), _lib.ptr(g), M, C, groups, float(eps),
                  _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(stats))
        return dx, dw, db, None, None


def groupnorm_leaky_train(x: torch.Tensor, norm: nn.GroupNorm) -> torch.Tensor:
    return _GroupNormLeakyFn.apply(x, norm.weight, norm.bias, norm.num_groups, norm.eps)


def linear_train(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0) -> torch.Tensor:
    """Differentiable dense layer on the engine's kernels; ``x`` may have leading batch dimensions."""
    lead = x.shape[:-1]
    y = _LinearFn.apply(x.reshape(-1, x.size(-1)), weight, bias, act)
    return y.reshape(lead + (weight.size(0),))


# ---- differentiable grouping + max-pool on packed distinct-neighbour rows -------------------------------------------------
class _PackRows(torch.autograd.Function):
    """QueryAndGroup(use_xyz=True) without the padding: -> rows [R, 3+C]; gradient flows to ``feat`` only."""

    @staticmethod
    def forward(ctx, feat, xyz, xyz_stride, new_xyz, new_stride, feat_stride, C, idx, cnt, offsets, R, dims):
        B, N, npoint, nsample = dims
        ld = (3 + C + 3) // 4 * 4  # rows padded to 16 bytes (zero columns): the GEMMs take them as they are, no padding copy
        rows = torch.empty((R, ld), dtype=torch.float32, device=idx.device)
        _lib.call("mpx_pack_rows_ld", _lib.ptr(xyz), xyz_stride, _lib.ptr(new_xyz), new_stride, _lib.ptr(feat),
                  feat_stride, C, _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(offsets), B, N, npoint, nsample, _lib.ptr(rows), ld)
        ctx.save_for_backward(idx, cnt, offsets)
        ctx.meta = (C, dims, tuple(feat.shape), feat_stride)
        return rows

    @staticmethod
    def backward(ctx, g):
        idx, cnt, offsets = ctx.saved_tensors
        C, (B, N, npoint, nsample), shape, feat_stride = ctx.meta
        if not ctx.needs_input_grad[0]:
            return (None,) * 12
        if g.dtype != torch.float32 or g.stride(1) != 1 or g.stride(0) < 3 + C:
            g = _lib.f32c(g)
        gf = torch.zeros(shape, dtype=torch.float32, device=g.device)
        _lib.call("mpx_pack_rows_grad_ld", _lib.ptr(g), g.stride(0), C, _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(offsets), B, N,
                  npoint, nsample, _lib.ptr(gf), gf.stride(1))
        return (gf,) + (None,) * 11


class _SegmentMax(torch.autograd.Function):
    """Max-pool over each query's rows: y [R,C], offsets [Q+1] -> [Q,C].  (The per-layer form the tests hold the pooled
    ``_MLPChainFn`` against; the model pools inside the chain.)"""

    @staticmethod
    def forward(ctx, y, offsets, Q):
        y = _lib.f32c(y)
        C = y.size(1)
        out = torch.empty((Q, C), dtype=torch.float32, device=y.device)
        arg = torch.empty((Q, C), dtype=torch.int64, device=y.device)
        _lib.call("mpx_segment_max", _lib.ptr(y), C, _lib.ptr(offsets), Q, _lib.ptr(out), C, _lib.ptr(arg))
        ctx.save_for_backward(arg)
        ctx.meta = (y.size(0), C, Q)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        R, C, Q = ctx.meta
        g = _lib.f32c(g)
        gy = torch.zeros((R, C), dtype=torch.float32, device=g.device)
        _lib.call("mpx_segment_max_grad", _lib.ptr(g), g.stride(0), _lib.ptr(arg), Q, C, _lib.ptr(gy))
        return gy, None, None


# ---- a stack of dense layers (and its max-pool) as one node -----------------------------------------------------------------
class _MLPChainFn(torch.autograd.Function):
    """A stack of dense layers ``h <- act_i(h @ W_i.T + b_i)`` as ONE autograd node (row N1).

    Arguments: x [M, K0], acts (tuple of activation codes), offsets (int64 [Q+1] with offsets[0] = 0 and offsets[Q] = M: the
    segments tile the rows; or None), x3 (bool), then W_0, b_0, W_1, b_1, ...  Returns the last layer's rows [M, N_last],
    or with ``offsets`` (the set-abstraction modules) their per-segment maximum [Q, N_last]: the last GEMM max-pools in
    its epilogue (``mpx_linear_segmax``, bit for bit ``mpx_linear`` + ``mpx_segment_max``), so its [M, N_last] rows (2 GB
    for the second module at batch 256) are neither written nor kept, only the pooled rows and their arg-max rows.

    Backward: ``dY * act'(y)`` gets no pass of its own where a GEMM can apply it.  An input gradient takes one of three routes:
      * ``mpx_pool_dgrad``: the last layer of a pooled stack under ``SPARSE_POOL_BACKWARD`` (the default).  The pool hands
        each (query, channel) gradient to ONE row, so that layer's two products (with ``mpx_pool_wgrad``) walk those
        Q * N_last non-zeros.  Both kernels are ALWAYS fp32, also under ``x3``.  ``SPARSE_POOL_BACKWARD = False`` is the A/B
        route: ``mpx_segment_max_grad_act`` writes the [M, N_last] gradient and the last layer is a dense one like the rest;
      * skinny, ``not lx3 and mpx_linear_workspace(M, Kp, Np) > 0`` (the reference's batch of 10): split-K ``linear`` over
        the whole chip, then ``mpx_act_backward`` in place for the activation of the layer below;
      * otherwise ``mpx_linear_dact`` / ``mpx_linear_bf16x3_dact``: the 128 x 128 tile GEMM with that backward in its epilogue.
    Gradients equal the per-layer form (``_LinearFn`` per layer + ``_SegmentMax``) bit for bit only on the dact route and
    the dense pooled route, where both forms run the same GEMM kernel; the other two routes sum in another order.

    ``x3``: the three GEMMs of every layer that ``_use_x3`` admits run in the split-bf16 arithmetic of the ``bf16x3`` mode
    (fp32 master weights, accumulation and activations): the engine's form of the reference's ``precision=16``
    (run_training.py:112).
    """

    @staticmethod
    def _use_x3(x3, M, N, K):
        return bool(x3) and M >= 1024 and N >= 128 and K >= 16

    @staticmethod
    def forward(ctx, x, acts, offsets, x3, *wb):
        L = len(acts)
        assert len(wb) == 2 * L and x.ndim == 2
        M, K0 = x.shape
        dev = x.device
        h = _pad4(_lib.f32c(x.detach()))
        xs, ws, meta = [], [], []
        arg = None
        for i in range(L):
            w, b = wb[2 * i], wb[2 * i + 1]
            N, K = w.shape
            wp = _pad4(_lib.f32c(w.detach()))
            Kp = wp.size(1)
            assert h.size(1) == Kp, "layer widths do not chain"
            bias = None if b is None else _lib.f32c(b.detach())
            xs.append(h)
            ws.append(wp)
            meta.append((N, K, b is not None))
            lx3 = _MLPChainFn._use_x3(x3, M, N, Kp)
            if offsets is not None and i == L - 1:
                Q = offsets.numel() - 1
                seg = torch.repeat_interleave(torch.arange(Q, dtype=torch.int32, device=dev), offsets[1:] - offsets[:-1],
                                              output_size=M)
                y = torch.empty((Q, N), dtype=torch.float32, device=dev)  # (the pooled rows)
                arg = torch.empty((Q, N), dtype=torch.int64, device=dev)
                keys = torch.empty((Q, N), dtype=torch.int64, device=dev)
                _lib.call("mpx_linear_segmax_bf16x3" if lx3 else "mpx_linear_segmax", _lib.ptr(h), h.stride(0),
                          _lib.ptr(split_pairs(wp) if lx3 else wp), _lib.ptr(bias), M, N, Kp, acts[i], _lib.ptr(seg), Q,
                          _lib.ptr(keys), _lib.ptr(y), N, _lib.ptr(arg))
            elif lx3:
                y = torch.empty((M, N), dtype=torch.float32, device=dev)
                _lib.call("mpx_linear_bf16x3", _lib.ptr(h), h.stride(0), _lib.ptr(split_pairs(wp)), _lib.ptr(bias), M, N, Kp,
                          acts[i], _lib.ptr(y), N)
            else:  # (not a name pair with the call above: ``linear`` owns the choice between mpx_linear and its split-K form)
                y = linear(h, wp, bias, acts[i])
            h = _pad4(y) if i + 1 < L else y
        # (of a pooled stack the last layer's rows are not needed again: the pooled rows, their arg-max, the segments)
        ctx.save_for_backward(*xs, *ws, *((h,) if offsets is None else (h, arg, offsets)))
        ctx.meta = (tuple(acts), tuple(meta), M, K0, offsets is not None, bool(x3))
        return h

    @staticmethod
    def backward(ctx, g):
        acts, meta, M, K0, pooled_out, x3 = ctx.meta
        L = len(acts)
        saved = ctx.saved_tensors
        xs, ws = saved[:L], saved[L:2 * L]
        g = _lib.f32c(g)
        dev = g.device
        needs = ctx.needs_input_grad  # (x, acts, offsets, x3, W_0, b_0, ...)
        grads = [None] * (2 * L)
        top = L - 1  # the layers [0, top] go through the dense GEMMs below
        if pooled_out and SPARSE_POOL_BACKWARD:
            pooled, arg, offsets = saved[2 * L:]
            Q, N = pooled.shape
            _, K, has_bias = meta[top]
            Kp = ws[top].size(1)
            assert ws[top].size(0) == N
            if needs[4 + 2 * top] or (has_bias and needs[5 + 2 * top]):
                grads[2 * top], grads[2 * top + 1] = _pool_wgrad(g, arg, pooled, acts[top], xs[top], K, has_bias)
            dz = None
            if top > 0 or needs[0]:
                below = acts[top - 1] if top > 0 else 0
                dz = torch.empty((M, Kp), dtype=torch.float32, device=dev)  # (every row is written: the segments tile [0, M))
                _lib.call("mpx_pool_dgrad", _lib.ptr(g), g.stride(0), _lib.ptr(arg), _lib.ptr(pooled), N, _lib.ptr(offsets),
                          Q, N, acts[top], _lib.ptr(ws[top]), Kp, _lib.ptr(xs[top]) if below else None, xs[top].stride(0),
                          below, Kp, 0, _lib.ptr(dz), Kp)
            top -= 1
        elif pooled_out:
            pooled, arg, offsets = saved[2 * L:]
            Q, C = pooled.shape
            dz = torch.empty((M, C), dtype=torch.float32, device=dev)  # (every row is written: the segments tile [0, M))
            _lib.call("mpx_segment_max_grad_act", _lib.ptr(g), g.stride(0), _lib.ptr(arg), _lib.ptr(pooled), C,
                      _lib.ptr(offsets), Q, C, acts[-1], _lib.ptr(dz))
        else:
            dz = _act_backward(g, saved[2 * L], acts[-1])
        for i in range(top, -1, -1):
            N, K, has_bias = meta[i]
            dz = _pad4(dz)
            Np, Kp = dz.size(1), ws[i].size(1)
            lx3 = _MLPChainFn._use_x3(x3, M, N, Kp)
            if needs[4 + 2 * i] or (has_bias and needs[5 + 2 * i]):
                grads[2 * i], grads[2 * i + 1] = _dense_wgrad(dz, xs[i], N, K, has_bias, lx3)
            gx = None
            if i > 0 or needs[0]:
                wt = _transposed(ws[i])  # [Kp, Np]
                gx = torch.empty((M, Kp), dtype=torch.float32, device=dev)
                # xs[i] IS the output of layer i - 1 (zero-padded columns: their gradient columns are dropped at the end)
                below = acts[i - 1] if i > 0 else 0
                if not lx3 and _lib.load().mpx_linear_workspace(M, Kp, Np) > 0:
                    # skinny (a handful of 128 x 128 tiles walking K alone): the split-K GEMM over the whole chip + the
                    # elementwise backward beats the fused epilogue on 8 CUs
                    linear(dz, wt, None, 0, out=gx)
                    if below:
                        _lib.call("mpx_act_backward", _lib.ptr(gx), _lib.ptr(xs[i]), gx.numel(), below, _lib.ptr(gx))
                else:
                    _lib.call("mpx_linear_bf16x3_dact" if lx3 else "mpx_linear_dact", _lib.ptr(dz), dz.stride(0),
                              _lib.ptr(split_pairs(wt) if lx3 else wt), M, Kp, Np, _lib.ptr(xs[i]) if below else None,
                              xs[i].stride(0), below, _lib.ptr(gx), Kp)
            dz = gx
        gx0 = dz[:, :K0] if (dz is not None and needs[0]) else None
        return (gx0, None, None, None) + tuple(grads)


def mlp_chain_train(x: torch.Tensor, layers, acts, offsets: Optional[torch.Tensor] = None,
                    precision: str = "fp32", offsets_checked: bool = False) -> torch.Tensor:
    """Differentiable stack of dense layers on the engine's kernels (one autograd node, see ``_MLPChainFn``).
    ``layers``: sequence of (weight [N,K], bias or None); ``acts``: one activation code per layer; ``x`` may have leading
    batch dimensions (flattened; not with ``offsets``); ``precision``: "fp32" or "bf16x3" (the large GEMMs of forward and
    backward in split bf16, see ``_MLPChainFn``).  ``offsets`` (int64 [Q+1]) must tile the rows: offsets[0] = 0, ascending,
    offsets[Q] = number of rows -- the pool's backward writes whole segments into an uninitialised buffer, so a gap would
    leak garbage into the gradients; checked here (one host sync) unless the caller vouches with ``offsets_checked``."""
    assert precision in PRECISIONS
    if offsets is not None and not offsets_checked:
        assert x.ndim == 2 and offsets.ndim == 1 and offsets.numel() >= 2, "offsets: int64 [Q+1] over 2-D rows"
        ends = offsets[[0, -1]].tolist()
        assert ends == [0, x.size(0)] and bool((offsets[1:] >= offsets[:-1]).all()), \
            f"offsets must tile the {x.size(0)} rows (got [{ends[0]} .. {ends[1]}], ascending required)"
    lead = x.shape[:-1]
    wb = []
    for w, b in layers:
        wb += [w, b]
    y = _MLPChainFn.apply(x.reshape(-1, x.size(-1)), tuple(int(a) for a in acts), offsets, precision == "bf16x3", *wb)
    return y if offsets is not None else y.reshape(lead + (y.size(-1),))


def segment_offsets(cnt: torch.Tensor) -> torch.Tensor:
    """int64 [Q+1]: start of every query's rows in the packed matrix (a query without a hit keeps one row)."""
    offsets = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=cnt.device)
    torch.cumsum(cnt.reshape(-1).clamp(min=1), 0, out=offsets[1:])
    return offsets


def sa_module_train(convs: List[nn.Conv2d], xyz: torch.Tensor, xyz_stride: int, new_xyz: torch.Tensor,
                    new_stride: int, feat: torch.Tensor, feat_stride: int, C: int, idx: torch.Tensor,
                    cnt: torch.Tensor, dims: Tuple[int, int, int, int], precision: str = "fp32",
                    offsets: Optional[torch.Tensor] = None, R: Optional[int] = None) -> torch.Tensor:
    """Differentiable set-abstraction MLP + max-pool -> [B, npoint, C_out].  ``feat`` is any tensor whose storage
    holds the point-major features (``feat_stride`` floats between points); it receives the gradient.
    ``offsets`` / ``R`` (``segment_offsets(cnt)`` and its last entry as a host int): a caller that has them already --
    the model reads both modules' row counts with ONE host sync -- passes them in."""
    B, N, npoint, nsample = dims
    if offsets is None:
        offsets = segment_offsets(cnt)
    if R is None:
        R = int(offsets[-1].item())  # a host sync: the row count sizes the activations
    h = _PackRows.apply(feat, xyz, xyz_stride, new_xyz, new_stride, feat_stride, C, idx, cnt, offsets, R, dims)
    layers = [(conv.weight.view(conv.out_channels, -1), conv.bias) for conv in convs]
    # (offsets = cumsum of the clamped counts, R = its last entry = the rows _PackRows made: the segments tile them)
    return mlp_chain_train(h, layers, [1] * len(layers), offsets=offsets, precision=precision,
                           offsets_checked=True).view(B, npoint, -1)
