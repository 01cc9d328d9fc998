"""The training step at the benchmark's batch sizes against float64, stage by stage, EVERY parameter, every element.

The backward's launch choices switch with the row count: gemv / split-K / tile for the heads' GEMMs, weight gradients
written directly (one split) or as split partials reduced in a fixed order, 64- or 128-wide weight-gradient tiles, the
max-pool's sparse weight gradient in one split or several, the chains' skinny split-K input gradient, split-bf16 layers
in ``bf16x3``.  A split dropped or counted twice, a pool gradient routed to the wrong row or a scatter that loses an
update stays deterministic and finite; a bar of 2e-4 of the largest gradient at batch 2 cannot see it.
``training_route_table`` mirrors the C predicates (checked against the library's own scratch sizes on the GPU) and
``test_training_cases_cover_every_route`` makes sure the six cases turn each route on AND off.

What runs.  One ``training_step`` of ``TrainingMotionPolicyNetwork(2048, 1.0, 5.0)`` on the problem and seeded weights of
test_gpu_batch_parity.py (supervision as in bench.py: clamp(q + 0.05 N(0,1), -1, 1)), then the same step composed by hand
(``tm(xyz, q, aux=aux)``, clamp, the loss container) whose loss must equal training_step's bit for bit, and its
backward.  Node hooks on every ``_MLPChainFn`` / ``_LinearFn`` / ``_GroupNormLeakyFn`` / ``_PackRows`` node record the
HIP upstream gradient and the HIP gradients each node returns; ``node.saved_tensors`` give the HIP layer inputs
(``xs[i]``: each layer's post-activation rows), the pooled rows, the arg-max rows and the segment offsets.

Reference: per stage, float64 torch ops on the GPU (query-aligned slabs of <= 2^20 rows), from the HIP input of that
stage, the HIP upstream gradient and the HIP discrete decisions (arg-max rows, activation signs); nothing else from
``libmpinets_hip``.  Stages: loss (d loss / d dq from the oracle's float64 robot cloud and losses at the HIP dq), decoder
and joint-encoder chains, the fc head node by node (three dense layers, two GroupNorm + LeakyReLU), the group-all chain,
SA2 (its packed rows bit-exact against torch indexing, the chain, the scatter into f1 against a float64 ``index_add`` of
the HIP row gradients), SA1 (the chain; the cloud's label column gets no gradient).  Every ``named_parameters()``
gradient is compared in exactly one stage; the test asserts this.
Decision validity: every HIP arg-max row is a float64 near-max of its segment (its float64 value is at least the
segment's float64 max minus the arg-max row's forward bar minus the segment's largest forward bar), and every HIP
activation sign agrees with the float64 layer evaluated on the HIP layer input wherever |z64| exceeds the forward bar.
Each layer's HIP output is also held to that float64 evaluation (forward bar), so the HIP layer inputs the reference
starts from are themselves checked.

Error bars: the magnitude pass of test_gpu_batch_parity.py run backwards.  ``mag_dz`` starts at |HIP upstream gradient|
(times the activation's slope), a layer maps it to ``mag_dx = mag_dz |W|`` and ``mag_dz <- mag_dx * mask`` below it, the
pool routes it along the HIP arg-max.  With ``u`` = 1e-6 per fp32 GEMM and 3e-5 per split-bf16 GEMM (as in the forward
test):
  * the stage's input gradient: ``(sum over its layers of u_dX) * mag_dx``;
  * a layer's dW: ``(kappa_w + sum of u_dX of the layers above it) * (mag_dz^T |x|)``, and db with ``sum(mag_dz)``.
    ``kappa_w`` is derived from the wgrad's reduction shape, not fitted: the kernels (mpx_linear_wgrad, mpx_pool_wgrad)
    reduce ``n`` = rows_per_split rows (queries per split for the pool) in one fp32 fma chain, then the S split partials
    in a fixed order.  The cdna_hip_programming guide gives 0.75-1.5e-7 * sum|a b| for an fp32 chain at K <= 1024 and
    3.5e-7 at K = 4096 (square-root growth) for terms of mixed sign; terms of one sign keep partial sums as large as
    sum |a b|, for which the probabilistic bound is sqrt(n) 2^-24.  So a chain of n costs
    ``k(n) = 3.5e-7 * max(1, sqrt(n / 4096)) + 2^-24 sqrt(n)`` and ``kappa_w = k(rows_per_split) + k(S)`` (+ 3e-5 for
    mpx_linear_wgrad_bf16x3's split products).  SA1's first layers at batch 256 (~2.1 M rows in 1024 splits of ~2 K
    rows): kappa_w ~ 5e-6.
  * GroupNorm + LeakyReLU backward (mean mu, rstd r, x_hat = (x - mu) r, per group, m = |dy| * slope * |gamma|,
    a = |x_hat| + (|x| + |mu|) r + |x_hat| r^2 mean(|x - mu| (|x| + |mu|)), the size of x_hat plus the scale of its
    first-order perturbation by x, mu and r -- the forward test's GroupNorm term with mag = |x| + |mu|):
    ``|dx| <= r (m + mean(m) + a mean(m a))``, bar 1e-6 times that; dgamma ``sum(|dy| slope a)``, dbeta ``sum(|dy| slope)``,
    1e-6 times those.  (The forward's term, in test_gpu_batch_parity.py, is the same perturbation of x, mu and s.)
  * the f1 scatter (float atomics, any order): ``k(largest number of rows one point receives) * index_add(|g_rows|)``;
  * the loss gradient: 2e-5 of its largest element, the bar of test_training_step_shape_batch_vs_oracle, in every
    environment none of whose robot points lies within 1e-6 m of a branch of the collision loss -- the hinge, a tie
    between two primitives, two equally near faces inside one, a face plane -- or has a coordinate within the HIP
    clouds' position errors of the target's (the kink of the point-match L1 term, where the signs can differ).  Such a point takes its branch from fp32 rounding and moves its environment's
    gradient by that point's share; those environments are counted and printed, and may be at most 1 in 20.  The HIP robot cloud is asserted to
    lie within 5e-7 m of the float64 one, so 1e-6 m covers its position error and the distances' own rounding.
The worst err / bar of every stage and tensor is printed.

Training forward at scale: f1, sa3_in's feature columns, f3, the encoding and dq of the TRAINING forward (pack rows ->
mpx_linear -> mpx_linear_segmax, not the inference kernels) against the per-module references and bars of
test_gpu_batch_parity.py (float64_policy.reference).

Controls, each planted into a fresh copy of the HIP result at >= 20 spread places where the defect changes the result at
all; fp32 must flag >= 90 %, bf16x3 some (share printed): a dropped weight-gradient split (SA2's first layer minus the
float64 contribution of one split's rows, split bounds from ``wgrad_route``, splits whose rows carry gradient), a
misrouted pool gradient (SA1's last layer: one (query, channel) gradient of the largest tenth moved to the row of
its segment that differs most), a lost scatter update (one packed row with a gradient missing from the f1 gradient).
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from float64_policy import (KAPPA, NP1, NP2, NS, _cdiv, check, dev, problem, reference,  # noqa: F401
                            weights)
from launch_routes import linear_route, pool_wgrad_splits, wgrad_route

CASES = [(4, "fp32"), (4, "bf16x3"), (10, "fp32"), (10, "bf16x3"), (256, "fp32"), (256, "bf16x3")]
MIN_CAUGHT = {"fp32": 0.9, "bf16x3": 1e-9}
ROW_SLAB = 1 << 20  # rows per float64 slab: SA2's widest layer, 2^20 x 256 x 8 B = 2 GB per tensor
N_PLANT = 24
LOSS_TOL = 2e-5  # of the largest d loss / d dq (test_gpu_loss.py test_training_step_shape_batch_vs_oracle)
# a robot point this close (m) to a branch of the losses takes its branch from fp32 rounding: its environment's
# d loss / d dq may leave LOSS_TOL by that point's share (the loss kernels export no per-point decision).  Half of it
# bounds the HIP robot cloud's position error (asserted), the other half the fp32 rounding of the distances themselves.
HINGE_EPS = 1e-6
DQ_TOL = 1e-5
U_FP32, U_X3 = 1e-6, 3e-5  # per GEMM (float64_policy.KAPPA)
NAMES = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights",
         "cylinder_quats")

X3_MIN_M, X3_MIN_N, X3_MIN_K = 1024, 128, 16  # train_ops._MLPChainFn._use_x3


def chain_u(n):
    """Relative error of an fp32 fma chain of n terms, times sum |a b|: the cdna_hip_programming guide's figure (terms of
    mixed sign) plus the probabilistic bound sqrt(n) 2^-24 of a sum whose terms share one sign (partial sums as large as
    sum |a b|: the rows of a small-batch weight gradient)."""
    return 3.5e-7 * max(1.0, (n / 4096) ** 0.5) + 2.0 ** -24 * n ** 0.5


def _wgrad(kind, M, N, K):
    r = wgrad_route(M, N, K)
    return kind, r.splits, r.tile


def use_x3(x3, M, N, K):  # train_ops._MLPChainFn._use_x3
    return bool(x3) and M >= X3_MIN_M and N >= X3_MIN_N and K >= X3_MIN_K


def _p4(n):
    return (n + 3) // 4 * 4


# the model's dense layers: (stage, layer, N, K) -- model.py MotionPolicyNetwork / MPiNetsPointNet._build_model
HEAD_LINEARS = [("fc", 0, 4096, 1024), ("fc", 3, 2048, 4096), ("fc", 6, 1024, 2048)]
HEAD_CHAINS = {"feature_encoder": [(32, 7), (64, 32), (128, 64), (128, 128), (64, 128)],
               "decoder": [(512, 2112), (256, 512), (128, 256), (7, 128)]}
POOLED_CHAINS = {"SA1": [(64, 4), (64, 64), (64, 64)], "SA2": [(128, 67), (128, 128), (256, 128)],
                 "SA3": [(256, 259), (512, 256), (1024, 512)]}


def training_gemms(B, precision, R1, R2):
    """Every GEMM of one training step: dicts with stage, layer, M, N, K (padded as launched), the forward / input-gradient
    / weight-gradient routes.  R1, R2: packed rows of SA1 / SA2 (data: B * npoint <= R <= B * npoint * nsample)."""
    x3 = precision == "bf16x3"
    out = []
    for st, li, N, K in HEAD_LINEARS:  # train_ops._LinearFn: forward and dX through linear(), dW mpx_linear_wgrad
        Np, Kp = _p4(N), _p4(K)
        out.append(dict(stage=st, layer=li, M=B, N=Np, K=Kp, fwd=linear_route(B, Np, Kp), dx=linear_route(B, Kp, Np),
                        wgrad=_wgrad("linear", B, Np, Kp), x3=False, head=True))
    for st, layers in HEAD_CHAINS.items():  # _MLPChainFn without a pool, fp32 (model.py:597)
        for li, (N, K) in enumerate(layers):
            Np, Kp = _p4(N), _p4(K)
            dx = None if (st == "feature_encoder" and li == 0) else (
                "split-K" if linear_route(B, Kp, Np) == "split-K" else "dact")  # the skinny route of _MLPChainFn.backward
            out.append(dict(stage=st, layer=li, M=B, N=Np, K=Kp, fwd=linear_route(B, Np, Kp), dx=dx,
                            wgrad=_wgrad("linear", B, Np, Kp), x3=False, head=True))
    for st, layers in POOLED_CHAINS.items():  # _MLPChainFn with the pool (_MLPChainFn.forward / .backward)
        M, Q = {"SA1": (R1, B * NP1), "SA2": (R2, B * NP2), "SA3": (B * NP2, B)}[st]
        for li, (N, K) in enumerate(layers):
            Np, Kp = _p4(N), _p4(K)
            lx3 = use_x3(x3, M, Np, Kp)
            last = li == len(layers) - 1
            dx = None if (st == "SA1" and li == 0) else ("pool_dgrad" if last else "dact-x3" if lx3 else "dact")
            wg = ("pool", pool_wgrad_splits(Q, Np, Kp), None) if last else \
                _wgrad("linear-x3" if lx3 else "linear", M, Np, Kp)
            out.append(dict(stage=st, layer=li, M=M, N=Np, K=Kp, fwd="segmax-x3" if (last and lx3) else "segmax" if last else
                            "x3" if lx3 else linear_route(M, Np, Kp), dx=dx, wgrad=wg, x3=lx3, head=False, Q=Q))
    return out


def training_route_table(B, precision, R1=None, R2=None):
    """{route: True / False, or None where the route does not exist in this precision} for one training step.
    R1 / R2 default to the fewest rows (one per query); the routes below do not depend on them at these cases'
    batch sizes except the SA2 split-bf16 layers, which the GPU test reports with the real counts."""
    R1 = B * NP1 if R1 is None else R1
    R2 = B * NP2 if R2 is None else R2
    g = training_gemms(B, precision, R1, R2)
    heads = [e for e in g if e["head"]]
    fc = [e for e in g if e["stage"] == "fc"]
    hchain = [e for e in heads if e["stage"] != "fc" and e["dx"] is not None]
    sa3 = [e for e in g if e["stage"] == "SA3"]
    bf = precision == "bf16x3"
    r = {
        "head forward GEMM on gemv (gemv_fits)": any(e["fwd"] == "gemv" for e in heads),
        "head forward GEMM on split-K (splitk_plan)": any(e["fwd"] == "split-K" for e in heads),
        "head forward GEMM on the tile kernel": any(e["fwd"] == "tile" for e in heads),
        "fc input gradient on gemv": any(e["dx"] == "gemv" for e in fc),
        "fc input gradient on split-K": any(e["dx"] == "split-K" for e in fc),
        "decoder / joint-encoder input gradient: skinny split-K + mpx_act_backward": any(e["dx"] == "split-K" for e in hchain),
        "head weight gradient written directly (one split)": any(e["wgrad"][1] == 1 for e in heads),
        "head weight gradient through split partials": any(e["wgrad"][1] > 1 for e in heads),
        "group-all pooled weight gradient in one split (pool_wgrad_splits S = 1)": sa3[-1]["wgrad"][1] == 1,
        "group-all layers in split bf16 (_use_x3)": any(e["x3"] for e in sa3) if bf else None,
        "bf16x3 weight gradient (mpx_linear_wgrad_bf16x3)": any(e["wgrad"][0] == "linear-x3" for e in g) if bf else None,
    }
    return r


# routes every case takes or leaves the same way, whatever the batch (asserted constant, printed)
def training_route_constants(B, precision, R1=None, R2=None):
    g = training_gemms(B, precision, B * NP1 if R1 is None else R1, B * NP2 if R2 is None else R2)
    pick = lambda st, li: next(e for e in g if e["stage"] == st and e["layer"] == li)
    return {
        "SA1 / SA2 pooled weight gradient in > 1 split (Q >= 512 queries)": pick("SA1", 2)["wgrad"][1] > 1
        and pick("SA2", 2)["wgrad"][1] > 1,
        "group-all dense layers' weight gradient through split partials (>= 512 rows)": all(
            pick("SA3", li)["wgrad"][1] > 1 for li in (0, 1)),
        "64-wide weight-gradient tile (SA1, joint encoder's first layers)": any(e["wgrad"][2] == 64 for e in g),
        "128-wide weight-gradient tile": any(e["wgrad"][2] == 128 for e in g),
        "chain input gradient through mpx_linear_dact": any(e["dx"] == "dact" for e in g),
        "SA1 layers stay fp32 (64 outputs)": not any(e["x3"] for e in g if e["stage"] == "SA1"),
    }


def test_training_cases_cover_every_route():
    """Every route is taken by at least one case and left by at least one, in each precision where it exists, at the
    fewest and at the most packed rows; the constant routes are the same in every case."""
    seen = {}
    for B, prec in CASES:
        for R1, R2 in ((B * NP1, B * NP2), (B * NP1 * NS, B * NP2 * NS)):
            for k, v in training_route_table(B, prec, R1, R2).items():
                if v is not None:
                    seen.setdefault((k, prec), set()).add(bool(v))
            for k, v in training_route_constants(B, prec, R1, R2).items():
                assert v, k
    names = list(training_route_table(256, "fp32"))
    lines = ["training route table (fewest packed rows): " + " | ".join(f"{B}/{p}" for B, p in CASES)]
    for k in names:
        lines.append(f"  {k}: " + " ".join("-" if v is None else "on" if v else "off"
                                           for v in (training_route_table(B, p)[k] for B, p in CASES)))
    print("\n".join(lines))
    missing = [(k, p, sorted(s)) for (k, p), s in seen.items() if s != {False, True}]
    assert not missing, f"routes not both on and off over the cases: {missing}"
    for k in names:
        assert any((k, p) in seen for p in ("fp32", "bf16x3")), k


# ---- the training step and its intermediates ---------------------------------------------------------------------------
def _param_of(fn):
    """The leaf tensor behind a graph edge (through views / reshapes), or None."""
    while fn is not None and not hasattr(fn, "variable"):
        if not any(k in type(fn).__name__ for k in ("View", "Reshape")):
            return None
        fn = fn.next_functions[0][0]
    return None if fn is None else fn.variable


def _stage_of(pname):
    if pname.startswith("point_cloud_encoder.SA_modules."):
        return "SA" + str(int(pname.split(".")[2]) + 1)
    if pname.startswith("point_cloud_encoder.fc_layer."):
        return "fc." + pname.split(".")[2]
    return pname.split(".")[0]


def run_step(tm, batch):
    """The step composed as training_step composes it, with hooks on every HIP node -> (loss, dq, aux, nodes)."""
    xyz, q = batch["xyz"], batch["configuration"]
    aux = {}
    dq = tm(xyz, q, aux=aux)
    y_hat = torch.clamp(q + dq, min=-1, max=1)
    coll, pm = tm.loss_fun(y_hat, *[batch[k] for k in NAMES], batch["supervision"])
    loss = tm.point_match_loss_weight * pm + tm.collision_loss_weight * coll
    names = {id(p): n for n, p in tm.named_parameters()}
    kinds = {"_MLPChainFnBackward": "chain", "_LinearFnBackward": "linear", "_GroupNormLeakyFnBackward": "gn",
             "_PackRowsBackward": "pack"}
    nodes, todo, done = {}, [loss.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in done:
            continue
        done.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
        kind = kinds.get(type(fn).__name__)
        if kind is None:
            continue
        params = [names[id(p)] for p in (_param_of(f) for f, _ in fn.next_functions) if p is not None and id(p) in names]
        key = "SA2.pack" if kind == "pack" else _stage_of(params[0])
        assert key not in nodes, key
        rec = dict(kind=kind, params=params, saved=fn.saved_tensors, node=fn)
        fn.register_hook(lambda gin, gout, rec=rec: rec.update(gin=gin, gout=gout))
        nodes[key] = rec
    return loss, dq, aux, nodes


# ---- float64 per-stage references ---------------------------------------------------------------------------------------
def _act(z, a):
    return z if a == 0 else torch.relu(z) if a == 1 else F.leaky_relu(z, 0.01)


def _slope(y, a):
    """The activation's derivative from its OUTPUT y (mpx_act_backward: ReLU y > 0, LeakyReLU y >= 0)."""
    if a == 0:
        return torch.ones_like(y)
    return (y > 0).to(y.dtype) if a == 1 else torch.where(y >= 0, 1.0, 0.01).to(y.dtype)


def _positive(v, a):
    return v > 0 if a == 1 else v >= 0


class Tally:
    """Worst err / bar per stage and tensor, decision counts, failures (all stages run before the test fails)."""

    def __init__(self):
        self.ratio, self.fail, self.counts = {}, [], {}

    def cmp(self, name, got, ref, bar):
        err = (got.detach().to(ref.device, torch.float64) - ref).abs()
        bar = torch.as_tensor(bar, dtype=torch.float64, device=ref.device).expand_as(err)
        bad = ~(err <= bar)  # (NaN is outside)
        r = float(torch.where(err == 0, 0.0, err / bar).nan_to_num(float("inf")).max()) if err.numel() else 0.0
        self.ratio[name] = max(self.ratio.get(name, 0.0), r)
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            self.fail.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bar, first flat {i}: got "
                             f"{float(got.flatten()[i]):.9g} ref {float(ref.flatten()[i]):.9g} bar {float(bar.flatten()[i]):.3g}")
        return int(bad.sum())

    def count(self, name, n, of):
        a, b = self.counts.get(name, (0, 0))
        self.counts[name] = (a + n, b + of)


def _query_slabs(off_c):
    """Query ranges [q0, q1) of at most ROW_SLAB rows (a query is never split)."""
    Q = off_c.numel() - 1
    q0, out = 0, []
    while q0 < Q:
        q1 = int(torch.searchsorted(off_c, off_c[q0] + ROW_SLAB, right=True)) - 1
        q1 = min(Q, max(q1, q0 + 1))
        out.append((q0, q1))
        q0 = q1
    return out


def chain_stage(name, rec, tm, x3, T, split_control=None):
    """Float64 backward of one _MLPChainFn node from its HIP input, upstream gradient and decisions.  Compares every
    parameter gradient and the input gradient; returns {param: (ref, bar)} and, with ``split_control`` (row ranges of
    wgrad splits of layer 0), the float64 contribution of each range to layer 0's dW."""
    node = rec["node"]
    acts, meta, M, K0, pooled_out, _ = node.meta
    L = len(acts)
    sv = rec["saved"]
    xs = sv[:L]
    params = dict(tm.named_parameters())
    Ws, bs = [], []
    for i in range(L):
        w = params[rec["params"][2 * i]]
        Ws.append(w.detach().double().reshape(w.size(0), -1))
        bs.append(params[rec["params"][2 * i + 1]].detach().double())
    Ns, Ks = [w.size(0) for w in Ws], [w.size(1) for w in Ws]
    g = rec["gout"][0].reshape(-1, Ns[-1])
    gx_hip = rec["gin"][0]
    need_dx = gx_hip is not None
    if pooled_out:
        pooled, arg, offsets = sv[2 * L], sv[2 * L + 1], sv[2 * L + 2]
        off_c = offsets.cpu()
        slabs = [(q0, q1, int(off_c[q0]), int(off_c[q1])) for q0, q1 in _query_slabs(off_c)]
        Q = pooled.size(0)
    else:
        y_last = sv[2 * L]
        slabs = [(r0, min(M, r0 + ROW_SLAB), r0, min(M, r0 + ROW_SLAB)) for r0 in range(0, M, ROW_SLAB)]
    # per layer: u of its forward GEMM and of its input-gradient GEMM, kappa_w of its weight gradient
    u_f, u_dx, kw = [], [], []
    for i in range(L):
        Np, Kp = _p4(Ns[i]), xs[i].size(1)
        lx3 = use_x3(x3, M, Np, Kp)
        u_f.append(U_X3 if lx3 else U_FP32)
        if pooled_out and i == L - 1:  # mpx_pool_dgrad / mpx_pool_wgrad: fp32
            u_dx.append(U_FP32)
            S = pool_wgrad_splits(Q, Np, Kp)
            kw.append(chain_u(_cdiv(Q, S)) + chain_u(S))
        else:
            u_dx.append(U_X3 if lx3 else U_FP32)
            _, S, rps = wgrad_route(M, Np, Kp)
            kw.append(chain_u(rps) + chain_u(S) + (U_X3 if lx3 else 0.0))
    dev_ = g.device
    dW = [torch.zeros_like(w) for w in Ws]
    db = [torch.zeros_like(b) for b in bs]
    mW = [torch.zeros_like(w) for w in Ws]
    mb = [torch.zeros_like(b) for b in bs]
    contrib = None if split_control is None else [torch.zeros_like(Ws[0]) for _ in split_control]
    for q0, q1, r0, r1 in slabs:
        x = [xs[i][r0:r1, :Ks[i]].double() for i in range(L)]
        # forward re-evaluation on the HIP layer inputs: outputs, activation signs, arg-max rows
        for i in range(L):
            z = torch.addmm(bs[i], x[i], Ws[i].t())
            bar = u_f[i] * torch.addmm(bs[i].abs(), x[i].abs(), Ws[i].abs().t())
            if i < L - 1 or not pooled_out:
                hip = (xs[i + 1][r0:r1, :Ns[i]] if i < L - 1 else y_last[r0:r1, :Ns[i]]).double()
                T.cmp(f"{name} forward layer {i}", hip, _act(z, acts[i]), bar)
                if acts[i]:
                    decided = z.abs() > bar
                    wrong = decided & (_positive(z, acts[i]) != _positive(hip, acts[i]))
                    T.count(f"{name} layer {i} activation signs", int(wrong.sum()), int(decided.sum()))
                    if bool(wrong.any()):
                        T.fail.append(f"{name} layer {i}: {int(wrong.sum())} HIP activation signs disagree with float64")
            else:
                y = _act(z, acts[i])
                seg = torch.repeat_interleave(torch.arange(q1 - q0, device=dev_), offsets[q0 + 1:q1 + 1] - offsets[q0:q1])
                idx = seg[:, None].expand(-1, Ns[i])
                ymax = torch.zeros((q1 - q0, Ns[i]), dtype=torch.float64, device=dev_).scatter_reduce_(
                    0, idx, y, "amax", include_self=False)
                bmax = torch.zeros_like(ymax).scatter_reduce_(0, idx, bar, "amax", include_self=False)
                a_loc = arg[q0:q1] - r0
                inside = ((a_loc >= 0) & (a_loc < r1 - r0)).all()
                assert bool(inside), f"{name}: an arg-max row outside its segment's rows"
                seg_ok = bool((seg.gather(0, a_loc.flatten()).view_as(a_loc) == torch.arange(
                    q1 - q0, device=dev_)[:, None]).all())
                assert seg_ok, f"{name}: an arg-max row outside its segment"
                ya, ba = y.gather(0, a_loc), bar.gather(0, a_loc)
                near = ya >= ymax - ba - bmax
                T.count(f"{name} arg-max rows near-max", int((~near).sum()), near.numel())
                if not bool(near.all()):
                    T.fail.append(f"{name}: {int((~near).sum())} HIP arg-max rows are not float64 near-maxima")
                T.cmp(f"{name} forward pooled", pooled[q0:q1], ya, ba)
                if acts[i]:
                    decided = ya.abs() > ba
                    wrong = decided & (_positive(ya, acts[i]) != _positive(pooled[q0:q1].double(), acts[i]))
                    T.count(f"{name} pooled activation signs", int(wrong.sum()), int(decided.sum()))
                    if bool(wrong.any()):
                        T.fail.append(f"{name}: {int(wrong.sum())} HIP pooled activation signs disagree with float64")
            del z, bar
        # backward from the HIP upstream gradient with the HIP decisions
        if pooled_out:
            sl = _slope(pooled[q0:q1].double(), acts[-1])
            gq = g[q0:q1].double()
            a_loc = arg[q0:q1] - r0
            dz = torch.zeros((r1 - r0, Ns[-1]), dtype=torch.float64, device=dev_).scatter_(0, a_loc, gq * sl)
            mdz = torch.zeros_like(dz).scatter_(0, a_loc, gq.abs() * sl)
        else:
            sl = _slope(y_last[r0:r1, :Ns[-1]].double(), acts[-1])
            dz = g[r0:r1].double() * sl
            mdz = g[r0:r1].double().abs() * sl
        for i in range(L - 1, -1, -1):
            dW[i] += dz.t() @ x[i]
            db[i] += dz.sum(0)
            mW[i] += mdz.t() @ x[i].abs()
            mb[i] += mdz.sum(0)
            if i == 0 and contrib is not None:
                for c, (a, b) in zip(contrib, split_control):
                    a, b = max(a, r0), min(b, r1)
                    if a < b:
                        c += dz[a - r0:b - r0].t() @ x[0][a - r0:b - r0]
            if i > 0 or need_dx:
                dx = dz @ Ws[i]
                mdx = mdz @ Ws[i].abs()
                if i > 0:
                    sl = _slope(x[i], acts[i - 1])
                    dz, mdz = dx * sl, mdx * sl
                else:
                    T.cmp(f"{name} dX", gx_hip[r0:r1, :Ks[0]], dx, sum(u_dx) * mdx)
        del x, dz, mdz
    refs = {}
    for i in range(L):
        above = sum(u_dx[i + 1:])
        wn, bn = rec["params"][2 * i], rec["params"][2 * i + 1]
        refs[wn] = (dW[i], (kw[i] + above) * mW[i])
        refs[bn] = (db[i], (kw[i] + above) * mb[i])
    return refs, contrib


def linear_stage(name, rec, tm, T):
    """Float64 dW, db, dX of one _LinearFn (act 0) from its HIP input and upstream gradient."""
    xp, _, _ = rec["saved"]
    params = dict(tm.named_parameters())
    W, b = (params[n].detach().double() for n in rec["params"])
    N, K = W.shape
    x = xp[:, :K].double()
    g = rec["gout"][0].double()
    M = x.size(0)
    _, S, rps = wgrad_route(M, _p4(N), _p4(K))
    kw = chain_u(rps) + chain_u(S)
    T.cmp(f"{name} dX", rec["gin"][0], g @ W, U_FP32 * (g.abs() @ W.abs()))
    return {rec["params"][0]: (g.t() @ x, kw * (g.abs().t() @ x.abs())),
            rec["params"][1]: (g.sum(0), kw * g.abs().sum(0))}


def linear_forward(name, rec, tm, out_hip, T):
    """The HIP output of a _LinearFn (read where the next node saved it) against float64 on its HIP input."""
    xp = rec["saved"][0]
    params = dict(tm.named_parameters())
    W, b = (params[n].detach().double() for n in rec["params"])
    x = xp[:, :W.size(1)].double()
    T.cmp(f"{name} forward", out_hip, torch.addmm(b, x, W.t()), U_FP32 * torch.addmm(b.abs(), x.abs(), W.abs().t()))


def gn_stage(name, rec, y_hip, T):
    """GroupNorm(16) + LeakyReLU backward in float64 from the HIP input, the HIP upstream gradient and the HIP output's
    signs (``y_hip``: the next layer's saved input)."""
    xc, w, b = (t.double() for t in rec["saved"])
    groups, eps = rec["node"].meta
    M, C = xc.shape
    xg = xc.view(M, groups, -1)
    mu = xg.mean(2, keepdim=True)
    r = 1.0 / torch.sqrt(xg.var(2, unbiased=False, keepdim=True) + eps)
    xh = (xg - mu) * r
    a = xh.abs() + (xg.abs() + mu.abs()) * r + xh.abs() * r * r * ((xg - mu).abs() * (xg.abs() + mu.abs())).mean(2, keepdim=True)
    gw, gb = w.view(groups, -1), b.view(groups, -1)
    o = xh * gw + gb
    obar = U_FP32 * (a * gw.abs() + gb.abs())
    y = y_hip.double().view(M, groups, -1)
    T.cmp(f"{name} forward", y, F.leaky_relu(o, 0.01), obar)
    decided = o.abs() > obar
    wrong = decided & ((o >= 0) != (y >= 0))
    T.count(f"{name} activation signs", int(wrong.sum()), int(decided.sum()))
    if bool(wrong.any()):
        T.fail.append(f"{name}: {int(wrong.sum())} HIP activation signs disagree with float64")
    sl = torch.where(y >= 0, 1.0, 0.01).double()
    dy = rec["gout"][0].double().view(M, groups, -1)
    do, mo = dy * sl, dy.abs() * sl
    dxh, m = do * gw, mo * gw.abs()
    dx = r * (dxh - dxh.mean(2, keepdim=True) - xh * (dxh * xh).mean(2, keepdim=True))
    mdx = r * (m + m.mean(2, keepdim=True) + a * (m * a).mean(2, keepdim=True))
    T.cmp(f"{name} dX", rec["gin"][0].view(M, groups, -1), dx, U_FP32 * mdx)
    wn, bn = rec["params"]
    return {wn: ((do * xh).sum(0).reshape(C), U_FP32 * (mo * a).sum(0).reshape(C)),
            bn: (do.sum(0).reshape(C), U_FP32 * mo.sum(0).reshape(C))}


def packed_index(offsets, nbr, npoint, N):
    """For every packed row: the flat (environment, point) it was read from and its query."""
    R = int(offsets[-1])
    rows = torch.arange(R, device=offsets.device)
    qid = torch.searchsorted(offsets, rows, right=True) - 1
    slot = rows - offsets[qid]
    pt = nbr.reshape(-1, nbr.size(-1)).long()[qid, slot]
    return (qid // npoint) * N + pt, qid


def loss_stage(tm, batch, dq, oracle):
    """d loss / d dq in float64 at the HIP dq (the oracle's robot cloud and losses, the clamp in front)."""
    from mpinets_amd import franka_tables as ft
    from mpinets_amd import utils

    lim = torch.tensor(ft.JOINT_LIMITS_REAL, dtype=torch.float64)
    unnorm = lambda x: (x + 1) * (lim[:, 1] - lim[:, 0]) / 2 + lim[:, 0]
    pts, link = ft.link_point_table(4096, with_base_link=False)
    sub = tm.loss_fun.fk_sampler._fixed.cpu().numpy()
    d = dq.detach().cpu().double().requires_grad_(True)
    y = torch.clamp(batch["configuration"].cpu().double() + d, -1, 1)
    cloud = oracle.robot_cloud_torch(unnorm(y), pts, link, sub)
    target = oracle.robot_cloud_torch(unnorm(batch["supervision"].cpu().double()), pts, link, sub)
    npb = {k: batch[k].cpu().numpy() for k in NAMES}
    cf = torch.tensor(oracle.inv_frames_4x4(npb["cuboid_centers"], npb["cuboid_quats"]), dtype=torch.float64)
    yf = torch.tensor(oracle.inv_frames_4x4(npb["cylinder_centers"], npb["cylinder_quats"]), dtype=torch.float64)
    t64 = lambda k: torch.tensor(npb[k], dtype=torch.float64)
    coll = oracle.collision_loss_torch(cloud, cf, t64("cuboid_dims"), yf, t64("cylinder_radii")[..., 0],
                                       t64("cylinder_heights")[..., 0])
    loss = tm.point_match_loss_weight * oracle.point_match_loss_torch(cloud, target) + tm.collision_loss_weight * coll
    loss.backward()
    with torch.no_grad():  # points whose hinge, nearest primitive or nearest face is within fp32 rounding of a switch
        sc, tc = _primitive_sdf(cloud, cf, t64("cuboid_dims"))
        sy, ty = _primitive_sdf(cloud, yf, t64("cylinder_radii")[..., 0], t64("cylinder_heights")[..., 0])
        sp, tie = torch.cat((sc, sy), 1), torch.cat((tc, ty), 1)  # [B, primitives, points]
        two = sp.topk(2, dim=1, largest=False) if sp.size(1) > 1 else None
        sdf = sp.min(1).values
        active = sdf < 0.03
        undecided = (0.03 - sdf).abs() <= HINGE_EPS
        if two is not None:
            near = two.indices[:, :1]
            undecided |= active & (((two.values[:, 1] - two.values[:, 0]) <= HINGE_EPS) | tie.gather(1, near)[:, 0])
        # the point-match loss's L1 term: |a - b| has a kink where a coordinate meets the target's.  The HIP sign of
        # a - b can differ from the float64 one only where |a - b| is within the two clouds' HIP position errors.
        # (Coordinates equal by construction -- a link upstream of every joint that differs -- differ by float64 noise
        # alone, < 1e-12 m, and depend on no joint whose gradient flows: their sign moves nothing.)
        fk = tm.loss_fun.fk_sampler
        a_hip = fk.sample(utils.unnormalize_franka_joints(torch.clamp(batch["configuration"] + dq, min=-1, max=1)))
        b_hip = fk.sample(utils.unnormalize_franka_joints(batch["supervision"]))
        window = (a_hip.cpu().double() - cloud).abs() + (b_hip.cpu().double() - target).abs()
        gap = (cloud - target).abs()
        undecided |= ((gap <= window) & (gap > 1e-12)).any(-1)
    return d.grad, undecided.any(1), cloud.detach()


def _primitive_sdf(points, frames, a, b=None):
    """Per primitive: the float64 signed distance of every point (oracle.sdf_torch's arithmetic) and whether the point
    sits within HINGE_EPS of a branch of it (two faces equally near inside, a clamp at a face plane)."""
    proj = torch.einsum("bmij,bnj->bmni", frames[:, :, :3, :3], points) + frames[:, :, None, :3, 3]
    if b is None:
        valid = ~(a.abs() <= 1e-8).any(-1)
        d = proj.abs() - (a / 2)[:, :, None, :]
    else:
        valid = ~((a.abs() <= 1e-8) | (b.abs() <= 1e-8))
        d = torch.stack((torch.linalg.norm(proj[..., :2], dim=-1) - a[:, :, None], proj[..., 2].abs() - (b / 2)[:, :, None]), -1)
    s = torch.linalg.norm(d.clamp(min=0), dim=-1) + d.max(-1).values.clamp(max=0)
    s = torch.where(valid[:, :, None], s, torch.full_like(s, float("inf")))
    top = d.topk(2, dim=-1).values
    tie = ((top[..., 0] - top[..., 1] <= HINGE_EPS) & (top[..., 0] < 0)) | (d.abs() <= HINGE_EPS).any(-1)
    return s, tie & valid[:, :, None]


def _spread(n, k):
    return sorted({int(v) for v in np.linspace(0, n - 1, k).round()})


def _flagged(planted, ref, bar):
    return bool((~((planted - ref).abs() <= bar)).any())


@pytest.fixture(scope="module")
def train_model(weights):
    from mpinets_amd.model import TrainingMotionPolicyNetwork

    _, sd, _, _ = weights
    from mpinets_amd.robot import FrankaSampler

    tm = TrainingMotionPolicyNetwork(2048, 1.0, 5.0)
    tm.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    tm = tm.to(dev()).train()
    # the loss container's fixed robot-point subset, as its first call would draw it (loss.py), from a seeded host
    # stream: the same points whatever ran before in the session
    np.random.seed(0)
    tm.loss_fun.fk_sampler = FrankaSampler(dev(), num_fixed_points=tm.loss_fun.num_points, use_cache=True,
                                           with_base_link=False)
    return tm


@pytest.mark.gpu
@pytest.mark.parametrize("B,precision", CASES, ids=[f"B{B}-{p}" for B, p in CASES])
def test_training_step_matches_float64_every_stage(weights, train_model, oracle, B, precision):
    from mpinets_amd import _lib

    _, _, gsd, csd = weights
    tm = train_model
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    prob = problem(B)
    g = torch.Generator(device="cpu").manual_seed(B)
    q = prob["q_norm"]
    sup = torch.clamp(q + 0.05 * torch.randn(B, 7, generator=g).to(dev()), -1, 1)
    batch = {"xyz": prob["xyz"], "configuration": q, "supervision": sup, **{k: prob[k] for k in NAMES}}
    tm.set_training_precision(precision)
    try:
        tm.zero_grad(set_to_none=True)
        real = tm.training_step(batch, 0).detach().clone()
        loss, dq, aux, nodes = run_step(tm, batch)
        assert torch.equal(loss.detach(), real), (float(loss), float(real))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        tm.set_training_precision("fp32")
    t_step = time.perf_counter() - t0
    x3 = precision == "bf16x3"
    T = Tally()
    covered = {}

    def cover(stage, refs):
        for n, rb in refs.items():
            assert n not in covered, f"{n} compared twice ({covered[n]}, {stage})"
            covered[n] = stage
            p = dict(tm.named_parameters())[n]
            assert p.grad is not None, n
            T.cmp(f"{stage} d{n.rsplit('.', 2)[-2]}.{n.rsplit('.', 1)[-1]}", p.grad.reshape(rb[0].shape), rb[0], rb[1])

    # -- routes: the mirrored predicates against the library's own scratch sizes --
    lib = _lib.load()
    R1, R2 = int(aux["ball_cnt1"].clamp(min=1).sum()), int(aux["ball_cnt2"].clamp(min=1).sum())
    for e in training_gemms(B, precision, R1, R2):
        kind, S, _ = e["wgrad"]
        if kind == "pool":
            assert lib.mpx_pool_wgrad_scratch(e["Q"], e["N"], e["K"]) == S * (e["N"] * e["K"] + e["N"]), e
        else:
            assert lib.mpx_linear_wgrad_scratch(e["M"], e["N"], e["K"]) == S * (e["N"] * e["K"] + e["N"]), e
        if e["head"]:
            assert (lib.mpx_linear_workspace(e["M"], e["N"], e["K"]) > 0) == (e["fwd"] == "split-K"), e
    routes = training_route_table(B, precision, R1, R2)
    sa2_x3 = [e["layer"] for e in training_gemms(B, precision, R1, R2) if e["stage"] == "SA2" and e["x3"]]
    print(f"\nB={B} {precision}: packed rows SA1 {R1}, SA2 {R2}; SA2 split-bf16 layers {sa2_x3}; routes "
          + ", ".join(k for k, v in routes.items() if v))

    # -- stage 1: the loss --
    ref_dq, undecided, cloud64 = loss_stage(tm, batch, dq, oracle)
    ref_dq, undecided = ref_dq.to(dev()), undecided.to(dev())
    from mpinets_amd.utils import unnormalize_franka_joints

    with torch.no_grad():
        cloud = tm.loss_fun.fk_sampler.sample(unnormalize_franka_joints(torch.clamp(q + dq, min=-1, max=1)))
    pos_err = float((cloud.cpu().double() - cloud64).norm(dim=-1).max())
    assert pos_err <= HINGE_EPS / 2, f"HIP robot cloud {pos_err:.3g} m from float64: HINGE_EPS does not cover it"
    g_dq = nodes["decoder"]["gout"][0]
    out_dq = ~((g_dq.double() - ref_dq).abs() <= LOSS_TOL * ref_dq.abs().max())
    T.count("loss: environments outside the bar / with an undecided robot point", int(out_dq.any(1).sum()),
            int(undecided.sum()))
    T.cmp("loss d/d dq (decided environments)", g_dq[~undecided], ref_dq[~undecided], LOSS_TOL * ref_dq.abs().max())
    assert int(undecided.sum()) <= max(1, B // 20), f"{int(undecided.sum())} of {B} environments undecided"
    # -- stage 2: decoder and joint encoder --
    cover("decoder", chain_stage("decoder", nodes["decoder"], tm, False, T)[0])
    cover("feature_encoder", chain_stage("feature_encoder", nodes["feature_encoder"], tm, False, T)[0])
    gcat = nodes["decoder"]["gin"][0]
    assert torch.equal(nodes["feature_encoder"]["gout"][0], gcat[:, 2048:])
    assert torch.equal(nodes["fc.6"]["gout"][0], gcat[:, :2048])
    # -- stage 3: the fc head, node by node --
    enc_in = nodes["decoder"]["saved"][0][:, :2048]
    linear_forward("fc.0", nodes["fc.0"], tm, nodes["fc.1"]["saved"][0], T)
    linear_forward("fc.3", nodes["fc.3"], tm, nodes["fc.4"]["saved"][0], T)
    linear_forward("fc.6", nodes["fc.6"], tm, enc_in, T)
    for k in ("fc.0", "fc.3", "fc.6"):
        cover(k, linear_stage(k, nodes[k], tm, T))
    cover("fc.1", gn_stage("fc.1", nodes["fc.1"], nodes["fc.3"]["saved"][0], T))
    cover("fc.4", gn_stage("fc.4", nodes["fc.4"], nodes["fc.6"]["saved"][0], T))
    assert torch.equal(nodes["SA3"]["gout"][0], nodes["fc.0"]["gin"][0])
    # -- stage 4: group-all --
    cover("SA3", chain_stage("SA3", nodes["SA3"], tm, x3, T)[0])
    sa3_in = nodes["SA3"]["saved"][0]
    C2 = 256
    # -- stage 5: SA2 --
    pk = nodes["SA2.pack"]
    off2 = nodes["SA2"]["saved"][2 * 3 + 2]
    flat2, qid2 = packed_index(off2, aux["ball_idx2"], NP2, NP1)
    xyz1, f1 = aux["xyz1"], aux["f1"]
    xyz2 = xyz1.gather(1, aux["fps_idx2"].long()[:, :, None].expand(-1, -1, 3))
    rows2 = nodes["SA2"]["saved"][0]
    ref_rows = torch.cat((xyz1.reshape(-1, 3)[flat2] - xyz2.reshape(-1, 3)[qid2], f1.reshape(-1, f1.size(2))[flat2],
                          torch.zeros((flat2.numel(), rows2.size(1) - 3 - f1.size(2)), device=dev())), dim=1)
    assert torch.equal(rows2, ref_rows), "SA2's packed rows differ from torch indexing"
    del ref_rows
    assert torch.equal(sa3_in.view(B, NP2, -1)[:, :, :3], xyz2)
    # the scatter into f1 (and the chain's input gradient is the pack node's upstream gradient)
    gr = pk["gout"][0]
    assert torch.equal(gr, nodes["SA2"]["gin"][0])
    gf1 = pk["gin"][0].reshape(B * NP1, -1)
    Cf = gf1.size(1)
    grd = gr[:, 3:3 + Cf].double()
    ref_f1 = torch.zeros((B * NP1, Cf), dtype=torch.float64, device=dev()).index_add_(0, flat2, grd)
    mag_f1 = torch.zeros_like(ref_f1).index_add_(0, flat2, grd.abs())
    hits = int(torch.bincount(flat2, minlength=B * NP1).max())
    bar_f1 = chain_u(hits) * mag_f1
    T.cmp("SA2 scatter into f1", gf1, ref_f1, bar_f1)
    assert torch.equal(nodes["SA1"]["gout"][0].reshape(B * NP1, -1), gf1)
    # chain, with the dropped-split control's row ranges of layer 0 (mpx_linear_wgrad's split bounds)
    M2, (N0, K0) = rows2.size(0), (128, rows2.size(1))
    _, S0, rps0 = wgrad_route(M2, N0, K0)
    ctrl_splits = _spread(S0, 2 * N_PLANT)
    ranges = [(s * rps0, min(M2, (s + 1) * rps0)) for s in ctrl_splits]
    refs2, contrib = chain_stage("SA2", nodes["SA2"], tm, x3, T, split_control=ranges)
    cover("SA2", refs2)
    # -- stage 6: SA1 --
    off1 = nodes["SA1"]["saved"][2 * 3 + 2]
    flat1, qid1 = packed_index(off1, aux["ball_idx1"], NP1, prob["xyz"].size(1))
    xyz1f = xyz1.reshape(-1, 3)
    pcf = prob["xyz"].reshape(-1, 4)
    ref_rows = torch.cat((pcf[flat1, :3] - xyz1f[qid1], pcf[flat1, 3:]), dim=1)
    assert torch.equal(nodes["SA1"]["saved"][0], ref_rows), "SA1's packed rows differ from torch indexing"
    del ref_rows
    refs1, _ = chain_stage("SA1", nodes["SA1"], tm, False, T)
    cover("SA1", refs1)
    names = [n for n, _ in tm.named_parameters()]
    assert sorted(covered) == sorted(names), sorted(set(names) ^ set(covered))

    # -- controls --
    caught = {}
    w0 = "point_cloud_encoder.SA_modules.1.mlps.0.0.weight"
    ref_w0, bar_w0 = refs2[w0]
    hip_w0 = dict(tm.named_parameters())[w0].grad.reshape(ref_w0.shape).double()
    live = [c for c in contrib if bool((c != 0).any())]  # (a split whose rows carry no gradient drops nothing)
    caught["dropped wgrad split (SA2 layer 0)"] = (sum(_flagged(hip_w0 - c, ref_w0, bar_w0) for c in live), len(live))
    # misrouted pool gradient: SA1's last layer, (query, channel) moved to another row of its segment
    sv1 = nodes["SA1"]["saved"]
    pooled1, arg1 = sv1[2 * 3], sv1[2 * 3 + 1]
    x_last = sv1[2][:, :64].double()
    g1 = nodes["SA1"]["gout"][0].reshape(-1, 64).double() * (pooled1 > 0)
    lens = (off1[1:] - off1[:-1])
    # (query, channel) pairs with a gradient in the largest tenth, in segments of >= 2 rows: at batch 256 one pair is
    # ~1e-5 of a column's sum over 131 K queries, so a small one moves dW by less than that sum's rounding
    nz = g1[g1 != 0].abs()
    thr = nz.kthvalue(max(1, int(0.9 * nz.numel()))).values
    cand = ((lens >= 2)[:, None] & (g1.abs() >= thr)).nonzero()
    wl = "point_cloud_encoder.SA_modules.0.mlps.0.4.weight"
    ref_wl, bar_wl = refs1[wl]
    hip_wl = dict(tm.named_parameters())[wl].grad.reshape(ref_wl.shape).double()
    n_flag = 0
    picks = cand[_spread(cand.size(0), N_PLANT)]
    for qq, c in picks.tolist():
        a = int(arg1[qq, c])
        seg_rows = x_last[int(off1[qq]):int(off1[qq + 1])]
        diff = (seg_rows - x_last[a]).abs().sum(1)
        other = int(off1[qq]) + int(diff.argmax())
        planted = hip_wl.clone()
        planted[c] += g1[qq, c] * (x_last[other] - x_last[a])
        n_flag += _flagged(planted[c], ref_wl[c], bar_wl[c])
    caught["misrouted pool gradient (SA1 last layer)"] = (n_flag, len(picks))
    # lost scatter update: one packed row's contribution missing from the f1 gradient
    live_rows = (gr[:, 3:3 + Cf] != 0).any(1).nonzero().flatten()  # (a row without gradient adds nothing)
    n_flag, rows_ = 0, live_rows[_spread(live_rows.numel(), N_PLANT)].tolist()
    for r in rows_:
        p_ = int(flat2[r])
        planted = gf1[p_].double() - grd[r]
        n_flag += _flagged(planted, ref_f1[p_], bar_f1[p_])
    caught["lost scatter update (f1)"] = (n_flag, len(rows_))

    # -- the training forward at scale against the inference test's per-module references --
    hip = dict(fps_idx1=aux["fps_idx1"], ball_idx1=aux["ball_idx1"], fps_idx2=aux["fps_idx2"], ball_idx2=aux["ball_idx2"],
               f1=f1.detach(), sa3_in=sa3_in.view(B, NP2, -1), f3=aux["f3"].detach())
    fwd = reference(gsd, csd, prob["xyz"], q, hip)
    kappa = KAPPA[precision]
    fr = {}
    try:
        check("train dq", dq.detach(), fwd["dq"].to(dev()), DQ_TOL, fr)
        check("train f1", f1.detach(), fwd["f1"], kappa * fwd["f1_mag"], fr)
        check("train sa3_in", sa3_in.view(B, NP2, -1)[:, :, 3:3 + C2], fwd["f2"], kappa * fwd["f2_mag"], fr)
        check("train f3", aux["f3"].detach(), fwd["f3"], kappa * fwd["f3_mag"], fr)
        check("train encoding", enc_in.cpu(), fwd["encoding"], kappa * fwd["encoding_mag"], fr)
    except AssertionError as e:
        T.fail.append(str(e))
    del fwd

    print(f"B={B} {precision}: worst err/bar " + ", ".join(f"{k} {v:.3g}" for k, v in T.ratio.items()))
    print(f"B={B} {precision}: training forward worst err/bar " + ", ".join(f"{k} {v:.3g}" for k, v in fr.items()))
    print(f"B={B} {precision}: decisions (disagreeing / decided) " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in T.counts.items()))
    print(f"B={B} {precision}: controls flagged " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in caught.items()))
    print(f"B={B} {precision}: step {t_step:.1f} s, total {time.perf_counter() - t0:.1f} s, "
          f"peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    assert not T.fail, "\n".join(T.fail[:20])
    for k, (a, b) in caught.items():
        assert b >= 20, (k, b)
        assert a >= MIN_CAUGHT[precision] * b, f"{k}: only {a} of {b} planted defects flagged"
    for n, p in tm.named_parameters():
        p.grad = None
