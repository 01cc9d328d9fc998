"""The inference forward at the benchmark's batch sizes against a float64 reference, EVERY environment, every element.

The kernels switch launch shapes with the batch size (queries per wave, a persistent grid fed from a device-side unit queue,
whole environments per XCD, the fused group-all chain, XCD remaps in the pairs GEMMs, split-K / gemv heads).  A unit
claimed twice or skipped, a wrong tail unit or a remap that sends a tile to the wrong rows stays deterministic and finite,
so only a full-tensor comparison with an independent reference can see it.  ``route_table`` asks the library which forms
its launchers take (launch_routes.py) and ``test_parametrization_covers_every_route`` makes sure the cases below turn each route on AND off.

Reference: float64, torch ops only (gather, matmul, amax, group_norm, leaky_relu), nothing from ``libmpinets_hip``
except the sampling / neighbour INDICES, which depend on geometry alone (checked bit-exact against the C oracle on a
spread of environments) and, for the per-module checks, the kernels' own input to each module.  ``dq`` is compared with
an end-to-end float64 pass from the point cloud.  f1 (SA1 reads the cloud), sa3_in's feature columns (SA2 from the HIP
f1), f3 (group-all from the HIP sa3_in) and encoding (fc head from the HIP f3) are each compared with a float64
evaluation of THAT module on the kernels' input, so each bar spans one module's layers.  Grouped MLPs and the group-all
module run on the GPU in environment slabs, the heads on the CPU.  Index rows are the padded ones (pointnet2_ops
semantics): padding repeats the first hit, which changes no max, so the same reference also covers the hits-only path of
the call without ``aux``.

Error bars.  ``mag`` is the float64 network evaluated on absolute values: a layer maps ``mag -> |W| mag + |b|``, ReLU /
LeakyReLU pass it through, a max-pool takes the largest ``mag`` over the pooled slots, and GroupNorm (mean mu, sd s,
x_hat = (x - mu) / s, per group) maps it to ``|g| / s * (mag + mean(mag) + |x_hat| * mean(|x - mu| * mag) / s) + |b|``
(first-order perturbation of x, of mu and of s).  SA2's first layer is evaluated per point and per query (the factored
kernels: ``W x_nbr`` and ``W c`` apart), so its coordinate columns carry ``|x_nbr| + |c|`` instead of ``|x_nbr - c|``.
For each layer ``|err_out| <= |W| |err_in| + u_layer |W| |x|``, hence ``|err| <= (sum of u_layer) * mag`` along the chain.
``mag`` starts at the module's input (|cloud rows| for SA1, |HIP f1| for SA2, |HIP sa3_in| for group-all, |HIP f3| for
the fc head), which carries no error of the reference's own: only that module's roundings are in the bar.
  * fp32: u_layer is 0.75 - 1.5e-7 per fp32 MFMA chain at K <= 1024 (cdna_hip_programming guide); three GEMMs per module
    (and two GroupNorms in the fc head, K up to 4096): kappa = 1e-6.
  * bf16x3: each product is hi*hi + hi*lo + lo*hi of bf16 halves, 2^-16 relative per split product (csrc/dense_bf16.hip
    header): kappa = 3e-5.
``dq`` is held to the project's absolute 1e-5 in both precisions.
The worst case is wide where a module has many wide layers: the fc head's bar is about half a typical encoding value in
fp32 and well above it in bf16x3, so that check guards gross defects only (wrong rows, NaN); the bf16x3 group-all bar is
about half a typical f3 value.  The dropped-neighbour controls print how many planted single-row drops each bar flags.
"""
import time

import numpy as np
import pytest
import torch

from float64_policy import (KAPPA, NP1, NP2, NS, _cdiv, _gather, _sa_layers, check, cu_count,  # noqa: F401
                            offending_envs, problem, reference, sa1_rows, sa2_rows, weights)
from launch_routes import linear_route, sa_route

pytestmark = pytest.mark.gpu

# share of the planted dropped neighbours (every query of the last environment whose max moves) the bars must flag.
# fp32 bars sit at ~1 % of a typical value and catch nearly all of them; bf16x3 bars are 30x wider (2^-16 per split
# product, worst case) and let the smaller moves through -- there the control asserts only that the comparator sees drops
# at all, and the share is printed.
MIN_CAUGHT = {"fp32": 0.9, "bf16x3": 1e-9}
DQ_TOL = 1e-5

# (B, precision, elide_padding)
CASES = [
    (8192, "fp32", True),     # the headline configuration
    (8192, "bf16x3", True),
    (8192, "fp32", False),    # all 128 slots: the bench's dense-scene figure, non-packed sa_mlp_kernel for SA1
    (1027, "fp32", True),     # queue on, B % 8 != 0 (no XCD mapping), tail units, decoder not split-K
    (1027, "bf16x3", True),
    (256, "fp32", True),      # group-all chain threshold, queue off, large Q
    (256, "bf16x3", True),
    (4, "fp32", True),        # the small-batch side of every switch: small Q, gemv heads
    (4, "bf16x3", True),
]

SA3_CHAIN_MIN_BATCH = 256               # model.py (asserted equal below)
PAIRS_BM = 256                          # rows per tile of the bf16x3 pairs GEMMs (gridDim.y = cdiv(rows, 256))


def route_table(B, precision, elide, cus, aux):
    """{route: True / False, or None where the route does not exist in this precision} for one forward call."""
    fp32 = precision == "fp32"
    r = {}
    # -- SA1 grouped MLP (mpx_sa_mlp; mpx_sa_mlp_bf16x3): counts given = the packed kernel; without them every slot is walked --
    sa1 = sa_route(cus, B, NP1, NS, elide, 1, precision, False)
    r["SA1 non-packed sa_mlp_kernel (padding kept)"] = (not sa1.packed) if fp32 else None
    r["SA1 large Q (32 queries / wave)"] = bool(sa1.packed and sa1.Q == 32) if fp32 else None
    r["SA1 persistent grid from the unit queue"] = bool(sa1.packed and sa1.persistent) if fp32 else None
    r["SA1 whole environments per XCD (bpe / wpe)"] = bool(sa1.packed and sa1.per_env > 0) if fp32 else sa1.per_env > 0
    # -- SA2 grouped MLP, factored (mpx_sa_mlp_factored; mpx_sa_mlp_bf16x3_factored is always persistent) --
    sa2 = sa_route(cus, B, NP2, NS, True, 64, precision, True)
    r["SA2 large Q (8 queries / wave)"] = (sa2.Q == 8) if fp32 else None
    r["SA2 persistent grid from the unit queue"] = bool(sa2.persistent) if fp32 else None
    r["SA2 whole environments per XCD (bpe / xcd_aware)"] = sa2.per_env > 0 if fp32 else bool(sa2.xcd_aware)
    # -- group-all module (model.py MPiNetsPointNet.forward) --
    r["group-all as one kernel (mpx_sa3_chain)"] = (B >= SA3_CHAIN_MIN_BATCH) if fp32 else None
    r["bf16x3 group-all last layer: XCD remap (gridDim.y % 8 == 0)"] = None if fp32 else _cdiv(B * NP2, PAIRS_BM) % 8 == 0
    r["bf16x3 fc pairs GEMMs: XCD remap"] = None if (fp32 or aux) else _cdiv(B, PAIRS_BM) % 8 == 0
    r["bf16x3 pooled straight to pairs + _fc_through_pairs"] = None if fp32 else not aux
    # -- heads --
    r["fc 1024->4096 split-K"] = (linear_route(B, 4096, 1024) == "split-K") if fp32 else None
    r["decoder 2112->512 split-K"] = (linear_route(B, 512, 2112) == "split-K") if fp32 else None
    r["decoder 2112->512 gemv"] = (linear_route(B, 512, 2112) == "gemv") if fp32 else None
    r["decoder 512->256 split-K (fp32 in both modes)"] = linear_route(B, 256, 512) == "split-K"
    r["decoder 512->256 gemv (fp32 in both modes)"] = linear_route(B, 256, 512) == "gemv"
    # -- neighbour search: hits-only rows for the engine's call (no aux, padding elided) --
    r["hits-only ball query (mpx_ball_query_hits)"] = elide and not aux
    return r


def test_parametrization_covers_every_route():
    """Every route is taken by at least one case and left by at least one, in each precision where it exists."""
    from mpinets_amd import model as model_mod

    assert model_mod.SA3_CHAIN_MIN_BATCH == SA3_CHAIN_MIN_BATCH
    cus = cu_count()
    seen = {}
    for B, prec, elide in CASES:
        for aux in (False, True):  # every case makes the engine's call and the aux call
            for k, v in route_table(B, prec, elide, cus, aux).items():
                if v is not None:
                    seen.setdefault((k, prec), set()).add(bool(v))
    names = route_table(8192, "fp32", True, cus, False).keys()
    lines = [f"route table on {cus} CUs (engine call, no aux):", "  " + " | ".join(f"{B}/{p}{'' if e else '/padded'}"
                                                                                for B, p, e in CASES)]
    for k in names:
        row = [route_table(B, p, e, cus, False)[k] for B, p, e in CASES]
        lines.append(f"  {k}: " + " ".join("-" if v is None else "on" if v else "off" for v in row))
    print("\n".join(lines))
    missing = [(k, p, sorted(s)) for (k, p), s in seen.items() if s != {False, True}]
    assert not missing, f"routes not both on and off over the cases: {missing}"
    for k in names:
        assert any((k, p) in seen for p in ("fp32", "bf16x3")), k


def slot_rows(x, layers):
    """Per-slot activations of a grouped MLP (no pool): x [Q, S, Cin] -> [Q, S, Cout]."""
    for w, b in layers:
        x = torch.relu(x @ w.t() + b)
    return x


def dropped_neighbour_control(acts, cnt, hip_full, ref_full, bar_full, e):
    """Sensitivity control: in a copy of the kernel's pooled rows, replace EVERY query of environment ``e`` whose max
    changes when its last hit is dropped (cnt >= 2) with that pool -- what a kernel skipping the query's last row would
    write.  The comparator must flag environment ``e`` alone, and only planted queries.  -> (flagged, planted)."""
    slot = torch.arange(acts.size(1), device=acts.device)
    keep = (slot[None, :] < (cnt[:, None] - 1))[:, :, None]
    drop = torch.where(keep, acts, torch.full_like(acts, -1.0)).amax(1)  # (post-ReLU values are >= 0)
    changed = (cnt >= 2) & (drop != acts.amax(1)).any(1)  # (padding repeats the first hit: the max over every slot)
    assert changed.any(), "no query of the environment changes its pool when its last hit is dropped"
    planted = hip_full.clone()
    planted[e][changed] = drop[changed].to(planted.dtype)
    envs, bad = offending_envs(planted, ref_full, bar_full)
    flagged = bad[e].any(1)
    assert envs == [e], envs
    assert not (flagged & ~changed).any(), "queries flagged that were not planted"
    return int(flagged.sum()), int(changed.sum())


def spread(B):
    return sorted({e for s in (0, B // 2, B - 8) for e in range(s, s + 8) if 0 <= e < B})


# ---- the cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,precision,elide", CASES, ids=[f"B{B}-{p}{'' if e else '-padded'}" for B, p, e in CASES])
def test_forward_matches_float64_every_environment(weights, oracle, B, precision, elide):
    mdl, sd, gsd, csd = weights
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    prob = problem(B)
    xyz, qn = prob["xyz"], prob["q_norm"]
    cus = cu_count()
    print(f"\nB={B} {precision}{'' if elide else ' padded'}: routes "
          + ", ".join(k for k, v in route_table(B, precision, elide, cus, False).items() if v))
    mdl.set_precision(precision).set_elide_padding(elide)
    try:
        with torch.no_grad():
            dq = mdl(xyz, qn).clone()  # the call RolloutEngine.step() makes
            counts = tuple(c.clone() for c in mdl.point_cloud_encoder.last_counts)
            aux = {}
            dq_aux = mdl(xyz, qn, aux=aux)
        torch.cuda.synchronize()
    finally:
        mdl.set_precision("fp32").set_elide_padding(True)
    assert torch.equal(aux["ball_cnt1"], counts[0]) and torch.equal(aux["ball_cnt2"], counts[1])
    assert torch.equal(dq_aux, dq), float((dq_aux - dq).abs().max())

    # indices bit-exact against the C oracle on every position of an 8-env XCD group, the middle and the tail
    sel = spread(B)
    pc_np = xyz[sel].cpu().numpy()
    fi1 = oracle.fps(pc_np, NP1)
    np.testing.assert_array_equal(aux["fps_idx1"][sel].cpu().numpy(), fi1)
    x1 = oracle.gather_points(pc_np, fi1)
    bi1, bc1 = oracle.ball_query(x1, pc_np[:, :, :3], 0.05, NS, return_counts=True)
    np.testing.assert_array_equal(aux["ball_idx1"][sel].cpu().numpy(), bi1)
    np.testing.assert_array_equal(aux["ball_cnt1"][sel].cpu().numpy(), bc1)
    fi2 = oracle.fps(x1, NP2)
    np.testing.assert_array_equal(aux["fps_idx2"][sel].cpu().numpy(), fi2)
    bi2, bc2 = oracle.ball_query(oracle.gather_points(x1, fi2), x1, 0.3, NS, return_counts=True)
    np.testing.assert_array_equal(aux["ball_idx2"][sel].cpu().numpy(), bi2)
    np.testing.assert_array_equal(aux["ball_cnt2"][sel].cpu().numpy(), bc2)

    ref = reference(gsd, csd, xyz, qn, aux)
    kappa = KAPPA[precision]
    ratios = {}
    C2 = ref["f2"].size(2)
    assert torch.equal(aux["sa3_in"][:, :, :3], _gather(xyz[:, :, :3], aux["fps_idx1"]).gather(
        1, aux["fps_idx2"].long()[:, :, None].expand(-1, -1, 3)))
    f2h = aux["sa3_in"][:, :, 3:3 + C2]
    check("dq", dq, ref["dq"], DQ_TOL, ratios)
    check("f1", aux["f1"], ref["f1"], kappa * ref["f1_mag"], ratios)
    check("sa3_in", f2h, ref["f2"], kappa * ref["f2_mag"], ratios)
    check("f3", aux["f3"], ref["f3"], kappa * ref["f3_mag"], ratios)
    check("encoding", aux["encoding"], ref["encoding"], kappa * ref["encoding_mag"], ratios)

    # sensitivity control (a): dropped neighbours in SA1 (f1) and in SA2 (sa3_in) of the last environment
    e = B - 1
    x, xyz1 = sa1_rows(xyz[e:e + 1], aux["fps_idx1"][e:e + 1], aux["ball_idx1"][e:e + 1])
    caught = {"f1": dropped_neighbour_control(slot_rows(x[0], _sa_layers(gsd, 0)), aux["ball_cnt1"][e].long(),
                                              aux["f1"], ref["f1"], kappa * ref["f1_mag"], e)}
    f1e = aux["f1"][e:e + 1].double()
    x, _, _ = sa2_rows(xyz1, f1e, None, aux["fps_idx2"][e:e + 1], aux["ball_idx2"][e:e + 1])
    caught["sa3_in"] = dropped_neighbour_control(slot_rows(x[0], _sa_layers(gsd, 1)), aux["ball_cnt2"][e].long(),
                                                 f2h, ref["f2"], kappa * ref["f2_mag"], e)
    del x
    for k, (n_flag, n_plant) in caught.items():  # (a drop that moves a max by less than the rounding bar is invisible)
        assert n_flag >= MIN_CAUGHT[precision] * n_plant, f"{k}: only {n_flag} of {n_plant} dropped neighbours flagged"
    # (b): two environments' dq rows swapped
    i, j = B // 2 - 1 if B > 2 else 0, B - 1
    assert (ref["dq"][i] - ref["dq"][j]).abs().max() > 2 * DQ_TOL
    sw = dq.clone()
    sw[[i, j]] = dq[[j, i]]
    assert offending_envs(sw, ref["dq"], DQ_TOL)[0] == sorted({i, j})

    print(f"B={B} {precision}{'' if elide else ' padded'}: worst err/bar " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items())
          + "; dropped neighbours flagged " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in caught.items())
          + f"; {time.perf_counter() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


def test_reference_matches_the_oracle(weights, oracle):
    """Anchor of the restatement: on three environments the float64 reference equals oracle.policy_forward (its own C
    sampler, float64 accumulate / float32 store) within 1e-6 -- a wrong label column or centring would show here."""
    mdl, sd, gsd, csd = weights
    B = 256
    prob = problem(B)
    sel = [0, 129, 255]
    xyz, qn = prob["xyz"][sel].contiguous(), prob["q_norm"][sel].contiguous()
    aux = {}
    with torch.no_grad():
        mdl(xyz, qn, aux=aux)
    ref = reference(gsd, csd, xyz, qn, aux)
    odq, oaux = oracle.policy_forward(sd, xyz.cpu().numpy(), qn.cpu().numpy())
    np.testing.assert_allclose(ref["dq"].numpy(), odq, rtol=0, atol=1e-6)
    np.testing.assert_array_equal(aux["fps_idx1"].cpu().numpy(), oaux["sa1"]["fps_idx"])
