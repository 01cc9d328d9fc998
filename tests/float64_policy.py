"""The float64 policy of the parity tests, shared by the inference-forward test (test_gpu_batch_parity.py) and the
training-step test (test_gpu_training_parity.py): the benchmark problem and the seeded weights, the per-module float64
references with their magnitude pass (see test_gpu_batch_parity.py's docstring for the bars) and the per-element
comparator.  (Which kernel a shape takes is asked of the library: launch_routes.py.)  A plain module, imported by the tests: it holds no test of its own."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

KAPPA = {"fp32": 1e-6, "bf16x3": 3e-5}  # relative rounding bar per module (see the forward test's docstring)
SLAB = 64  # environments per float64 slab: SA1's padded rows, 64 * 512 * 128 x 64 channels x 8 B = 2.1 GB per activation
NP1, NP2, NS = 512, 128, 128            # model.py MPiNetsPointNet._build_model: npoint / nsample of SA1, SA2


def _cdiv(a, b):
    return -(-a // b)


def cu_count():
    import ctypes

    from mpinets_amd import _lib

    n = ctypes.c_int(0)
    assert _lib.load().mpx_device_info(None, 0, ctypes.addressof(n), None) == 0
    return n.value


# ---- fixtures ------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


_PROBLEMS = {}


def problem(B):
    if B not in _PROBLEMS:
        from mpinets_amd.scenes import make_problem_batch

        _PROBLEMS.clear()  # (cases are ordered by B: one problem alive at a time)
        _PROBLEMS[B] = make_problem_batch(B, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16, device=dev(),
                                          device_clouds=True)
    return _PROBLEMS[B]


@pytest.fixture(scope="module")
def weights():
    import seeded_weights
    from mpinets_amd.model import MotionPolicyNetwork

    m = MotionPolicyNetwork()
    sd = seeded_weights.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=0)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.to(dev()).eval()
    gpu = {k: torch.from_numpy(v).double().to(dev()) for k, v in sd.items() if ".SA_modules." in k}
    cpu = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    return m, sd, gpu, cpu


# ---- the float64 reference --------------------------------------------------------------------------------------------
def _sa_layers(sd, i):
    p = f"point_cloud_encoder.SA_modules.{i}.mlps.0."
    return [(sd[p + f"{k}.weight"].reshape(sd[p + f"{k}.weight"].shape[0], -1), sd[p + f"{k}.bias"]) for k in (0, 2, 4)]


def _mlp_pool(x, m, layers, dim):
    """Conv1x1 + ReLU stack on the last axis, max over ``dim``; the same on magnitudes (``m`` None: values only)."""
    shape = x.shape[:-1]
    x = x.reshape(-1, x.size(-1))
    m = None if m is None else m.reshape(-1, m.size(-1))
    for w, b in layers:
        x = torch.relu(torch.addmm(b, x, w.t()))
        if m is not None:
            m = torch.addmm(b.abs(), m, w.abs().t())
    return x.view(*shape, -1).amax(dim), None if m is None else m.view(*shape, -1).amax(dim)


def _gather(t, idx):
    """t [E, N, C], idx [E, ...] -> [E, ..., C]."""
    E = t.size(0)
    flat = idx.reshape(E, -1).long()
    return torch.gather(t, 1, flat[:, :, None].expand(-1, -1, t.size(2))).view(*idx.shape, t.size(2))


def _group_norm_mag(x, m, gn_w, gn_b, groups, eps):
    B, C = x.shape
    xg, mg = x.view(B, groups, -1), m.view(B, groups, -1)
    mu = xg.mean(2, keepdim=True)
    s = torch.sqrt(xg.var(2, unbiased=False, keepdim=True) + eps)
    xh = (xg - mu) / s
    mo = (mg + mg.mean(2, keepdim=True) + xh.abs() * ((xg - mu).abs() * mg).mean(2, keepdim=True) / s) / s
    return (mo.view(B, C) * gn_w.abs() + gn_b.abs())


def sa1_rows(pc, fps1, nb1):
    """SA1's grouped rows [E, 512, 128, 4] = [xyz - centre | label] (the reference's channel order), float64."""
    p = pc.double()
    xyz = p[:, :, :3].contiguous()
    xyz1 = _gather(xyz, fps1)
    return torch.cat((_gather(xyz, nb1) - xyz1[:, :, None, :], _gather(p[:, :, 3:].contiguous(), nb1)), dim=3), xyz1


def sa2_rows(xyz1, f1, f1_mag, fps2, nb2):
    """SA2's grouped rows [E, 128, 128, 3 + 64] = [xyz1 - centre | f1] and their magnitudes (None without ``f1_mag``).
    The factored kernels form ``W x_nbr`` and ``W c`` apart: the coordinate columns carry ``|x_nbr| + |c|``."""
    xyz2 = _gather(xyz1, fps2)
    g = _gather(xyz1, nb2)
    x = torch.cat((g - xyz2[:, :, None, :], _gather(f1, nb2)), dim=3)
    m = None if f1_mag is None else torch.cat((g.abs() + xyz2.abs()[:, :, None, :], _gather(f1_mag, nb2)), dim=3)
    return x, m, xyz2


def fc_head(csd, x, m):
    """fc_layer (Linear, GroupNorm(16), LeakyReLU, Linear, GroupNorm(16), LeakyReLU, Linear) on the CPU in float64."""
    pf = "point_cloud_encoder.fc_layer."
    for li, gi in ((0, 1), (3, 4), (6, None)):
        w, b = csd[pf + f"{li}.weight"], csd[pf + f"{li}.bias"]
        x = torch.addmm(b, x, w.t())
        if m is not None:
            m = torch.addmm(b.abs(), m, w.abs().t())
        if gi is not None:
            gw, gb = csd[pf + f"{gi}.weight"], csd[pf + f"{gi}.bias"]
            if m is not None:
                m = _group_norm_mag(x, m, gw, gb, 16, 1e-5)
            x = F.leaky_relu(F.group_norm(x, 16, gw, gb, eps=1e-5))
    return x, m


def reference(gsd, csd, pc, qn, hip):
    """float64 references from the kernels' indices (``hip``: fps_idx1 / ball_idx1 (padded) / fps_idx2 / ball_idx2
    (padded) and the module outputs f1 / sa3_in / f3 of the aux forward).

    * end to end, from the point cloud: ``dq`` (the project's bar) -- and f1, since SA1 reads the cloud itself;
    * per module, from the kernels' own input to that module: f2 from the HIP f1, f3 from the HIP sa3_in, encoding from
      the HIP f3.  Each bar then spans that module's layers only (mag restarts at |input|), so a defect inside one module
      is measured against that module's rounding, not against the slack accumulated by every layer before it.
    -> float64 values and magnitudes: f1, f2, f3 on the GPU; encoding, dq on the CPU."""
    B = pc.size(0)
    L1, L2, L3 = (_sa_layers(gsd, i) for i in range(3))
    C2 = L2[-1][0].size(0)
    parts = {k: [] for k in ("f1", "f1_mag", "f2", "f2_mag", "f3", "f3_mag", "f3_e2e")}
    for b0 in range(0, B, SLAB):
        sl = slice(b0, min(B, b0 + SLAB))
        x, xyz1 = sa1_rows(pc[sl], hip["fps_idx1"][sl], hip["ball_idx1"][sl])
        a, am = _mlp_pool(x, x.abs(), L1, 2)                         # [E, 512, 64]
        del x
        # end to end (values only): SA2 and group-all on the reference's own f1
        x, _, xyz2 = sa2_rows(xyz1, a, None, hip["fps_idx2"][sl], hip["ball_idx2"][sl])
        c, _ = _mlp_pool(x, None, L2, 2)
        del x
        e, _ = _mlp_pool(torch.cat((xyz2, c), dim=2), None, L3, 1)   # group-all: absolute coordinates | features
        # per module: SA2 on the HIP f1, group-all on the HIP sa3_in
        f1h = hip["f1"][sl].double()
        x, xm, _ = sa2_rows(xyz1, f1h, f1h.abs(), hip["fps_idx2"][sl], hip["ball_idx2"][sl])
        cm_v, cm_m = _mlp_pool(x, xm, L2, 2)                         # [E, 128, 256]
        del x, xm
        h = hip["sa3_in"][sl, :, :3 + C2].double()
        em_v, em_m = _mlp_pool(h, h.abs(), L3, 1)
        for k, t in (("f1", a), ("f1_mag", am), ("f2", cm_v), ("f2_mag", cm_m), ("f3", em_v), ("f3_mag", em_m),
                     ("f3_e2e", e)):
            parts[k].append(t)
    out = {k: torch.cat(v) for k, v in parts.items()}
    f3h = hip["f3"].double().cpu()
    out["encoding"], out["encoding_mag"] = fc_head(csd, f3h, f3h.abs())
    enc, _ = fc_head(csd, out.pop("f3_e2e").cpu(), None)
    q = qn.double().cpu()
    for k in (0, 2, 4, 6, 8):
        q = torch.addmm(csd[f"feature_encoder.{k}.bias"], q, csd[f"feature_encoder.{k}.weight"].t())
        q = F.leaky_relu(q) if k != 8 else q
    y = torch.cat((enc, q), dim=1)
    for k in (0, 2, 4, 6):
        y = torch.addmm(csd[f"decoder.{k}.bias"], y, csd[f"decoder.{k}.weight"].t())
        y = F.leaky_relu(y) if k != 6 else y
    out["dq"] = y
    return out


# ---- comparator ------------------------------------------------------------------------------------------------------
def offending_envs(got, ref, bar):
    """-> (sorted environment indices with any element outside its bar, per-element bool mask).  NaN is outside."""
    err = (got.to(ref.device, torch.float64) - ref).abs()
    bad = ~(err <= bar)
    return bad.flatten(1).any(1).nonzero().flatten().tolist(), bad


def check(name, got, ref, bar, ratios):
    """Assert every element is inside its bar; record the worst err / bar."""
    err = (got.to(ref.device, torch.float64) - ref).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64, device=ref.device).expand_as(err)
    ratio = err / bar
    ratios[name] = float(ratio.max())
    envs, bad = offending_envs(got, ref, bar)
    if envs:
        e = envs[0]
        r = ratio[e].nan_to_num(float("inf"))
        w = tuple(int(i) for i in np.unravel_index(int(r.argmax()), tuple(r.shape)))
        raise AssertionError(
            f"{name}: {len(envs)} environment(s) outside the bar, first env {e} (B % 8 position {e % 8}): worst element "
            f"{w} got {float(got[e][w]):.9g} ref {float(ref[e][w]):.9g} err {float(err[e][w]):.3g} "
            f"bar {float(bar[e][w]):.3g}; envs {envs[:16]}{' ...' if len(envs) > 16 else ''}")
