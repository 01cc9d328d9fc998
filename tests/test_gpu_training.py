"""Row N1: the differentiable forward + training_step of the engine vs a float64 torch-autograd oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights",
         "cylinder_quats")


def dev():
    return torch.device("cuda:0")


def small_batch(B, seed):
    from mpinets_amd.scenes import make_problem_batch

    prob = make_problem_batch(B, seed=seed, device=dev(), kinds=("tabletop", "cubby"), M1=12, M2=8)
    rng = np.random.default_rng(seed)
    sup = torch.clamp(prob["q_norm"] + torch.tensor(rng.normal(scale=0.05, size=(B, 7)), dtype=torch.float32,
                                                    device=dev()), -1, 1)
    batch = {"xyz": prob["xyz"], "configuration": prob["q_norm"], "supervision": sup}
    batch.update({k: prob[k] for k in NAMES})
    return batch


def test_segment_ops_match_torch():
    from mpinets_amd.train_ops import _SegmentMax

    g = torch.Generator(device="cpu").manual_seed(0)
    lens = torch.randint(1, 40, (50,), generator=g)
    off = torch.zeros(51, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    y = torch.randn(int(off[-1]), 96, generator=g)
    y[3] = y[2]  # a tie inside one segment: first row wins
    yd = y.to(dev()).requires_grad_(True)
    out = _SegmentMax.apply(yd, off.to(dev()), 50)
    w = torch.randn(50, 96, generator=g)
    (out * w.to(dev())).sum().backward()
    yc = y.clone().requires_grad_(True)
    ref = torch.stack([yc[off[i]:off[i + 1]].max(0).values for i in range(50)])
    (ref * w).sum().backward()
    assert torch.equal(out.cpu(), ref.detach())
    assert torch.equal(yd.grad.cpu(), yc.grad)


def test_training_forward_equals_inference_forward():
    """Same weights, same cloud: the differentiable path and the fused engine path agree to fp32 round-off."""
    from mpinets_amd.model import MotionPolicyNetwork

    torch.manual_seed(0)
    mdl = MotionPolicyNetwork().to(dev())
    batch = small_batch(3, 1)
    mdl.train()
    y_train = mdl(batch["xyz"], batch["configuration"])
    assert y_train.requires_grad
    mdl.eval()
    with torch.no_grad():
        y_inf = mdl(batch["xyz"], batch["configuration"])
    np.testing.assert_allclose(y_train.detach().cpu().numpy(), y_inf.cpu().numpy(), atol=1e-5)  # north-star tolerance


def test_training_step_gradients_match_oracle(oracle):
    from mpinets_amd import franka_tables as ft
    from mpinets_amd.model import TrainingMotionPolicyNetwork

    torch.manual_seed(1)
    mdl = TrainingMotionPolicyNetwork(num_robot_points=2048, point_match_loss_weight=1.0, collision_loss_weight=5.0)
    mdl = mdl.to(dev()).train()
    B = 2
    batch = small_batch(B, 3)
    loss = mdl.training_step(batch, 0)
    loss.backward()
    assert set(mdl.logged) == {"point_match_loss", "collision_loss", "val_loss"}

    # ---- oracle: float64 autograd over the restated network + restated losses
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mdl.state_dict().items()}
    q = batch["configuration"].cpu().double()
    dq = oracle.policy_forward_torch(sd, batch["xyz"].cpu().numpy(), q)
    y = torch.clamp(q + dq, -1, 1)
    lim = torch.tensor(ft.JOINT_LIMITS_REAL, dtype=torch.float64)
    unnorm = lambda x: (x + 1) * (lim[:, 1] - lim[:, 0]) / 2 + lim[:, 0]
    pts, link = ft.link_point_table(4096, with_base_link=False)
    sub = mdl.loss_fun.fk_sampler._fixed.cpu().numpy()
    cloud = oracle.robot_cloud_torch(unnorm(y), pts, link, sub)
    target = oracle.robot_cloud_torch(unnorm(batch["supervision"].cpu().double()), pts, link, sub)
    npb = {k: batch[k].cpu().numpy() for k in NAMES}
    cf = torch.tensor(oracle.inv_frames_4x4(npb["cuboid_centers"], npb["cuboid_quats"]), dtype=torch.float64)
    yf = torch.tensor(oracle.inv_frames_4x4(npb["cylinder_centers"], npb["cylinder_quats"]), dtype=torch.float64)
    t64 = lambda k: torch.tensor(npb[k], dtype=torch.float64)
    coll = oracle.collision_loss_torch(cloud, cf, t64("cuboid_dims"), yf, t64("cylinder_radii")[..., 0],
                                       t64("cylinder_heights")[..., 0])
    pm = oracle.point_match_loss_torch(cloud, target)
    ref_loss = pm + 5.0 * coll
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    assert abs(mdl.logged["collision_loss"].item() - coll.item()) < 1e-6
    worst = 0.0
    for name, p in mdl.named_parameters():
        ref = sd[name].grad
        assert p.grad is not None and ref is not None, name
        scale = ref.abs().max().item()
        err = (p.grad.cpu().double() - ref).abs().max().item()
        assert err <= 2e-4 * scale + 1e-9, (name, err, scale)
        worst = max(worst, err / (scale + 1e-30))
    print("worst relative gradient error", worst)


def test_gradient_step_decreases_loss_as_predicted():
    """End-to-end directional-derivative check on the device: a small step along -grad lowers the training loss by
    ~ lr * |grad|^2 (first order), and a short SGD run keeps lowering it."""
    from mpinets_amd.model import TrainingMotionPolicyNetwork

    torch.manual_seed(2)
    mdl = TrainingMotionPolicyNetwork(2048, 1.0, 1.0).to(dev()).train()
    batch = small_batch(4, 5)
    batch["configuration"] = batch["configuration"].clamp(-0.7, 0.7)
    batch["supervision"] = batch["configuration"] + 0.2  # something to learn: every joint shifted
    params = [p for p in mdl.parameters()]
    loss0 = mdl.training_step(batch, 0)
    grads = torch.autograd.grad(loss0, params)
    g2 = sum((g.double() ** 2).sum() for g in grads).item()
    lr = 2e-3 / g2 ** 0.5  # parameter step of norm 2e-3
    with torch.no_grad():
        for p, g in zip(params, grads):
            p.sub_(lr * g)
        loss1 = mdl.training_step(batch, 0)
    predicted = lr * g2
    assert loss1.item() < loss0.item()
    assert 0.5 * predicted < loss0.item() - loss1.item() < 1.5 * predicted, (loss0.item(), loss1.item(), predicted)
    opt = torch.optim.SGD(mdl.parameters(), lr=lr)
    losses = [loss1.item()]
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        loss = mdl.training_step(batch, 0)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses


def test_linear_train_matches_torch_autograd():
    """Hand-written dense forward/backward (mpx_linear, mpx_act_backward, mpx_linear_wgrad) vs torch in float64."""
    from mpinets_amd.train_ops import linear_train

    rng = np.random.default_rng(0)
    for (M, N, K, act) in [(300, 64, 4, 1), (1000, 128, 67, 1), (129, 7, 128, 0), (4096, 512, 259, 1), (77, 32, 7, 2),
                           (20000, 128, 128, 1), (16, 4096, 1024, 0)]:
        x = torch.tensor(rng.normal(size=(M, K)), dtype=torch.float32, device=dev(), requires_grad=True)
        w = torch.tensor(rng.normal(size=(N, K)) / np.sqrt(K), dtype=torch.float32, device=dev(), requires_grad=True)
        b = torch.tensor(rng.normal(size=N), dtype=torch.float32, device=dev(), requires_grad=True)
        g = torch.tensor(rng.normal(size=(M, N)), dtype=torch.float32, device=dev())
        y = linear_train(x, w, b, act)
        (y * g).sum().backward()
        xd, wd, bd = (t.detach().double().requires_grad_(True) for t in (x, w, b))
        z = torch.nn.functional.linear(xd, wd, bd)
        yd = z if act == 0 else (torch.relu(z) if act == 1 else torch.nn.functional.leaky_relu(z, 0.01))
        (yd * g.double()).sum().backward()
        tol = lambda ref: 2e-5 * max(ref.abs().max().item(), 1e-6) * np.sqrt(max(M, K) / 64)
        assert (y.double() - yd).abs().max() <= tol(yd), (M, N, K)
        assert (x.grad.double() - xd.grad).abs().max() <= tol(xd.grad), (M, N, K, "dx")
        assert (w.grad.double() - wd.grad).abs().max() <= tol(wd.grad), (M, N, K, "dw")
        assert (b.grad.double() - bd.grad).abs().max() <= tol(bd.grad), (M, N, K, "db")
    # deterministic: fixed-order split reduction
    x = torch.randn(50000, 64, device=dev(), requires_grad=True)
    w = torch.randn(128, 64, device=dev(), requires_grad=True)
    outs = []
    for _ in range(2):
        w.grad = None
        linear_train(x, w, None, 1).square().sum().backward()
        outs.append(w.grad.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("pooled", [False, True, "sparse"])
def test_mlp_chain_is_the_per_layer_backward_without_the_activation_passes(pooled, monkeypatch):
    """``mlp_chain_train`` (one autograd node for a stack of dense layers; the activation's elementwise backward rides in
    the input-gradient GEMM's epilogue, mpx_linear_dact, or in the max-pool's backward, mpx_segment_max_grad_act) vs the
    per-layer nodes (``linear_train`` + ``_SegmentMax``): the same kernels' arithmetic per element -- gradients equal bit
    for bit at sizes where both take the 128 x 128 tile GEMM -- and vs torch autograd in float64.  The pooled stacks also
    run in ``bf16x3`` against their own fp32 run.
    Widths as in the set-abstraction modules (67 -> 128 -> 128 -> 256; a 7-wide output for the decoder's shape)."""
    from mpinets_amd import train_ops
    from mpinets_amd.train_ops import _SegmentMax, linear_train, mlp_chain_train

    # "sparse" (the default route): the pooled stack's last layer goes through mpx_pool_wgrad / mpx_pool_dgrad -- the same
    # sums in another order, so that case is held to the float64 reference only; True = the dense route (bit-equal)
    sparse = pooled == "sparse"
    pooled = bool(pooled)
    monkeypatch.setattr(train_ops, "SPARSE_POOL_BACKWARD", sparse)
    rng = np.random.default_rng(3)
    M = 3000
    widths, acts = ((67, 128, 128, 256), (1, 1, 1)) if pooled else ((132, 512, 64, 7), (2, 2, 0))
    mk = lambda *sh, s=1.0: torch.tensor(rng.normal(size=sh) * s, dtype=torch.float32, device=dev())
    x0 = mk(M, widths[0])
    ws = [mk(widths[i + 1], widths[i], s=1 / np.sqrt(widths[i])) for i in range(3)]
    bs = [mk(widths[i + 1]) for i in range(3)]
    offsets = None
    if pooled:
        seg = rng.integers(1, 40, size=400)
        seg = seg[np.cumsum(seg) <= M]  # segments of 1..39 rows, the last one takes the remainder
        seg[-1] += M - seg.sum()
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(seg)]), dtype=torch.int64, device=dev())
    n_out = (offsets.numel() - 1) if pooled else M
    g = mk(n_out, widths[-1])

    def run(kind, precision="fp32"):
        x = x0.clone().requires_grad_(True)
        w = [t.clone().requires_grad_(True) for t in ws]
        b = [t.clone().requires_grad_(True) for t in bs]
        if kind == "chain":
            y = mlp_chain_train(x, list(zip(w, b)), acts, offsets=offsets, precision=precision)
        else:
            h = x
            for i in range(3):
                h = linear_train(h, w[i], b[i], acts[i])
            y = _SegmentMax.apply(h, offsets, n_out) if pooled else h
        (y * g).sum().backward()
        return y.detach(), [x.grad] + [t.grad for t in w] + [t.grad for t in b]

    y_c, g_c = run("chain")
    y_l, g_l = run("layers")
    assert torch.equal(y_c, y_l)
    for a, b_ in zip(g_c, g_l):
        if sparse:
            assert (a - b_).abs().max() <= 2e-5 * max(b_.abs().max().item(), 1e-6) * np.sqrt(M / 64)
        else:
            assert torch.equal(a, b_)
    if pooled:
        # the same stack in ``bf16x3`` (every layer here is large enough for the split-bf16 entries: segmax, dact, wgrad) vs
        # its own fp32 run, at the bar of test_split_bf16_chain_follows_the_fp32_chain
        y_x, g_x = run("chain", "bf16x3")
        assert (y_x - y_c).abs().max() <= 1e-5 * y_c.abs().max()
        assert max(_rel_l2(a, r) for a, r in zip(g_x, g_c)) <= 2e-3 and not torch.equal(g_x[1], g_c[1])
    # float64 reference
    xd = x0.double().requires_grad_(True)
    wd = [t.double().requires_grad_(True) for t in ws]
    bd = [t.double().requires_grad_(True) for t in bs]
    h = xd
    for i in range(3):
        z = torch.nn.functional.linear(h, wd[i], bd[i])
        h = z if acts[i] == 0 else (torch.relu(z) if acts[i] == 1 else torch.nn.functional.leaky_relu(z, 0.01))
    if pooled:
        h = torch.stack([h[offsets[q]:offsets[q + 1]].max(dim=0).values for q in range(n_out)])
    (h * g.double()).sum().backward()
    for got, ref in zip(g_c, [xd.grad] + [t.grad for t in wd] + [t.grad for t in bd]):
        assert (got.double() - ref).abs().max() <= 3e-5 * max(ref.abs().max().item(), 1e-6) * np.sqrt(M / 64)
    # a stack whose input needs no gradient (the first module: its rows are data) returns none for it
    xn = x0.clone()
    w = [t.clone().requires_grad_(True) for t in ws]
    mlp_chain_train(xn, [(w[i], None) for i in range(3)], acts, offsets=offsets).sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in w)


@pytest.mark.parametrize("C,N,npoint,nsample", [(1, 300, 40, 128), (64, 200, 24, 128), (5, 90, 17, 32)])
def test_pack_rows_and_its_scatter_backward_match_torch_indexing(C, N, npoint, nsample):
    """mpx_pack_rows_ld / mpx_pack_rows_grad_ld (QueryAndGroup over the distinct neighbours, rows at a 16-byte pitch) vs plain
    torch indexing and its autograd: queries with 0 hits (one row: slot 0), with more than 64 rows (two id windows of the
    kernel), feature widths of 1 (the first module), 64 (the second, 68-float rows: not a multiple of the wave) and 5."""
    from mpinets_amd.train_ops import _PackRows, segment_offsets

    B = 3
    rng = np.random.default_rng(C * 100 + N)
    T = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=dev())
    xyz, new_xyz = T(rng.normal(size=(B, N, 3))), T(rng.normal(size=(B, npoint, 3)))
    feat = T(rng.normal(size=(B, N, C))).requires_grad_(True)
    cnt = rng.integers(0, nsample + 1, size=(B, npoint)).astype(np.int32)
    cnt[0, 0], cnt[0, 1], cnt[1, 2] = 0, nsample, 1
    idx = rng.integers(0, N, size=(B, npoint, nsample)).astype(np.int32)
    cnt_d, idx_d = T(cnt, torch.int32), T(idx, torch.int32)
    off = segment_offsets(cnt_d)
    R = int(off[-1])
    rows = _PackRows.apply(feat, xyz, 3, new_xyz, 3, C, C, idx_d, cnt_d, off, R, (B, N, npoint, nsample))
    ld = (3 + C + 3) // 4 * 4
    assert rows.shape == (R, ld)
    # reference: per query its first max(cnt, 1) slots
    fr = feat.detach().clone().requires_grad_(True)
    parts = []
    for b in range(B):
        for j in range(npoint):
            k = torch.as_tensor(idx[b, j, :max(int(cnt[b, j]), 1)].astype(np.int64), device=dev())
            parts.append(torch.cat((xyz[b, k] - new_xyz[b, j], fr[b, k], torch.zeros(k.numel(), ld - 3 - C, device=dev())), dim=1))
    ref = torch.cat(parts)
    assert torch.equal(rows.detach(), ref.detach())
    g = T(rng.normal(size=(R, ld)))
    (rows * g).sum().backward()
    (ref * g).sum().backward()
    assert (feat.grad - fr.grad).abs().max() <= 1e-5 * max(fr.grad.abs().max().item(), 1.0)  # (atomic adds: order free)


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("M,N,K,act", [(3000, 256, 128, 1), (1000, 64, 64, 1), (515, 200, 68, 2), (700, 130, 20, 0)])
def test_fused_pool_forward_is_the_two_step_form_bit_for_bit(M, N, K, act, x3):
    """mpx_linear_segmax (_bf16x3): the GEMM's epilogue max-pools each query's rows through 64-bit {value, ~row} keys; pooled
    values AND arg-max rows equal mpx_linear (_bf16x3) + mpx_segment_max exactly -- negative values (no activation /
    LeakyReLU), ties (duplicated rows: the first one wins), row and column counts that are not multiples of the tile."""
    from mpinets_amd import _lib
    from mpinets_amd.pointnet2 import split_pairs

    if x3 and K % 16:
        K = (K + 15) // 16 * 16
    rng = np.random.default_rng(M + N)
    lens = []
    while sum(lens) < M:
        lens.append(int(rng.integers(1, 90)))
    lens[-1] -= sum(lens) - M
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Q = len(lens)
    x = rng.normal(size=(M, K)).astype(np.float32)
    x[5] = x[4]  # a tie inside the first segment(s)
    w = (rng.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.normal(size=N).astype(np.float32)
    T = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=dev())
    xd, wd, bd, od = T(x), T(w), T(b), T(off, torch.int64)
    seg = torch.repeat_interleave(torch.arange(Q, dtype=torch.int32, device=dev()), od[1:] - od[:-1])
    y = torch.empty((M, N), device=dev())
    if x3:
        wp = split_pairs(wd)
        _lib.call("mpx_linear_bf16x3", _lib.ptr(xd), K, _lib.ptr(wp), _lib.ptr(bd), M, N, K, act, _lib.ptr(y), N)
    else:
        _lib.call("mpx_linear", _lib.ptr(xd), K, _lib.ptr(wd), _lib.ptr(bd), M, N, K, act, _lib.ptr(y), N)
    p0, a0 = torch.empty((Q, N), device=dev()), torch.empty((Q, N), dtype=torch.int64, device=dev())
    _lib.call("mpx_segment_max", _lib.ptr(y), N, _lib.ptr(od), Q, _lib.ptr(p0), N, _lib.ptr(a0))
    p1, a1 = torch.full((Q, N), float("nan"), device=dev()), torch.full((Q, N), -1, dtype=torch.int64, device=dev())
    keys = torch.empty((Q, N), dtype=torch.int64, device=dev())
    if x3:
        _lib.call("mpx_linear_segmax_bf16x3", _lib.ptr(xd), K, _lib.ptr(wp), _lib.ptr(bd), M, N, K, act, _lib.ptr(seg), Q,
                  _lib.ptr(keys), _lib.ptr(p1), N, _lib.ptr(a1))
    else:
        _lib.call("mpx_linear_segmax", _lib.ptr(xd), K, _lib.ptr(wd), _lib.ptr(bd), M, N, K, act, _lib.ptr(seg), Q,
                  _lib.ptr(keys), _lib.ptr(p1), N, _lib.ptr(a1))
    assert torch.equal(p0, p1)
    assert torch.equal(a0, a1)


@pytest.mark.parametrize("Q,C,K,act,below,win", [(37, 256, 128, 1, 1, 128), (64, 64, 64, 1, 1, 16), (5, 1024, 512, 1, 1, 128),
                                                  (50, 96, 68, 2, 2, 32), (33, 70, 20, 0, 0, 128), (9, 130, 132, 1, 0, 16)])
def test_sparse_pool_backward_kernels_match_float64(Q, C, K, act, below, win):
    """mpx_pool_wgrad / mpx_pool_dgrad (the backward of [dense layer + activation + segment max-pool] over the pool's
    Q * C non-zero gradients) vs the dense definition in float64: segments of 1..200 rows and one of 600 (more than the
    input-gradient kernel's 256-row window: several passes), channel / column counts that are not multiples of 64, every activation code, dead channels
    (pooled value <= 0 under ReLU), several channels sharing one arg-max row, rows that receive no gradient at all."""
    from mpinets_amd import _lib

    rng = np.random.default_rng(Q * 1000 + C)
    lens = rng.integers(1, 200 if Q < 40 else 30, size=Q)
    lens[1] = 600  # more rows than one window of the input-gradient kernel (256)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    R = int(off[-1])
    T = lambda a, dt=torch.float32: torch.tensor(a, dtype=dt, device=dev())
    x = rng.normal(size=(R, K)).astype(np.float32)
    w = (rng.normal(size=(C, K)) / np.sqrt(K)).astype(np.float32)
    pooled = rng.normal(size=(Q, C)).astype(np.float32)  # the activation's output at the arg-max (sign decides act')
    g = rng.normal(size=(Q, C)).astype(np.float32)
    arg = np.stack([off[q] + rng.integers(0, lens[q], size=C) for q in range(Q)]).astype(np.int64)
    arg[0, : C // 2] = off[0]  # half of the first query's channels share one row
    d = lambda o, a: np.ones_like(o) if a == 0 else ((o > 0).astype(np.float64) if a == 1 else np.where(o >= 0, 1.0, 0.01))
    gz = g.astype(np.float64) * d(pooled.astype(np.float64), act)
    dz = np.zeros((R, C))
    for q in range(Q):
        dz[arg[q], np.arange(C)] += gz[q]
    dw_ref, db_ref = dz.T @ x.astype(np.float64), dz.sum(0)
    gx_ref = (dz @ w.astype(np.float64)) * d(x.astype(np.float64), below)

    lib = _lib.load()
    xd, wd, pd, gd, ad, od = T(x), T(w), T(pooled), T(g), T(arg, torch.int64), T(off, torch.int64)
    both = torch.full((C * K + C,), float("nan"), device=dev())
    scratch = torch.empty(lib.mpx_pool_wgrad_scratch(Q, C, K), dtype=torch.float32, device=dev())
    _lib.call("mpx_pool_wgrad", _lib.ptr(gd), C, _lib.ptr(ad), _lib.ptr(pd), C, Q, C, act, _lib.ptr(xd), K, K, _lib.ptr(both),
              _lib.ptr(both[C * K:]), _lib.ptr(scratch))
    gx = torch.full((R, K), float("nan"), device=dev())
    _lib.call("mpx_pool_dgrad", _lib.ptr(gd), C, _lib.ptr(ad), _lib.ptr(pd), C, _lib.ptr(od), Q, C, act, _lib.ptr(wd), K,
              _lib.ptr(xd) if below else None, K, below, K, win, _lib.ptr(gx), K)
    torch.cuda.synchronize()
    tol = lambda ref: 2e-6 * max(np.abs(ref).max(), 1e-6) * np.sqrt(max(Q, 64) / 64)
    dw, db = both[:C * K].view(C, K).cpu().numpy().astype(np.float64), both[C * K:].cpu().numpy().astype(np.float64)
    assert np.abs(dw - dw_ref).max() <= tol(dw_ref) and np.abs(db - db_ref).max() <= tol(db_ref)
    assert np.abs(gx.cpu().numpy().astype(np.float64) - gx_ref).max() <= tol(gx_ref)
    # a second run gives the same bits (fixed summation order)
    both2, gx2 = torch.empty_like(both), torch.empty_like(gx)
    _lib.call("mpx_pool_wgrad", _lib.ptr(gd), C, _lib.ptr(ad), _lib.ptr(pd), C, Q, C, act, _lib.ptr(xd), K, K, _lib.ptr(both2),
              _lib.ptr(both2[C * K:]), _lib.ptr(scratch))
    _lib.call("mpx_pool_dgrad", _lib.ptr(gd), C, _lib.ptr(ad), _lib.ptr(pd), C, _lib.ptr(od), Q, C, act, _lib.ptr(wd), K,
              _lib.ptr(xd) if below else None, K, below, K, win, _lib.ptr(gx2), K)
    assert torch.equal(both, both2) and torch.equal(gx, gx2)


def test_split_bf16_training_gemms_match_float64():
    """Row N1, the `bf16x3` training arithmetic (the engine's form of the reference's precision=16,
    run_training.py:112).  Kernel by kernel against float64 with the discrete choices GIVEN (the mask of the activation
    below, dense and 2 %-dense gradients as the max-pool's backward produces them): the input-gradient GEMM with the
    activation backward in its epilogue (mpx_linear_bf16x3_dact) and the weight / bias gradient (mpx_linear_wgrad_bf16x3)
    stay within 3e-5 of the largest entry (fp32 kernels: 2e-7)."""
    from mpinets_amd import _lib
    from mpinets_amd.pointnet2 import split_pairs

    torch.manual_seed(0)
    M, N, K = 5000, 128, 256
    for density in (1.0, 0.02):
        keep = lambda *sh: (torch.rand(*sh, device=dev()) < density).float()
        x = torch.randn(M, K, device=dev()) * keep(M, K)
        w = torch.randn(N, K, device=dev()) / 16
        below = torch.randn(M, N, device=dev())  # the output rows of the layer below: sign -> mask
        wp = split_pairs(w)
        rel = lambda got, ref: ((got.double() - ref).abs().max() / ref.abs().max()).item()
        for act, mask in ((1, (below > 0).double()), (2, torch.where(below >= 0, 1.0, 0.01).double())):
            y = torch.empty(M, N, device=dev())
            _lib.call("mpx_linear_bf16x3_dact", _lib.ptr(x), K, _lib.ptr(wp), M, N, K, _lib.ptr(below), N, act, _lib.ptr(y), N)
            assert rel(y, (x.double() @ w.double().t()) * mask) <= 3e-5
            y32 = torch.empty(M, N, device=dev())
            _lib.call("mpx_linear_dact", _lib.ptr(x), K, _lib.ptr(w), M, N, K, _lib.ptr(below), N, act, _lib.ptr(y32), N)
            assert rel(y32, (x.double() @ w.double().t()) * mask) <= 1e-6
        dz = torch.randn(M, N, device=dev()) * keep(M, N)
        both = torch.empty(N * K + N, device=dev())
        scratch = torch.empty(_lib.load().mpx_linear_wgrad_scratch(M, N, K), device=dev())
        rw, rb = dz.double().t() @ x.double(), dz.double().sum(0)
        for fn, tol in (("mpx_linear_wgrad", 1e-6), ("mpx_linear_wgrad_bf16x3", 3e-5)):
            both.zero_()
            _lib.call(fn, _lib.ptr(dz), N, _lib.ptr(x), K, M, N, K, _lib.ptr(both), _lib.ptr(both[N * K:]), _lib.ptr(scratch))
            assert rel(both[:N * K].view(N, K), rw) <= tol and rel(both[N * K:], rb) <= tol, (fn, density)


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30)).item()


def test_split_bf16_chain_follows_the_fp32_chain():
    """A set-abstraction-shaped stack (67 -> 128 -> 128 -> 256, max-pooled per segment) forward + backward in ``bf16x3`` vs
    the same stack in fp32: outputs within 1e-5 of the largest; every gradient tensor within 2e-3 in relative L2 -- a few
    arg-max rows / ReLU signs of values within 1e-5 of a tie may flip between the two arithmetics, which moves single
    elements, so the bound is on the norm (the kernels themselves are pinned to float64 in the test above)."""
    from mpinets_amd.train_ops import mlp_chain_train

    rng = np.random.default_rng(5)
    M = 5000
    widths, acts = (67, 128, 128, 256), (1, 1, 1)
    mk = lambda *sh, s=1.0: torch.tensor(rng.normal(size=sh) * s, dtype=torch.float32, device=dev())
    x0 = mk(M, widths[0])
    ws = [mk(widths[i + 1], widths[i], s=1 / np.sqrt(widths[i])) for i in range(3)]
    bs = [mk(widths[i + 1], s=0.3) for i in range(3)]
    seg = rng.integers(1, 60, size=400)
    seg = seg[np.cumsum(seg) <= M]
    seg[-1] += M - seg.sum()
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(seg)]), dtype=torch.int64, device=dev())
    g = mk(offsets.numel() - 1, widths[-1])
    res = {}
    for prec in ("fp32", "bf16x3"):
        x = x0.clone().requires_grad_(True)
        w = [t.clone().requires_grad_(True) for t in ws]
        b = [t.clone().requires_grad_(True) for t in bs]
        y = mlp_chain_train(x, list(zip(w, b)), acts, offsets=offsets, precision=prec)
        (y * g).sum().backward()
        res[prec] = (y.detach(), [x.grad] + [t.grad for t in w] + [t.grad for t in b])
    (y32, g32), (y16, g16) = res["fp32"], res["bf16x3"]
    assert (y16 - y32).abs().max() <= 1e-5 * y32.abs().max()
    errs = [_rel_l2(a, r) for a, r in zip(g16, g32)]
    print("bf16x3 vs fp32 stack, relative L2 of dx, dW1..3, db1..3:", " ".join("%.1e" % e for e in errs))
    assert max(errs) <= 2e-3 and not torch.equal(g16[1], g32[1])


def test_training_step_in_split_bf16_matches_the_fp32_step():
    """One whole training_step + backward with ``set_training_precision("bf16x3")`` vs the fp32 step (whose gradients the
    reference-run golden pins, tests/test_gpu_model_golden.py): loss within 1e-4 relative; gradients of the heads (fc
    layer, joint encoder, decoder: no discrete choice upstream of them changes) within 1e-3 in relative L2; gradients of
    the set-abstraction weights within 3e-2 -- the max-pool routes a gradient element to ONE row, and about 0.05 % of
    the arg-max rows (values within 1e-5 of a tie) differ between the two forwards; the GEMMs themselves are pinned to
    float64 at 3e-5 above.  (fp16 mixed precision, the reference's precision=16, flips ~30x more.)"""
    from mpinets_amd.model import TrainingMotionPolicyNetwork
    from mpinets_amd.scenes import make_problem_batch

    B = 12
    prob = make_problem_batch(B, seed=31, device=dev(), kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16, device_clouds=True)
    keys = ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii", "cylinder_heights", "cylinder_quats")
    g = torch.Generator(device="cpu").manual_seed(1)
    sup = torch.clamp(prob["q_norm"] + 0.05 * torch.randn(B, 7, generator=g).to(dev()), -1, 1)
    batch = {"xyz": prob["xyz"], "configuration": prob["q_norm"], "supervision": sup, **{k: prob[k] for k in keys}}
    out = {}
    for prec in ("fp32", "bf16x3"):
        torch.manual_seed(0)
        np.random.seed(0)  # (the loss samples the robot cloud through robofin-style np.random subsets: same draws for both)
        tm = TrainingMotionPolicyNetwork(2048, 1.0, 5.0).to(dev()).train().set_training_precision(prec)
        loss = tm.training_step({k: v.clone() for k, v in batch.items()}, 0)
        loss.backward()
        out[prec] = (loss.item(), {n: p.grad.clone() for n, p in tm.named_parameters() if p.grad is not None})
    l32, g32 = out["fp32"]
    l16, g16 = out["bf16x3"]
    assert abs(l16 - l32) <= 1e-4 * abs(l32), (l16, l32)
    assert g32.keys() == g16.keys() and len(g32) > 30
    errs = sorted(((_rel_l2(g16[n], g32[n]), n) for n in g32), reverse=True)
    print("largest per-tensor relative L2 differences:", ", ".join("%s %.1e" % (n, e) for e, n in errs[:6]))
    worst = errs[0][0]
    heads = max(e for e, n in errs if "SA_modules" not in n)
    print("bf16x3 training step: loss %.6f (fp32 %.6f), largest relative L2 gradient difference %.1e (heads %.1e)" % (l16, l32, worst, heads))
    assert worst <= 3e-2 and heads <= 1e-3


def test_groupnorm_leaky_backward_matches_torch():
    from mpinets_amd.train_ops import groupnorm_leaky_train

    torch.manual_seed(3)
    for (M, C) in [(7, 4096), (256, 2048), (3, 64)]:
        gn = torch.nn.GroupNorm(16, C).to(dev())
        with torch.no_grad():
            gn.weight.normal_(1.0, 0.3), gn.bias.normal_(0.0, 0.3)
        x = (torch.randn(M, C, device=dev()) * 2 + 0.5).requires_grad_(True)
        g = torch.randn(M, C, device=dev())
        (groupnorm_leaky_train(x, gn) * g).sum().backward()
        got = (x.grad.clone(), gn.weight.grad.clone(), gn.bias.grad.clone())
        x.grad = None
        gn.zero_grad()
        # reference on the CPU in float64 (torch's own GPU GroupNorm backward returns wrong weight / bias gradients
        # at batch 256 on this ROCm build -- tools/probes/gn_dbg.py -- one more reason the layer has its own kernel)
        xd = x.detach().double().cpu().requires_grad_(True)
        gd = torch.nn.GroupNorm(16, C).double()
        gd.load_state_dict({k: v.double().cpu() for k, v in gn.state_dict().items()})
        (torch.nn.functional.leaky_relu(gd(xd), 0.01) * g.double().cpu()).sum().backward()
        for a, b in zip(got, (xd.grad, gd.weight.grad, gd.bias.grad)):
            assert (a.double().cpu() - b).abs().max() <= 2e-5 * max(b.abs().max().item(), 1.0), (M, C)


@pytest.mark.parametrize("left_in_eval", ["point_cloud_encoder", "point_cloud_encoder.SA_modules.1"])
def test_train_step_trains_a_submodule_left_in_eval(left_in_eval):
    """``train_step`` with the point-cloud encoder (or one set-abstraction module) in ``eval()``: the modules that pick
    their path by their own ``training`` flag are put back in training mode, so every parameter gets a gradient, the same
    as a fully-train step's -- bit for bit except SA1's, which sit behind the float-atomic scatter into f1 (any
    summation order) and are held to 1e-5 of their largest element."""
    from mpinets_amd.model import TrainingMotionPolicyNetwork
    from mpinets_amd.training import train_step

    batch = small_batch(4, 7)
    grads = {}
    for mode in ("train", left_in_eval):
        torch.manual_seed(0)
        np.random.seed(0)
        tm = TrainingMotionPolicyNetwork(2048, 1.0, 5.0).to(dev()).train()
        if mode != "train":
            tm.get_submodule(mode).eval()
        opt = torch.optim.SGD(tm.parameters(), lr=0.0)
        train_step(tm, opt, {k: v.clone() for k, v in batch.items()}, gradient_clip_val=None)
        assert all(m.training for m in tm.modules())
        grads[mode] = {n: None if p.grad is None else p.grad.clone() for n, p in tm.named_parameters()}
    ref, got = grads["train"], grads[left_in_eval]
    missing = [n for n, g in got.items() if g is None]
    assert not missing, f"no gradient after train_step with {left_in_eval} in eval(): {missing}"
    for n, g in got.items():
        if ".SA_modules.0." in n:
            assert (g - ref[n]).abs().max() <= 1e-5 * ref[n].abs().max(), n
        else:
            assert torch.equal(g, ref[n]), n
