"""Restatement of csrc/ik.hip (``mpx_franka_ik``) on the CPU, in float64 by default.

Same starts (Philox4x32-10 keyed by (seed, global problem id, start), the uniform mapped into the limits in float32 like
the device does, so both sides iterate from the SAME numbers), same iteration (FK, error ``[p_t - p ; rotvec(R_t R^T)]``,
geometric Jacobian, ``dq = J^T (J J^T + lambda^2 I)^-1 e``, step clip, clamp), same acceptance (one more FK of the final
q), same "lowest start that converged and is free" rule.  Built on ``oracle.fk_frames_torch`` (FK in the dtype of q) and
``oracle.collision_flags`` (the sphere-vs-primitive test); the self-collision model is the four-sphere one of
``mpx_trajectory_metrics``.  ``dtype=torch.float32`` runs the same statements in float32: the reference-against-reference
measurement that sets the bar of the one-step test.
"""
import numpy as np
import torch

from mpinets_amd import franka_tables as ft
from oracle import oracle as orc

SEEDS = 64
STREAM_IK = 13
DEFAULTS = dict(iterations=64, damping=0.05, step_clip=0.5, pos_tol=1e-3, rot_tol=float(np.radians(0.5)), clearance=0.0)
ACCEPT_SHARE, ACCEPT_ANGLE_MARGIN = 0.9999, 2e-6  # MPX_IK_ACCEPT_* of include/mpinets_hip.h
BIT_CONVERGED, BIT_ENV_HIT, BIT_SELF_HIT = 1, 2, 4


def philox4x32_np(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (uint32 arrays / scalars, broadcast) -> four uint32 arrays; checked against
    ``oracle.philox4x32`` in tests/test_ik_host.py."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    M32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n1 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32
        n2, n3 = (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def limits32(limits):
    """The float32 limits the device clamps to: the cast of ``limits``, moved one float32 toward the inside of the interval
    wherever the cast landed outside it (so a joint on a limit satisfies the float64 limits as given)."""
    lim = np.asarray(limits, dtype=np.float64)
    out = lim.astype(np.float32)
    for j in range(lim.shape[0]):
        if float(out[j, 0]) < lim[j, 0]:
            out[j, 0] = np.nextafter(out[j, 0], np.float32(np.inf))
        if float(out[j, 1]) > lim[j, 1]:
            out[j, 1] = np.nextafter(out[j, 1], np.float32(-np.inf))
    return out


def starts(B, limits, q_init=None, seed=0, env_offset=0):
    """-> float32 [B,64,7]: the device's starting configurations, bit for bit."""
    lim = limits32(limits)
    lo, hi = lim[:, 0], lim[:, 1]
    lane = np.arange(SEEDS, dtype=np.uint64)[None, :]
    gid = ((env_offset + np.arange(B, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))[:, None]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    r0 = philox4x32_np(2 * lane, gid, STREAM_IK, 0, k0, k1)
    r1 = philox4x32_np(2 * lane + 1, gid, STREAM_IK, 0, k0, k1)
    bits = np.stack(list(r0) + list(r1[:3]), axis=-1)  # [B,64,7]
    u = (bits >> np.uint32(8)).astype(np.float32) * np.float32(5.9604644775390625e-08)
    q = lo + u * (hi - lo)  # float32 multiply, then float32 add
    first = np.asarray(ft.DEFAULT_Q, dtype=np.float32)[None].repeat(B, 0) if q_init is None \
        else np.asarray(q_init, dtype=np.float32).reshape(B, 7)
    q[:, 0] = first
    return np.minimum(np.maximum(q, lo), hi).astype(np.float32)


def rotvec(Rt, R):
    """rotation vector of R_t R^T and its angle, by the kernel's formula (antisymmetric part, atan2)."""
    E = Rt @ R.transpose(-1, -2)
    w = 0.5 * torch.stack([E[..., 2, 1] - E[..., 1, 2], E[..., 0, 2] - E[..., 2, 0], E[..., 1, 0] - E[..., 0, 1]], -1)
    c = 0.5 * (E[..., 0, 0] + E[..., 1, 1] + E[..., 2, 2] - 1.0)
    s = torch.linalg.norm(w, dim=-1)
    theta = torch.atan2(s, c)
    k = torch.where(s > 1e-7, theta / torch.clamp(s, min=1e-30), torch.ones_like(s))
    return w * k[..., None], theta


def pose_error(q, Rt, pt, finger=ft.FINGER_OPENING):
    """-> position error [N], rotation angle [N] of right_gripper(q) against the target."""
    R, t = orc.fk_frames_torch(q, finger)
    _, theta = rotvec(Rt, R[:, 14])
    return torch.linalg.norm(pt - t[:, 14], dim=-1), theta


def jacobian(q, finger=ft.FINGER_OPENING):
    """-> J [N,6,7] (geometric, world frame, right_gripper), p [N,3], R [N,3,3]."""
    R, t = orc.fk_frames_torch(q, finger)
    o, z = t[:, 1:8], R[:, 1:8, :, 2]
    p = t[:, 14]
    J = torch.cat([torch.cross(z, p[:, None] - o, dim=-1), z], dim=-1).transpose(1, 2)
    return J, p, R[:, 14]


def step(q, Rt, pt, lo, hi, damping=0.05, step_clip=0.5, finger=ft.FINGER_OPENING):
    """One damped-least-squares iteration in q's dtype."""
    J, p, R = jacobian(q, finger)
    w, _ = rotvec(Rt, R)
    e = torch.cat([pt - p, w], dim=-1)
    A = J @ J.transpose(1, 2) + (damping * damping) * torch.eye(6, dtype=q.dtype)
    y = torch.cholesky_solve(e[..., None], torch.linalg.cholesky(A))
    dq = (J.transpose(1, 2) @ y)[..., 0]
    big = dq.abs().amax(dim=-1, keepdim=True)
    dq = dq * torch.where(big > step_clip, step_clip / torch.clamp(big, min=1e-30), torch.ones_like(big))
    return torch.minimum(torch.maximum(q + dq, lo), hi)


def self_hits(t):
    """t [N,15,3] frame origins -> bool [N]: the body-cylinder test of trajectory_metrics_kernel."""
    hit = torch.zeros(t.shape[0], dtype=torch.bool)
    for link, radius in ((7, 0.1), (9, 0.01), (12, 0.01), (13, 0.01)):
        c = t[:, link]
        dz = c[:, 2] - torch.clamp(c[:, 2], -0.3, 0.333)
        hit |= torch.sqrt(c[:, 0] ** 2 + c[:, 1] ** 2 + dz ** 2) < 0.15 + radius
    return hit


def env_hits(q, scene, clearance=0.0, with_base_link=False, finger=ft.FINGER_OPENING):
    """q [B,K,7] -> bool [B,K]: any collision sphere within radius + clearance of scene b's primitives."""
    B, K = q.shape[:2]
    R, t = orc.fk_frames_torch(q.reshape(-1, 7), finger)
    c, r, l, _ = ft.collision_sphere_table(with_base_link)
    link = torch.from_numpy(l).long()
    centres = torch.einsum("nsij,sj->nsi", R[:, link], torch.from_numpy(c).to(q.dtype)) + t[:, link]
    centres = centres.reshape(B, K, len(r), 3).numpy().astype(np.float32)
    _, msdf = orc.collision_flags(centres, r, tuple(scene[k] for k in ("cuboid_centers", "cuboid_dims", "cuboid_quats")),
                                  tuple(scene[k] for k in ("cylinder_centers", "cylinder_radii", "cylinder_heights",
                                                           "cylinder_quats")))
    return torch.from_numpy((msdf <= (r + np.float32(clearance))[None, None]).any(-1))


def solve(target_poses, limits=ft.JOINT_LIMITS_REAL, q_init=None, scene=None, seed=0, env_offset=0, check_self=None,
          dtype=torch.float64, with_base_link=False, chunk=512, **options):
    """-> q [B,7], status [B], all_q [B,64,7], all_status [B,64] (numpy; q in ``dtype``), like ``robot.franka_ik`` with
    ``return_all``: every converged start is tested, the lowest free one is the result."""
    opt = dict(DEFAULTS, **options)
    check_self = (scene is not None) if check_self is None else check_self
    tp = np.asarray(target_poses, dtype=np.float32)
    B = tp.shape[0]
    lim = torch.from_numpy(limits32(limits)).to(dtype)
    lo, hi = lim[:, 0], lim[:, 1]
    q0 = starts(B, limits, q_init, seed, env_offset)
    all_q = np.empty((B, SEEDS, 7), dtype=np.float64 if dtype == torch.float64 else np.float32)
    all_status = np.zeros((B, SEEDS), dtype=np.int32)
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        n = sl.stop - sl.start
        T = torch.from_numpy(tp[sl]).to(dtype)
        Rt = T[:, None, :3, :3].expand(n, SEEDS, 3, 3).reshape(-1, 3, 3)
        pt = T[:, None, :3, 3].expand(n, SEEDS, 3).reshape(-1, 3)
        q = torch.from_numpy(q0[sl]).to(dtype).reshape(-1, 7)
        for _ in range(opt["iterations"]):
            q = step(q, Rt, pt, lo, hi, opt["damping"], opt["step_clip"])
        perr, theta = pose_error(q, Rt, pt)
        conv = ((perr <= opt["pos_tol"] * ACCEPT_SHARE) &
                (theta <= opt["rot_tol"] * ACCEPT_SHARE - ACCEPT_ANGLE_MARGIN)).reshape(n, SEEDS)
        qk = q.reshape(n, SEEDS, 7)
        bits = conv.to(torch.int32) * BIT_CONVERGED
        if scene is not None:
            env = env_hits(qk, {k: v[sl] for k, v in scene.items()}, opt["clearance"], with_base_link)
            bits |= (env & conv).to(torch.int32) * BIT_ENV_HIT
        if check_self:
            _, t = orc.fk_frames_torch(q)
            bits |= (self_hits(t).reshape(n, SEEDS) & conv).to(torch.int32) * BIT_SELF_HIT
        all_q[sl], all_status[sl] = qk.numpy(), bits.numpy()
    return (*pick(all_q, all_status), all_q, all_status)


def pick(all_q, all_status):
    """The first-free-start rule: -> q [B,7] (NaN rows where status != 0), status [B]."""
    free = all_status == BIT_CONVERGED
    conv = (all_status & BIT_CONVERGED) != 0
    B = all_q.shape[0]
    winner = np.where(free.any(1), free.argmax(1), -1)
    status = np.where(winner >= 0, 0, np.where(conv.any(1), 1, 2)).astype(np.int32)
    q = np.full((B, 7), np.nan, dtype=all_q.dtype)
    ok = winner >= 0
    q[ok] = all_q[np.nonzero(ok)[0], winner[ok]]
    return q, status
