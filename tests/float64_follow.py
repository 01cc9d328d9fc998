"""Restatement of ``mpx_franka_follow`` on the CPU, in float64 by default, written from the contract in
include/mpinets_hip.h (not from csrc/follow.hip): one step of the follower (FK, switch, stop, attractor, obstacle term,
acceleration, position-first integration with the clamp), the dense path and its arc lengths, the retiming to T waypoints
and the verdict.  The follower is a STAND-IN for the reference's Geometric Fabrics expert, not Lula: this file restates the
stand-in, nothing of the fabric.

Built on ``float64_ik.jacobian / rotvec`` (the attractor), ``float64_plan.obstacle_gradient(want_fragile=True)`` (the
obstacle term) and ``float64_plan.validity`` (bits 0-2).  Every option is rounded to float32 first, the limits are the
device's ``limits32``, the inputs are float32: both sides start from the same numbers.  ``dtype=torch.float32`` runs the same
statements in float32: the reference-against-reference measurement that sets the bars of the GPU tests.

A step is FRAGILE when a comparison that decides its branch is within rounding of deciding the other way: a switch or
stop distance within ``FRAGILE_DIST`` of its radius (where the step count does not decide anyway), a joint whose unclamped
position is within ``FRAGILE_CLAMP`` of a limit without sitting on it exactly (a joint that rests on a limit with v = 0 lands
on it bit for bit in any arithmetic), or the obstacle gradient's own flag (``float64_plan.obstacle_gradient``).

``problems`` builds the inputs the host and the GPU tests share (construction and seeds recorded there).
"""
import numpy as np
import torch

import float64_ik as fik
import float64_plan as fp
from mpinets_amd import franka_tables as ft
from oracle import oracle as orc

# MPX_FOLLOW_DEFAULT_* of include/mpinets_hip.h (``lambda_``: the C struct's ``lambda``)
DEFAULTS = dict(dt=0.005, max_steps=1024, attract=144.0, damping=24.0, lambda_=0.05, step_clip=0.5, repel=40.0, epsilon=0.05,
                clearance=0.0, limit_gain=50.0, limit_band=0.1, speed_limit=1.6999, switch_radius=0.15, switch_steps=100,
                final_radius=0.005, final_steps=800, substeps=4, check_margin=1e-4, max_jerk=0.15, check_self=True,
                miss_tol=0.05)
_INT_OPTIONS = ("max_steps", "switch_steps", "final_steps", "substeps", "check_self")
MISS_SHARE = 0.9999  # MPX_FOLLOW_MISS_SHARE
BIT_MISS = 8
FRAGILE_DIST, FRAGILE_CLAMP = 1e-5, 1e-6  # [m], [rad]
RIGHT_GRIPPER = 14


def options(**given):
    """``given`` over ``DEFAULTS``, every float rounded to float32 (what the device's struct holds)."""
    unknown = set(given) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown option(s) {sorted(unknown)}")
    o = dict(DEFAULTS, **given)
    return {k: (int(v) if k in _INT_OPTIONS else float(np.float32(v))) for k, v in o.items()}


def _has_prims(scene):
    return scene is not None and scene["cub_dims"].shape[1] + scene["cyl_radii"].shape[1] > 0


def step(q, v, w, nw, fin, poses, scene, lo, hi, opt, want_fragile=False, with_base_link=False):
    """One step of every row from (q [B,7], v [B,7], w, nw int64 [B], fin bool [B]) in q's dtype; ``poses`` [B,W,4,4] in
    that dtype.  -> q', v', w', nw', fin' and a dict with ``took`` (bool [B]: the row took the step), ``repel_g`` (|repel g|
    max per row) and, with ``want_fragile``, ``fragile`` (bool [B]).  A finished row keeps its state."""
    B, W = poses.shape[:2]
    rows = torch.arange(B)
    J, p, R = fik.jacobian(q)

    def target(idx):
        return poses[rows, idx, :3, 3], poses[rows, idx, :3, :3]

    pw, Rw = target(w)
    dist = torch.linalg.norm(pw - p, dim=-1)
    last = w == W - 1
    by_count = nw >= opt["switch_steps"]
    switch = ~last & ((dist <= opt["switch_radius"]) | by_count)
    kinds = {"switch": ~last & ~by_count & ((dist - opt["switch_radius"]).abs() < FRAGILE_DIST)}
    w2, nw2 = torch.where(switch, w + 1, w), torch.where(switch, torch.zeros_like(nw), nw)
    pw, Rw = target(w2)
    dist = torch.linalg.norm(pw - p, dim=-1)
    end_count = nw2 >= opt["final_steps"]
    stop = last & ((dist < opt["final_radius"]) | end_count)
    kinds["stop"] = last & ~end_count & ((dist - opt["final_radius"]).abs() < FRAGILE_DIST)
    fin2 = fin | stop
    took = ~fin2

    rv, _ = fik.rotvec(Rw, R)
    e = torch.cat([pw - p, rv], dim=-1)
    A = J @ J.transpose(1, 2) + (opt["lambda_"] * opt["lambda_"]) * torch.eye(6, dtype=q.dtype)
    y = torch.cholesky_solve(e[..., None], torch.linalg.cholesky(A))
    u = (J.transpose(1, 2) @ y)[..., 0]
    big = u.abs().amax(dim=-1, keepdim=True)
    u = u * torch.where(big > opt["step_clip"], opt["step_clip"] / torch.clamp(big, min=1e-30), torch.ones_like(big))

    if _has_prims(scene):
        g, gf = fp.obstacle_gradient(q, scene, 1, opt["epsilon"], opt["clearance"], with_base_link, want_fragile=True)
        kinds["gradient"] = gf
    else:
        g = torch.zeros_like(q)
    barrier = torch.clamp((lo + opt["limit_band"]) - q, min=0) - torch.clamp(q - (hi - opt["limit_band"]), min=0)
    a = ((opt["attract"] * u - opt["repel"] * g) + opt["limit_gain"] * barrier) - opt["damping"] * v
    moved = q + opt["dt"] * v
    vn = torch.clamp(v + opt["dt"] * a, -opt["speed_limit"], opt["speed_limit"])
    qn = torch.minimum(torch.maximum(moved, lo), hi)
    vn = torch.where(qn != moved, torch.zeros_like(vn), vn)
    near = torch.minimum((moved - lo).abs(), (moved - hi).abs())
    kinds["clamp"] = ((near < FRAGILE_CLAMP) & (near > 0)).any(-1)

    keep = ~took
    out_q, out_v = torch.where(keep[:, None], q, qn), torch.where(keep[:, None], v, vn)
    # (a finished row keeps w and nw as they were on entry: the stop is tested before anything moves)
    out_w, out_nw = torch.where(keep, w, w2), torch.where(keep, nw, nw2 + 1)
    info = {"took": took, "repel_g": (opt["repel"] * g).abs().amax(-1)}
    if want_fragile:  # (a fragile stop decision counts for the step it ends; the others for a step that was taken)
        kinds = {k: f & (took | (stop & ~fin)) if k == "stop" else f & took for k, f in kinds.items()}
        info["fragile"] = torch.stack(list(kinds.values())).any(0)
        info["fragile_kinds"] = kinds
    return out_q, out_v, out_w, out_nw, fin2, info


def bad_input(q_start, poses, scene, limits, v_init, progress, opt, with_base_link=False):
    """-> bool [B]: the rows ``mpx_franka_follow`` answers with status 2."""
    qs = np.asarray(q_start, np.float32)
    B, W = poses.shape[:2]
    lim = fik.limits32(limits)
    bad = ~((qs >= lim[:, 0]) & (qs <= lim[:, 1])).all(-1)  # (NaN fails)
    bad |= ~np.isfinite(np.asarray(poses, np.float32)[:, :, :3]).reshape(B, -1).all(-1)
    if v_init is not None:
        bad |= ~np.isfinite(np.asarray(v_init, np.float32)).all(-1)
    if progress is not None:
        pg = np.asarray(progress)
        bad |= (pg[:, 0] < 0) | (pg[:, 0] >= W) | (pg[:, 1] < 0)
    if progress is not None:  # (a continued rollout is not refused for a state in collision)
        return bad
    cb = fp.config_bits(torch.from_numpy(np.nan_to_num(qs)).double(), scene if _has_prims(scene) else None, 1,
                        opt["clearance"] + opt["check_margin"], bool(opt["check_self"]), opt["check_margin"], with_base_link)
    return bad | (cb.numpy() != 0)


def rollout(q_start, poses, scene=None, limits=ft.JOINT_LIMITS_REAL, v_init=None, progress=None, dtype=torch.float64,
            with_base_link=False, record_states=False, **given):
    """The time loop.  -> dict: ``path`` [B,max_steps+1,7] and ``arc`` [B,max_steps+1] (numpy in ``dtype``; NaN beyond
    ``steps``), ``steps`` int32 [B], ``q_end``, ``v_end``, ``progress_end`` int32 [B,3], ``bad`` bool [B] (status 2: no steps),
    ``fragile`` bool [B,max_steps] (step i -> column i-1), ``fragile_kinds`` (kind -> bool [B]: a step of the row was fragile
    that way), ``repel_g`` [B] (the largest |repel g| of a step taken); with ``record_states`` also ``states``: v [B,n+1,7], w and nw
    [B,n+1] after every step of the loop (column i beside path[:, i]; n = the most steps a row took)."""
    opt = options(**given)
    qs32, ps32 = np.asarray(q_start, np.float32), np.asarray(poses, np.float32)
    B, W = ps32.shape[:2]
    n_max = opt["max_steps"]
    bad = torch.from_numpy(bad_input(qs32, ps32, scene, limits, v_init, progress, opt, with_base_link))
    lim = torch.from_numpy(fik.limits32(limits)).to(dtype)
    lo, hi = lim[:, 0], lim[:, 1]
    q = torch.from_numpy(np.nan_to_num(qs32)).to(dtype)
    q = torch.where(bad[:, None], torch.from_numpy(np.asarray(ft.DEFAULT_Q, np.float32)).to(dtype).expand(B, 7), q)  # (not stepped)
    P = torch.from_numpy(np.nan_to_num(ps32)).to(dtype)
    v = torch.zeros(B, 7, dtype=dtype) if v_init is None else torch.from_numpy(np.nan_to_num(np.asarray(v_init, np.float32))).to(dtype)
    pg = np.zeros((B, 3), np.int64) if progress is None else np.asarray(progress).astype(np.int64)
    w = torch.from_numpy(np.clip(pg[:, 0], 0, W - 1))
    nw, fin_given = torch.from_numpy(np.maximum(pg[:, 1], 0)), torch.from_numpy(pg[:, 2] != 0)
    fin = fin_given | bad
    path = torch.full((B, n_max + 1, 7), float("nan"), dtype=dtype)
    arc = torch.full((B, n_max + 1), float("nan"), dtype=dtype)
    path[:, 0], arc[:, 0] = q, 0
    steps = torch.zeros(B, dtype=torch.int32)
    states = {"v": [v.clone()], "w": [w.clone()], "nw": [nw.clone()]} if record_states else None
    fragile = torch.zeros(B, n_max, dtype=torch.bool)
    kinds = {k: torch.zeros(B, dtype=torch.bool) for k in ("switch", "stop", "gradient", "clamp")}
    repel_g = torch.zeros(B, dtype=dtype)
    for i in range(1, n_max + 1):
        if bool(fin.all()):
            break
        qn, v, w, nw, fin, info = step(q, v, w, nw, fin, P, scene, lo, hi, opt, True, with_base_link)
        took = info["took"]
        fragile[:, i - 1] = info["fragile"]
        for k, f in info["fragile_kinds"].items():
            kinds[k] |= f
        path[took, i] = qn[took]
        arc[took, i] = arc[took, i - 1] + torch.linalg.norm(qn - q, dim=-1)[took]
        steps[took] = i
        repel_g = torch.where(took, torch.maximum(repel_g, info["repel_g"]), repel_g)
        q = qn
        if record_states:
            for k, t in (("v", v), ("w", w), ("nw", nw)):
                states[k].append(t.clone())
    fin_out = torch.where(bad, fin_given, fin)
    q_end = np.where(bad.numpy()[:, None], qs32.astype(q.numpy().dtype), q.numpy())
    return {"path": path.numpy(), "arc": arc.numpy(), "steps": steps.numpy(), "q_end": q_end, "v_end": v.numpy(),
            "progress_end": np.stack([np.where(bad.numpy(), pg[:, 0], w.numpy()),
                                      np.where(bad.numpy(), pg[:, 1], nw.numpy()),
                                      fin_out.numpy().astype(np.int64)], -1).astype(np.int32),
            "states": None if states is None else {k: torch.stack(t, 1).numpy() for k, t in states.items()},
            "bad": bad.numpy(), "fragile": fragile.numpy(), "fragile_kinds": {k: f.numpy() for k, f in kinds.items()}, "repel_g": repel_g.numpy(), "options": opt}


def retime(path, arc, steps, T, dtype=np.float64):
    """path [B,N,7], arc [B,N], steps [B] -> [B,T,7] in ``dtype``: waypoint t at arc length (t / (T-1)) arc[n] on the last
    segment i <= n-1 with arc[i] <= s_t; waypoints 0 and T-1 are path[0] and path[n] themselves; n = 0: T copies of path[0]."""
    path, arc = np.asarray(path, dtype), np.asarray(arc, dtype)
    B = path.shape[0]
    out = np.empty((B, T, 7), dtype)
    frac = (np.arange(T, dtype=dtype) / dtype(T - 1)).astype(dtype)
    for b in range(B):
        n = int(steps[b])
        if n == 0:
            out[b] = path[b, 0]
            continue
        s = (frac * arc[b, n]).astype(dtype)
        i = np.clip(np.searchsorted(arc[b, :n + 1], s, side="right") - 1, 0, n - 1)
        den = arc[b, i + 1] - arc[b, i]
        f = np.where(den > 0, np.clip((s - arc[b, i]) / np.where(den > 0, den, 1), 0, 1), 0).astype(dtype)
        out[b] = path[b, i] + f[:, None] * (path[b, i + 1] - path[b, i])
        out[b, 0], out[b, -1] = path[b, 0], path[b, n]
    return out


def miss_distance(traj_last, poses):
    """|p_{W-1} - right_gripper(q_{T-1})| in float64 -> [B]."""
    _, t = orc.fk_frames_torch(torch.from_numpy(np.asarray(traj_last, np.float64)))
    return torch.linalg.norm(torch.from_numpy(np.asarray(poses, np.float64))[:, -1, :3, 3] - t[:, RIGHT_GRIPPER], dim=-1).numpy()


def verdict(traj, poses, scene, opt, with_base_link=False):
    """traj [B,T,7] -> int32 [B]: ``float64_plan.validity`` (bits 0-2) | BIT_MISS, in float64."""
    tr = torch.from_numpy(np.asarray(traj, np.float64))
    bits = fp.validity(tr[:, None], scene if _has_prims(scene) else None, opt["substeps"], opt["check_margin"],
                       opt["clearance"], opt["max_jerk"], bool(opt["check_self"]), with_base_link)[:, 0].numpy()
    miss = ~(miss_distance(tr[:, -1].numpy(), poses) <= opt["miss_tol"] * MISS_SHARE)
    return (bits | miss.astype(np.int32) * BIT_MISS).astype(np.int32)


def follow(q_start, poses, scene=None, limits=ft.JOINT_LIMITS_REAL, T=50, v_init=None, progress=None, dtype=torch.float64,
           with_base_link=False, **given):
    """Like ``robot.franka_follow(..., return_path=True, return_state=True)`` -> the ``rollout`` dict plus ``traj_any``,
    ``traj``, ``bits``, ``status``."""
    out = rollout(q_start, poses, scene, limits, v_init, progress, dtype, with_base_link, **given)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    B = out["steps"].shape[0]
    ok = ~out["bad"]
    traj_any = np.full((B, T, 7), np.nan, npdt)
    bits = np.full(B, 15, np.int32)
    if ok.any():
        traj_any[ok] = retime(out["path"][ok], out["arc"][ok], out["steps"][ok], T, npdt)
        sc = None if scene is None else {k: v[ok] for k, v in scene.items()}
        bits[ok] = verdict(traj_any[ok], np.asarray(poses, np.float32)[ok], sc, out["options"], with_base_link)
    traj = traj_any.copy()
    traj[bits != 0] = np.nan
    out.update(traj_any=traj_any, traj=traj, bits=bits, status=np.where(out["bad"], 2, (bits != 0).astype(np.int32)).astype(np.int32))
    return out


# ---- the inputs the host and the GPU tests share --------------------------------------------------------------------------
PROBLEM_SEED = 15  # ``problems``: the draws below are numpy's default_rng(PROBLEM_SEED + attempt).  Chosen on the CPU, from the
# float64 restatement alone and before any device run, so that the fragile rows stay under the caps of the GPU tests (the
# stop test |p - p_W-1| < 5 mm is approached at ~0.3 mm a step: about one row in ten lands within 1e-5 m of it)
GUIDE_POSES = 8
CUBOID_SIDE, CUBOID_OFFSET, CUBOID_AT = 0.1, 0.13, 3  # a 0.1 m cube, 0.13 m beside the FOURTH guide pose (index 3)


def guide_of_line(q_start, q_goal, W=GUIDE_POSES):
    """float32 [B,W,4,4]: the right_gripper pose (``oracle.franka_fk``, float32) of the straight joint line at s = i / W,
    i = 1..W -- the last pose is that of q_goal."""
    qs, qg = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    s = (np.arange(1, W + 1, dtype=np.float64) / W)[None, :, None]
    line = (qs[:, None] + s * (qg[:, None].astype(np.float64) - qs[:, None])).astype(np.float32)
    frames = orc.franka_fk(line.reshape(-1, 7))[:, RIGHT_GRIPPER]
    return orc.frames_to_4x4(frames).reshape(qs.shape[0], W, 4, 4).astype(np.float32)


def _scene_arrays(B, centres=None):
    """One cuboid per problem (a cube of CUBOID_SIDE at ``centres``; without centres a zero-volume row) and one zero-volume
    cylinder: the arrays of ``scenes.make_scenes``."""
    dims = np.zeros((B, 1, 3), np.float32) if centres is None else np.full((B, 1, 3), CUBOID_SIDE, np.float32)
    quat = np.tile(np.asarray([1, 0, 0, 0], np.float32), (B, 1, 1))
    return {"cuboid_centers": np.zeros((B, 1, 3), np.float32) if centres is None else centres.reshape(B, 1, 3).astype(np.float32),
            "cuboid_dims": dims, "cuboid_quats": quat, "cylinder_centers": np.zeros((B, 1, 3), np.float32),
            "cylinder_radii": np.zeros((B, 1, 1), np.float32), "cylinder_heights": np.zeros((B, 1, 1), np.float32),
            "cylinder_quats": quat.copy()}


def problems(B=32, seed=PROBLEM_SEED):
    """-> q_start, q_goal float32 [B,7], guide float32 [B,8,4,4], and the scene arrays of the BESIDE-CUBOID problems (the
    free-space problems are the same starts, goals and guides without the scene).

    Construction: start and goal uniform in the middle 80 % of the joint limits (numpy default_rng(seed + attempt)); the
    guide is ``guide_of_line``; the cube's centre is guide pose CUBOID_AT's position moved CUBOID_OFFSET along the guide
    frame's x axis.  A draw is kept when start and goal pass the planner's configuration test (spheres against the cube with
    the 1e-4 m margin, the self model) and the guide's positions stay 0.12 m clear of the base axis and above z = 0.05;
    rejected rows are drawn again, at most 64 times."""
    lim = np.asarray(ft.JOINT_LIMITS_REAL, np.float64)
    mid, half = lim.mean(1), 0.4 * (lim[:, 1] - lim[:, 0])
    qs, qg = np.zeros((B, 7), np.float32), np.zeros((B, 7), np.float32)
    todo = np.ones(B, bool)
    for attempt in range(64):
        rng = np.random.default_rng(seed + attempt)
        a = (mid + half * rng.uniform(-1, 1, (B, 7))).astype(np.float32)
        g = (mid + half * rng.uniform(-1, 1, (B, 7))).astype(np.float32)
        qs[todo], qg[todo] = a[todo], g[todo]
        guide = guide_of_line(qs, qg)
        centres = guide[:, CUBOID_AT, :3, 3] + CUBOID_OFFSET * guide[:, CUBOID_AT, :3, 0]
        scene = fp.scene_from_arrays(_scene_arrays(B, centres))
        ends = torch.from_numpy(np.concatenate([qs, qg])).double()
        both = {k: np.concatenate([v, v]) for k, v in scene.items()}
        cb = fp.config_bits(ends, both, 1, 1e-4, True, 1e-4).numpy().reshape(2, B)
        pos = guide[:, :, :3, 3]
        clear = (np.hypot(pos[..., 0], pos[..., 1]).min(1) > 0.12) & (pos[..., 2].min(1) > 0.05)
        todo = (cb != 0).any(0) | ~clear
        if not todo.any():
            break
    assert not todo.any(), "problems: a row found no admissible draw"
    return qs, qg, guide, _scene_arrays(B, centres)
