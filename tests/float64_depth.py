"""Restatement of the depth camera (``mpx_depth_render``, ``mpx_depth_select``) on the CPU, in float64 by default, written
from the contract in include/mpinets_hip.h and not from csrc/depth_device.h.

The method is not the kernel's.  Every primitive is a convex set, the intersection of its constraints (three slabs for a
cuboid; an infinite tube and one slab for a cylinder; one ball for a robot sphere), and a ray meets it on the intersection
[tn, tf] of the constraints' parameter intervals.  A hit is ``tn <= tf and tn > 0`` at depth tn, so an origin inside
(tn <= 0) sees nothing of that primitive: the camera-inside rule of the header.  The kernel picks roots and caps one by one.

Inputs are the float32 arrays the entry reads (camera poses, intrinsics, the STORED inverse frames -- taken as given, so
frames that are no rotations are covered -- sizes, sphere centres and radii, far_clip), evaluated in ``dtype``;
``torch.float32`` runs the same statements in float32: the reference-against-reference figure (e32) the tolerances of
tests/test_gpu_depth_float64.py are made of.

``leave_out`` marks the pixels where a decision is within ``margin`` of flipping, judged geometrically:
* a silhouette: an entry of one constraint within the margin of the exit of ANOTHER, both binding (a thin plate's own
  entry and exit are 2e-8 apart and never cross, so they do not count), a ray that passes a tube or a ball within the
  margin of its radius, a ray parallel to a face within the margin of its plane, an origin within the margin of a surface;
  each only where it can change the pixel, i.e. not behind the nearest hit;
* the nearest obstacle and a robot sphere within the margin of each other;
* a depth within the margin of far_clip.

The seeded case builders at the end make the inputs of the GPU tests; tests/test_depth_host.py checks the restatement, the
leave-out caps and the CPU oracle on the same arrays without a GPU.
"""
import functools
import math

import numpy as np
import torch

import float64_plan as fp
from float64_ik import philox4x32_np
from mpinets_amd import franka_tables as ft
from mpinets_amd import scenes
from mpinets_amd.depth import camera_pose
from oracle import oracle as orc

FRAGILE = fp.FRAGILE
LEAVE_OUT_CAP = 0.01
STREAM_DEPTH = 9
MIXED = ("tabletop", "cubby", "dresser")
INF = float("inf")


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


# ---------------------------------------------------------------- rays
def rays(poses, intr, W, H, pix=None, dtype=torch.float64):
    """poses float32 [B,4,4] (world from camera, OpenGL axes), intr = (fx, fy, cx, cy) as the float32 the entry receives
    -> origin [B,3] and unit directions [B,P,3] of the pixels ``pix`` (int [P] or [B,P]; all W*H pixels by default):
    the camera-frame direction ((u + 0.5 - cx) / fx, -(v + 0.5 - cy) / fy, -1), rotated, normalised in world space."""
    P = _t(poses, dtype)
    fx, fy, cx, cy = (float(np.float32(x)) for x in intr)
    pix = torch.arange(W * H) if pix is None else torch.as_tensor(np.asarray(pix)).long()
    u, v = (pix % W).to(dtype), torch.div(pix, W, rounding_mode="floor").to(dtype)
    dc = torch.stack([(u + 0.5 - cx) / fx, -((v + 0.5 - cy) / fy), -torch.ones_like(u)], -1)
    if dc.ndim == 2:
        dc = dc[None].expand(P.shape[0], -1, -1)
    dw = torch.einsum("bij,bpj->bpi", P[:, :3, :3], dc)
    return P[:, :3, 3], dw / torch.linalg.norm(dw, dim=-1, keepdim=True)


def back_project(depth32, poses, intr, W, H, pix, dtype=torch.float64):
    """depth32 float32 [B,H*W], pix int [B,n] -> world points [B,n,3] = o + s d of those pixels, s their stored depth."""
    o, d = rays(poses, intr, W, H, pix, dtype)
    pix = torch.as_tensor(np.asarray(pix)).long()
    s = torch.gather(_t(depth32, dtype).reshape(d.shape[0], -1), 1, pix)
    return o[:, None, :] + s[..., None] * d


# ---------------------------------------------------------------- parameter intervals
def _slab(lo, ld, half, margin):
    """|lo + t ld| <= half.  lo, half [..., 1], ld [..., P] -> entry, exit [..., P] ((-inf, inf) for a parallel ray between
    the planes, (inf, -inf) for one outside them) and bool: parallel within the margin of a plane."""
    par = ld == 0
    safe = torch.where(par, torch.ones_like(ld), ld)
    t1, t2 = (-half - lo) / safe, (half - lo) / safe
    inside = (lo.abs() <= half).expand_as(ld)
    pinf, ninf = torch.full_like(ld, INF), torch.full_like(ld, -INF)
    tin = torch.where(par, torch.where(inside, ninf, pinf), torch.minimum(t1, t2))
    tout = torch.where(par, torch.where(inside, pinf, ninf), torch.maximum(t1, t2))
    return tin, tout, par & ((lo.abs() - half).abs() < margin)


def _round(b, a, c, r, margin):
    """a t^2 + 2 b t + c <= 0 (a tube or a ball; c = |l|^2 - r^2) -> entry, exit, the parameter of the closest approach
    and bool: the ray passes within the margin of the radius."""
    par = a == 0
    safe = torch.where(par, torch.ones_like(a), a)
    disc = b * b - a * c
    root = torch.sqrt(torch.clamp(disc, min=0))
    pinf, ninf = torch.full_like(b, INF), torch.full_like(b, -INF)
    miss = disc < 0
    tin = torch.where(par, torch.where(c <= 0, ninf, pinf), torch.where(miss, pinf, (-b - root) / safe))
    tout = torch.where(par, torch.where(c <= 0, pinf, ninf), torch.where(miss, ninf, (-b + root) / safe))
    rho = torch.sqrt(torch.clamp(c + r * r - torch.where(par, torch.zeros_like(b), b * b / safe), min=0))
    return tin, tout, torch.where(par, torch.zeros_like(b), -b / safe), (rho - r).abs() < margin


def _convex(tin, tout, margin):
    """Constraint intervals [B,M,K,P] -> tn, tf [B,M,P] and bool: an entry and the exit of another constraint, both
    binding, within the margin of each other."""
    tn, tf = tin.amax(2), tout.amin(2)
    frag = torch.zeros_like(tn, dtype=torch.bool)
    K = tin.shape[2]
    for i in range(K):
        for j in range(K):
            if i != j:
                frag |= ((tin[:, :, i] - tout[:, :, j]).abs() < margin) & (tin[:, :, i] >= tn - margin) & \
                        (tout[:, :, j] <= tf + margin)
    return tn, tf, frag


def _local(F, o, d):
    lo = torch.einsum("bmij,bj->bmi", F[:, :, :3, :3], o) + F[:, :, :3, 3]
    return lo[..., None], torch.einsum("bmij,bpj->bmip", F[:, :, :3, :3], d)  # [B,M,3,1], [B,M,3,P]


def _reach(tn, tf):
    """Where along the ray a primitive's decision is taken: its entry, or its exit when it has no finite entry."""
    return torch.where(torch.isfinite(tn), tn, tf)


def render(poses, intr, W, H, scene, sph_centers=None, sph_radii=None, far_clip=10.0, dtype=torch.float64, margin=FRAGILE):
    """-> dict: ``depth`` [B,H*W] in ``dtype`` (-1 for an empty pixel), bool ``leave_out`` [B,H*W], and ``obstacle``
    [B,H*W] (the nearest obstacle entry before the robot and the far clip are applied, +inf without one).  ``scene`` is the
    dict of ``float64_plan.scene_from_arrays``."""
    o, d = rays(poses, intr, W, H, None, dtype)
    B, P = d.shape[:2]
    far = float(np.float32(far_clip))
    hits, frags = [], []  # per family: entry [B,M,P] (+inf where not hit), (fragile [B,M,P], where [B,M,P])
    cd = _t(scene["cub_dims"], dtype)
    if cd.shape[1]:
        lo, ld = _local(_t(scene["cub_frames"], dtype), o, d)
        tin, tout, edge = _slab(lo, ld, (cd / 2)[..., None], margin)
        tn, tf, frag = _convex(tin, tout, margin)
        live = ~(cd.abs() <= 1e-8).any(-1)[..., None]
        hits.append(torch.where(live & (tn <= tf) & (tn > 0), tn, torch.full_like(tn, INF)))
        frags.append((live & (frag | edge.any(2) | ((tn.abs() < margin) & (tn <= tf + margin))), _reach(tn, tf)))
    yr, yh = _t(scene["cyl_radii"], dtype), _t(scene["cyl_heights"], dtype)
    if yr.shape[1]:
        lo, ld = _local(_t(scene["cyl_frames"], dtype), o, d)
        a = ld[:, :, 0] * ld[:, :, 0] + ld[:, :, 1] * ld[:, :, 1]
        b = lo[:, :, 0] * ld[:, :, 0] + lo[:, :, 1] * ld[:, :, 1]
        c = (lo[:, :, 0] * lo[:, :, 0] + lo[:, :, 1] * lo[:, :, 1] - (yr * yr)[..., None]).expand_as(a)
        t_in, t_out, t_star, graze = _round(b, a, c, yr[..., None], margin)
        s_in, s_out, edge = _slab(lo[:, :, 2], ld[:, :, 2], (yh / 2)[..., None], margin)
        tn, tf, frag = _convex(torch.stack([t_in, s_in], 2), torch.stack([t_out, s_out], 2), margin)
        graze = graze & (t_star >= s_in - margin) & (t_star <= s_out + margin)
        live = ~((yr.abs() <= 1e-8) | (yh.abs() <= 1e-8))[..., None]
        hits.append(torch.where(live & (tn <= tf) & (tn > 0), tn, torch.full_like(tn, INF)))
        frags.append((live & (frag | edge | ((tn.abs() < margin) & (tn <= tf + margin))), _reach(tn, tf)))
        frags.append((live & graze, t_star))
    obstacle = torch.cat(hits, 1).amin(1) if hits else torch.full((B, P), INF, dtype=dtype)
    best = torch.clamp(obstacle, max=far)
    leave = (obstacle - far).abs() < margin
    robot = torch.zeros(B, P, dtype=torch.bool)
    if sph_centers is not None and np.asarray(sph_centers).shape[1]:
        r = _t(sph_radii, dtype)[None, :, None]
        m = o[:, None, :] - _t(sph_centers, dtype)  # [B,S,3]
        b = torch.einsum("bsi,bpi->bsp", m, d)
        c = ((m * m).sum(-1)[..., None] - r * r).expand_as(b)
        tn, tf, t_star, graze = _round(b, torch.ones_like(b), c, r, margin)
        entry = torch.where((tn <= tf) & (tn > 0), tn, torch.full_like(tn, INF))
        robot = (entry < best[:, None]).any(1)
        leave = leave | ((entry - best[:, None]).abs() < margin).any(1)
        frags.append((graze, t_star))
        frags.append(((tn.abs() < margin) & (tn <= tf), tn))
    for frag, where in frags:  # a fragile decision counts where it can change the pixel: not behind the nearest hit
        leave = leave | (frag & (where > -margin) & (where < best[:, None] + margin)).any(1)
    depth = torch.where(robot | ~(obstacle < far), torch.full_like(best, -1.0), best)
    return {"depth": depth, "leave_out": leave, "obstacle": obstacle}


def render_pair(inp, margin=None):
    """``inp``: the dict of ``inputs`` -> the float64 result with the figures the tolerances are made of: ``keep`` (not left
    out), ``left_out`` (share of the pixels), ``e32`` (largest float32-versus-float64 depth difference over the kept pixels
    valid in both) and ``flips32`` (kept pixels whose validity differs between the two)."""
    margin = inp["margin"] if margin is None else margin
    args = (inp["poses"], inp["intr"], inp["W"], inp["H"], inp["scene"], inp["sph_centers"], inp["sph_radii"], inp["far_clip"])
    r = render(*args, margin=margin)
    r32 = render(*args, dtype=torch.float32, margin=margin)
    r["keep"] = ~r["leave_out"]
    r["left_out"] = float(r["leave_out"].double().mean())
    r["flips32"], r["e32"] = judge(r32["depth"].numpy(), r)
    return r


def judge(depth32, r):
    """A float32 depth image [B,H*W] (the oracle's, the device's) against the float64 result -> (kept pixels whose validity
    differs, the largest depth difference over the kept pixels valid in both)."""
    got = torch.from_numpy(np.asarray(depth32, np.float32).reshape(r["depth"].shape)).double()
    keep = ~r["leave_out"]
    v_got, v_want = got >= 0, r["depth"] >= 0
    both = keep & v_got & v_want
    err = float((got - r["depth"]).abs()[both].max()) if bool(both.any()) else 0.0
    return int((keep & (v_got != v_want)).sum()), err


# ---------------------------------------------------------------- the subset draw
def select_pixels(depth32, n_out, seed, env_offset=0):
    """depth32 float32 [B,HW] -> count int [B] (pixels with depth >= 0: -0.0 counts, NaN and -1 do not) and per row the
    n_out pixels with the smallest (Philox key, pixel id) in that order, or None for a row with fewer valid pixels.  Pixel
    p of row b has word p & 3 of Philox4x32-10(counter (p >> 2, env_offset + b, 9, 0), key (seed lo, seed hi))."""
    d = np.asarray(depth32, np.float32)
    B, HW = d.shape
    pix = np.arange(HW, dtype=np.uint64)
    env = ((env_offset + np.arange(B, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))[:, None]
    words = philox4x32_np((pix >> np.uint64(2))[None, :], env, STREAM_DEPTH, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    key = np.choose((pix & np.uint64(3)).astype(np.int64)[None, :], [w.astype(np.uint64) for w in words])
    key = (key << np.uint64(32)) | pix[None, :]
    valid = d >= 0
    rows = []
    for b in range(B):
        k = np.sort(key[b][valid[b]])
        rows.append((k[:n_out] & np.uint64(0xFFFFFFFF)).astype(np.int64) if len(k) >= n_out else None)
    return valid.sum(1).astype(np.int32), rows


def populations(W, H, counts, seed, values=(0.3, 4.0)):
    """Synthetic depth images float32 [B,H*W]: row b has exactly counts[b] valid pixels at seeded places with depths in
    ``values``' range, -1 elsewhere."""
    rng = np.random.default_rng(seed)
    d = np.full((len(counts), W * H), -1.0, np.float32)
    for b, n in enumerate(counts):
        where = rng.permutation(W * H)[:n]
        d[b, where] = rng.uniform(values[0], values[1], n).astype(np.float32)
    return d


def tilted_poses(B, seed):
    """float32 [B,4,4]: seeded rotations (exact to float32 rounding) with origins within half a metre of (0, 0, 1)."""
    rng = np.random.default_rng(seed)
    P = np.zeros((B, 4, 4))
    for b in range(B):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        P[b, :3, :3] = q * np.sign(np.linalg.det(q))
        P[b, :3, 3] = (0, 0, 1) + rng.uniform(-0.5, 0.5, 3)
        P[b, 3, 3] = 1
    return P.astype(np.float32)


# ---------------------------------------------------------------- seeded cases
IDENTITY = np.eye(4, dtype=np.float32)
Q0 = (1.0, 0.0, 0.0, 0.0)
Q_ROLL = (math.sqrt(0.5), math.sqrt(0.5), 0.0, 0.0)  # the local z axis along world y, to float32 rounding (ez ~ 1e-7 on the centre row)
# a camera at (2.5, 0, 0) that looks along -x with world z up, an exact permutation: the world z component of its centre
# row's directions is exactly 0
POSE_SIDE = np.asarray([[0, 0, 1, 2.5], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float32)
Q_TILT = (0.9, 0.3, 0.2, 0.1)
Q_LOOSE = ((1.7, -0.8, 1.1, 0.6), (-1.2, 0.9, 0.7, -1.5))  # not unit length: the stored frames are no rotations
CRAFTED = (20.0, 20.0, 16.5, 8.5)  # 33 x 17, centre pixel (16, 8) looks exactly along -z; 0.1 m a pixel at 2 m
W0, H0 = 33, 17


def intrinsics(W, H, vertical_fov_deg=60.0):
    """DepthCamera's: square pixels, the principal point in the middle."""
    f = 0.5 * H / math.tan(math.radians(vertical_fov_deg) / 2)
    return (f, f, W / 2.0, H / 2.0)


def empty_scene(B, M1, M2):
    z = lambda *s: np.zeros(s, np.float32)
    scn = {"cuboid_centers": z(B, M1, 3), "cuboid_dims": z(B, M1, 3), "cuboid_quats": z(B, M1, 4),
           "cylinder_centers": z(B, M2, 3), "cylinder_radii": z(B, M2, 1), "cylinder_heights": z(B, M2, 1),
           "cylinder_quats": z(B, M2, 4)}
    scn["cuboid_quats"][..., 0] = 1
    scn["cylinder_quats"][..., 0] = 1
    return scn


def put_box(scn, b, m, centre, dims, quat=Q0):
    scn["cuboid_centers"][b, m], scn["cuboid_dims"][b, m], scn["cuboid_quats"][b, m] = centre, dims, quat


def put_cyl(scn, b, m, centre, radius, height, quat=Q0):
    scn["cylinder_centers"][b, m], scn["cylinder_quats"][b, m] = centre, quat
    scn["cylinder_radii"][b, m, 0], scn["cylinder_heights"][b, m, 0] = radius, height


def case(name, scn, poses=None, intr=CRAFTED, W=W0, H=H0, spheres=None, far_clip=10.0, margin=FRAGILE, capped=True, group=None):
    B = scn["cuboid_dims"].shape[0]
    poses = np.repeat(IDENTITY[None], B, 0) if poses is None else np.asarray(poses, np.float32)
    return {"name": name, "scn": scn, "poses": poses, "intr": tuple(float(x) for x in intr), "W": W, "H": H,
            "spheres": spheres, "far_clip": float(far_clip), "margin": margin, "capped": capped, "group": group or name}


def inputs(c, frames=None):
    """A case -> the arrays the entry reads.  ``frames`` = (cuboid, cylinder) inverse frames [B,M,4,4] of the library's own
    TorchCuboids / TorchCylinders in a GPU test; the oracle's by default (equal to rounding)."""
    scene = fp.scene_from_arrays(c["scn"])
    if frames is not None:
        scene["cub_frames"], scene["cyl_frames"] = (np.asarray(f, np.float32) for f in frames)
    sc, sr = c["spheres"] if c["spheres"] is not None else (None, None)
    return {"poses": c["poses"], "intr": c["intr"], "W": c["W"], "H": c["H"], "scene": scene, "sph_centers": sc,
            "sph_radii": sr, "far_clip": c["far_clip"], "margin": c["margin"]}


def oracle_render(c):
    """The float32 CPU oracle (the kernel's statements in the kernel's order) on a case."""
    s = {k: v for k, v in c["scn"].items()}
    B = s["cuboid_dims"].shape[0]
    pad = empty_scene(B, 1, 1)  # (the ctypes face wants one row per family: a zero-volume one)
    for fam in ("cuboid", "cylinder"):
        if s[fam + "_centers"].shape[1] == 0:
            s.update({k: v for k, v in pad.items() if k.startswith(fam)})
    sc, sr = c["spheres"] if c["spheres"] is not None else (None, None)
    return orc.depth_render(c["poses"], c["intr"], c["W"], c["H"],
                            (s["cuboid_centers"], s["cuboid_dims"], orc.repair_quaternions(s["cuboid_quats"])),
                            (s["cylinder_centers"], s["cylinder_radii"], s["cylinder_heights"],
                             orc.repair_quaternions(s["cylinder_quats"])), sc, sr, c["far_clip"])


def franka_spheres(q):
    """q float32 [B,7] -> (centres float32 [B,S,3], radii float32 [S]) of FrankaCollisionSampler(with_base_link=True), by
    the oracle's FK (a GPU test hands over the device's own centres)."""
    c, r, l, _ = ft.collision_sphere_table(True)
    return orc.transform_table(orc.franka_fk(np.asarray(q, np.float32)), c, l), np.asarray(r, np.float32)


def eval_poses(kinds, forward=0.0):
    """The evaluation camera of each kind, moved ``forward`` metres along its viewing direction."""
    P = np.stack([camera_pose(k) for k in kinds])
    P[:, :3, 3] -= np.float32(forward) * P[:, :3, 2]
    return P


LAUNCH_SIZES = ((1, 1), (3, 1), (17, 15), (16, 16), (257, 1), (33, 17))
LAUNCH_BATCHES = (1, 5)


def launch_name(W, H, B):
    return f"r2_{W}x{H}_B{B}"


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, every render case of the GPU test."""
    out = {}

    def add(c):
        out[c["name"]] = c

    # R1: generated scenes from the evaluation cameras, without and with the robot
    for name, seed, robot in (("r1_scenes", 2, False), ("r1_robot", 5, True)):
        scn = scenes.make_scenes(3, seed, MIXED, 16, 8)
        q = scenes.random_configurations(3, seed + 1)
        add(dict(case(name, scn, eval_poses(MIXED), intrinsics(64, 48), 64, 48, franka_spheres(q) if robot else None),
                 q=q if robot else None))
    # R2: launch edges on a one-box scene; env b looks from its own place (a batch index that slips shows)
    for W, H in LAUNCH_SIZES:
        for B in LAUNCH_BATCHES:
            scn = empty_scene(B, 1, 1)
            poses = np.repeat(IDENTITY[None], B, 0)
            for b in range(B):
                put_box(scn, b, 0, (0.05, 0.03, -2.5), (1.13, 0.77, 1.0))
                poses[b, :3, 3] = (0.07 * b, -0.05 * b, 0.1 * b)
            f = 0.6 * max(W, H)
            add(case(launch_name(W, H, B), scn, poses, (f, f, W / 2.0, H / 2.0), W, H, group="r2"))
    # R3: the centre pixel's ray is parallel to four faces of every axis-aligned box; the centre row and column to two
    scn = empty_scene(2, 2, 1)
    put_box(scn, 0, 0, (0, 0, -2.5), (1.1, 0.7, 1.0))  # straddles the axis
    put_box(scn, 1, 0, (0.8, 0.5, -2.5), (0.5, 0.5, 1.0))  # clear of it: front, left and bottom faces are seen
    put_box(scn, 1, 1, (-0.9, -0.62, -3.5), (0.5, 0.3, 1.0))
    add(case("r3_parallel", scn))
    scn = empty_scene(1, 1, 1)
    put_box(scn, 0, 0, (0.25, 0, -2.5), (0.5, 0.7, 1.0))  # the face x = 0 holds the axis: the centre column is all edge,
    add(case("r3_face_plane", scn, capped=False))          # 17 of 561 pixels, so this case has no leave-out cap
    # R4: cylinders
    scn = empty_scene(5, 1, 1)
    put_cyl(scn, 0, 0, (0, 0, -2.5), 0.55, 1.0)  # axis along the view: the centre pixel meets the caps only (a = 0)
    put_cyl(scn, 1, 0, (0, 0, 0), 0.45, 1.1)  # seen from POSE_SIDE: axis exactly across, ez = 0 on the centre row
    put_cyl(scn, 2, 0, (0.2, -0.1, -2.5), 0.4, 0.8, Q_TILT)  # oblique: the silhouette crosses a cap rim
    put_cyl(scn, 3, 0, (-0.1, 0.2, -2.0), 0.45, 0.01, Q_TILT)  # height 0.01
    put_cyl(scn, 4, 0, (0.3, 0.1, -2.2), 0.3, 0.9, (0.7, -0.4, 0.5, 0.2))
    poses = np.repeat(IDENTITY[None], 5, 0)
    poses[1] = POSE_SIDE
    add(case("r4_cylinders", scn, poses))
    scn = empty_scene(1, 1, 1)
    put_cyl(scn, 0, 0, (0, 0, -4.0), 0.01, 0.1, Q_ROLL)  # radius 0.01 at 4 m, 1 mm a pixel: b*b - a*c cancels
    add(case("r4_thin_far", scn, intr=(4000.0, 4000.0, 16.75, 8.5)))
    # R5: frames that are no rotations
    scn = empty_scene(3, 1, 1)
    put_box(scn, 0, 0, (0.1, -0.1, -2.5), (0.9, 0.6, 0.7), Q_LOOSE[0])
    put_cyl(scn, 1, 0, (-0.1, 0.1, -2.5), 0.4, 0.7, Q_LOOSE[1])
    put_box(scn, 2, 0, (-0.3, 0.1, -2.6), (0.6, 0.8, 0.5), Q_LOOSE[1])
    put_cyl(scn, 2, 0, (0.4, -0.1, -2.4), 0.3, 0.9, Q_LOOSE[0])
    add(case("r5_loose_frames", scn))
    # R6: masks and empties.  Read as live, every masked row would be the nearest hit of its pixels.
    scn = empty_scene(1, 5, 4)
    put_box(scn, 0, 0, (0, 0, -1.2), (1.3, 0.0, 0.5))  # one zero dim
    put_box(scn, 0, 1, (0.4, 0.3, -1.5), (0.7, 0.5, 1e-8))  # a size of exactly 1e-8: skipped
    put_box(scn, 0, 2, (-0.4, -0.3, -2.0), (0.7, 0.5, 2e-8))  # 2e-8: kept, a plate with no thickness to speak of
    put_box(scn, 0, 3, (0, 0, -3.5), (3.1, 1.7, 1.0))
    put_cyl(scn, 0, 0, (-0.5, 0.3, -1.0), 0.0, 0.5, Q_TILT)  # radius 0
    put_cyl(scn, 0, 1, (0.5, -0.3, -1.1), 0.3, 0.0, Q_TILT)  # height 0
    put_cyl(scn, 0, 2, (0.55, -0.25, -2.0), 0.25, 0.5, Q_TILT)
    put_cyl(scn, 0, 3, (-0.45, 0.35, -1.6), 0.3, 1e-8)  # height of exactly 1e-8: skipped
    add(case("r6_masked", scn))
    live = {k: v[:, 2:4] if k.startswith("cuboid") else v[:, 2:3] for k, v in scn.items()}
    add(case("r6_no_cuboids", {k: (v[:, :0] if k.startswith("cuboid") else v) for k, v in live.items()}))
    add(case("r6_no_cylinders", {k: (v[:, :0] if k.startswith("cylinder") else v) for k, v in live.items()}))
    add(case("r6_nothing", {k: v[:, :0] for k, v in live.items()}))
    # R7: the far clip.  Plates facing the camera, 0.025 m a pixel at 10 m.
    scn = empty_scene(2, 2, 1)
    put_box(scn, 0, 0, (-1.5125, 0, -9.995), (3.0, 3.0, 0.01))  # front face at 9.99 m: kept where the ray is short enough
    put_box(scn, 0, 1, (1.5125, 0, -10.015), (3.0, 3.0, 0.01))  # at 10.01 m: clipped everywhere
    put_box(scn, 1, 0, (0, 0, -10.0), (3.0, 3.0, 0.01))  # at 9.995 m: the clip cuts a circle of 12.6 pixels out of it
    add(case("r7_plates", scn, intr=(400.0, 400.0, 16.5, 8.5)))
    add(case("r7_clip_scene", scenes.make_scenes(3, 2, MIXED, 16, 8), eval_poses(MIXED, 1.3), intrinsics(64, 48), 64, 48,
             far_clip=1.0))
    # R8: the robot as spheres: in front of the box, behind it, in front of nothing, beyond far_clip, over the box's edge
    scn = empty_scene(1, 1, 1)
    put_box(scn, 0, 0, (0, 0, -2.5), (1.5, 1.1, 1.0))
    sph = (np.asarray([[(-0.4, 0.2, -1.2), (0.3, 0.2, -3.6), (1.2, 0.0, -2.0), (-5.5, 1.0, -11.0), (0.6, -0.3, -1.5)]],
                      np.float32), np.asarray([0.25, 0.2, 0.3, 0.5, 0.25], np.float32))
    add(case("r8_robot", scn, spheres=sph))
    # R9: the camera inside a cuboid, a cylinder along and across the view, a robot sphere: each is invisible, and the plate
    # behind it is seen at its own depth
    scn = empty_scene(4, 2, 1)
    for b in range(4):
        put_box(scn, b, 0, (0, 0, -3.0625), (6.0, 4.0, 0.125))  # front face at exactly 3 m
    put_box(scn, 0, 1, (0.3, -0.2, 0.1), (2.0, 2.0, 2.0))
    put_cyl(scn, 1, 0, (0.2, 0.1, -0.3), 1.0, 2.0)
    put_cyl(scn, 2, 0, (0.1, -0.2, 0.2), 1.0, 0.6, Q_ROLL)  # (a cap is in view from the inside)
    sph = (np.asarray([[(0, 0, -5.0)], [(0, 0, -5.0)], [(0, 0, -5.0)], [(0.1, -0.05, 0.2)]], np.float32),
           np.asarray([0.5], np.float32))
    add(case("r9_inside", scn, spheres=sph))
    # R10: overlapping primitives: the nearest wins whichever list it is in, and wherever it stands in its list
    scn = empty_scene(2, 2, 2)
    parts = (((0, 0, -2.5), (0.9, 0.5, 0.6), Q_TILT), ((0.3, 0.13, -2.6), (0.52, 0.9, 0.8), Q0))
    rounds = (((0.1, 0, -2.45), 0.35, 0.7, Q_TILT), ((-0.3, -0.1, -2.7), 0.45, 0.5, Q_ROLL))
    for b in range(2):
        for m in range(2):
            put_box(scn, b, m if b == 0 else 1 - m, *parts[m])
            put_cyl(scn, b, m if b == 0 else 1 - m, *rounds[m])
    add(case("r10_overlap", scn))
    return out


RENDER_CASES = tuple(cases().keys())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 result of a case around the oracle's frames, with its figures (computed once, shared, left unchanged)."""
    return render_pair(inputs(cases()[name]))


@functools.lru_cache(maxsize=None)
def group_e32(group):
    """The e32 a tolerance is stated with: the largest over the cases of the group (the launch-edge images are crops of one
    scene, down to one pixel, so they share the figure of the whole group)."""
    return max(reference(n)["e32"] for n, c in cases().items() if c["group"] == group)
