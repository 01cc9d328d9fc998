"""The two depth-camera entries of csrc/depth.hip against their float64 restatement (tests/float64_depth.py), called
through ``_lib.call`` so that image sizes, NULL arguments, strides and ``env_offset`` are the test's.

Render: per case, validity is equal on every kept pixel and ``|gpu - f64| <= 4 e32`` on the kept valid ones, e32 being the
case's own float32-versus-float64 figure of the restatement (times 4, as in tests/test_gpu_loss_float64.py, because the
kernel's order of operations is not torch's); the restatement is evaluated around the device's own frames and sphere
centres.  tests/test_depth_host.py holds the same inputs to the leave-out caps without a GPU.  Select: the pixel subset and
its order are the restatement's (smallest Philox keys), the points are within 4 e32 of the float64 back-projection, e32 the
float32-versus-float64 figure of the back-projection itself.

Each test prints its measured figures (``FIGURE ...`` lines, shown with ``pytest -s``): profiles/depth_float64.md.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_depth as fd  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 12345.678
TAIL = 300


def figure(*a):
    print("FIGURE", *a)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- render
def device_scene(scn):
    """scn arrays -> the tensors the entry reads, frames made by the library's own TorchCuboids / TorchCylinders, and the
    two frame arrays on the host."""
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    t = {k: dev(v) for k, v in scn.items()}
    cub = TorchCuboids(t["cuboid_centers"], t["cuboid_dims"], t["cuboid_quats"])
    cyl = TorchCylinders(t["cylinder_centers"], t["cylinder_radii"], t["cylinder_heights"], t["cylinder_quats"])
    d = {"cub_frames": cub.inv_frames, "cub_dims": t["cuboid_dims"].contiguous(), "cyl_frames": cyl.inv_frames,
         "cyl_radii": t["cylinder_radii"][..., 0].contiguous(), "cyl_heights": t["cylinder_heights"][..., 0].contiguous()}
    return d, (cub.inv_frames.cpu().numpy(), cyl.inv_frames.cpu().numpy())


def launch_render(c, d, spheres):
    """-> depth [B,H*W] on the host.  The buffer has a sentinel tail that must stay untouched."""
    from mpinets_amd import _lib

    B, W, H = c["poses"].shape[0], c["W"], c["H"]
    buf = torch.full((B * W * H + TAIL,), SENTINEL, device=DEV)
    sc, sr = (dev(spheres[0]), dev(spheres[1])) if spheres is not None else (None, None)
    S = 0 if sc is None else sc.shape[1]
    fx, fy, cx, cy = c["intr"]
    poses = dev(c["poses"])
    _lib.call("mpx_depth_render", poses.data_ptr(), fx, fy, cx, cy, W, H, B, ptr(d["cub_frames"]), ptr(d["cub_dims"]),
              d["cub_dims"].shape[1], ptr(d["cyl_frames"]), ptr(d["cyl_radii"]), ptr(d["cyl_heights"]), d["cyl_radii"].shape[1],
              ptr(sc), ptr(sr), S, c["far_clip"], buf.data_ptr())
    torch.cuda.synchronize()
    assert same_bits(buf[B * W * H:], torch.full((TAIL,), SENTINEL, device=DEV))
    return buf[:B * W * H].reshape(B, W * H).cpu().numpy()


def run_render_case(name):
    """One case on the device against the restatement around the device's own frames -> (device depth, float64 result)."""
    c = fd.cases()[name]
    d, frames = device_scene(c["scn"])
    spheres = c["spheres"]
    if c.get("q") is not None:  # the device's own sphere centres
        from mpinets_amd.robot import FrankaCollisionSampler

        cs = FrankaCollisionSampler(DEV, with_base_link=True)
        spheres = (cs.sphere_centers(dev(c["q"])).cpu().numpy(), cs.radii.cpu().numpy())
        assert np.abs(spheres[0] - c["spheres"][0]).max() <= 1e-5 and np.array_equal(spheres[1], c["spheres"][1])
    oracle_frames = fd.inputs(c)["scene"]
    for mine, theirs in zip(frames, (oracle_frames["cub_frames"], oracle_frames["cyl_frames"])):
        assert mine.shape == theirs.shape and (mine.size == 0 or np.abs(mine - theirs).max() <= 1e-6)
    r = fd.render_pair(fd.inputs(dict(c, spheres=spheres), frames))
    got = launch_render(c, d, spheres)
    e32 = fd.group_e32("r2") if c["group"] == "r2" else r["e32"]
    flips, err = fd.judge(got, r)
    figure(name, f"B={got.shape[0]} pixels={got.shape[1]} margin={c['margin']:.3g} e32={e32:.3g} atol={4 * e32:.3g} "
                 f"left_out={r['left_out']:.4f} kept_valid={int((r['keep'] & (r['depth'] >= 0)).sum())} flips={flips} "
                 f"gpu_err={err:.3g}")
    if c["capped"]:
        assert r["left_out"] <= fd.LEAVE_OUT_CAP, (name, r["left_out"])
    assert ((got >= 0) | (got == -1)).all()  # (an empty pixel is -1, nothing else)
    assert flips == 0, (name, flips)
    assert err <= 4 * e32, (name, err, 4 * e32)
    return got, r


@pytest.mark.parametrize("name", ["r1_scenes", "r1_robot"])
def test_render_generated_scenes(name):
    """R1: three mixed scenes from the evaluation cameras, 64 x 48, with S = 0 and NULL sphere pointers, and with the Franka's
    collision spheres."""
    got, r = run_render_case(name)
    assert int((r["keep"] & (r["depth"] >= 0)).sum()) >= 100
    if name == "r1_robot":  # the robot removes pixels
        c = fd.cases()[name]
        bare = launch_render(c, device_scene(c["scn"])[0], None)
        removed = (bare >= 0) & (got < 0)
        assert removed.sum() >= 3 and ((got == bare) | removed).all()


@pytest.mark.parametrize("B", fd.LAUNCH_BATCHES)
@pytest.mark.parametrize("W,H", fd.LAUNCH_SIZES)
def test_render_launch_edges(W, H, B):
    """R2: pixel counts below, at and above the 256-thread block and no multiple of 4; the sentinel tail stays."""
    run_render_case(fd.launch_name(W, H, B))


@pytest.mark.parametrize("name", ["r3_parallel", "r4_cylinders", "r4_thin_far", "r5_loose_frames", "r6_masked",
                                  "r6_no_cuboids", "r6_no_cylinders", "r7_plates", "r7_clip_scene", "r8_robot"])
def test_render_crafted_cases(name):
    """R3 .. R8 (tests/test_depth_host.py checks on the host that each case is what its name says)."""
    run_render_case(name)


def test_render_ray_in_a_face_plane_is_flagged_not_judged():
    """R3: the box whose face x = 0 holds the view axis.  The centre column is all edge: those pixels are only required to be
    flagged (this case has no leave-out cap), every other pixel is judged as usual."""
    got, r = run_render_case("r3_face_plane")
    col = np.arange(fd.H0) * fd.W0 + fd.W0 // 2
    flagged = r["leave_out"][0, col].numpy()
    assert flagged.sum() >= 7 and flagged[got[0, col] >= 0].all()  # whichever way the device decides them


def test_render_without_any_primitive_is_empty():
    """R6: M1 = M2 = 0 and NULL primitive pointers: every pixel is -1."""
    got, _ = run_render_case("r6_nothing")
    assert (got == -1).all()


def test_render_camera_inside_a_primitive_or_a_sphere_sees_past_it():
    """R9: a cuboid, a cylinder along and across the view and a robot sphere that contain the camera are invisible: every
    pixel shows the plate behind, at its own depth."""
    got, r = run_render_case("r9_inside")
    assert (got >= 0).all() and r["left_out"] == 0
    fx, fy, cx, cy = fd.CRAFTED
    u, v = np.meshgrid(np.arange(fd.W0), np.arange(fd.H0))
    want = (3.0 * np.sqrt(1 + ((u + 0.5 - cx) / fx) ** 2 + ((v + 0.5 - cy) / fy) ** 2)).reshape(-1)
    assert np.abs(got - want[None]).max() <= 4 * r["e32"]


def test_render_overlapping_primitives_nearest_wins():
    """R10: the same primitives in another order within their lists give the same bits."""
    got, _ = run_render_case("r10_overlap")
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))


# ---------------------------------------------------------------- select
def launch_select(depth, poses, intr, W, H, n_out, seed, env_offset=0, stride=3, batch_stride=None):
    """-> (out [B,batch_stride] on the host, NaN where nothing was written; count [B])."""
    from mpinets_amd import _lib

    B = depth.shape[0]
    batch_stride = n_out * stride if batch_stride is None else batch_stride
    assert batch_stride >= (n_out - 1) * stride + 3 and depth.shape[1] == W * H
    out = torch.full((B, batch_stride), float("nan"), device=DEV)
    count = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    fx, fy, cx, cy = intr
    depth_d, poses_d = dev(depth), dev(poses)  # (held until the call has finished)
    _lib.call("mpx_depth_select", depth_d.data_ptr(), poses_d.data_ptr(), fx, fy, cx, cy, W, H, B, n_out, seed,
              env_offset, out.data_ptr(), batch_stride, stride, count.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), count.cpu().numpy()


def judge_select(name, out, count, depth, poses, intr, W, H, n_out, seed, env_offset=0, stride=3):
    """count is exact, short rows keep their sentinel, full rows hold the restatement's pixels in its order: each point
    within 4 e32 of the float64 back-projection, and nothing but the triples is written."""
    want_count, rows = fd.select_pixels(depth, n_out, seed, env_offset)
    assert np.array_equal(count, want_count), (name, count, want_count)
    worst, e32_all = 0.0, 0.0
    for b, pix in enumerate(rows):
        if pix is None:
            assert np.isnan(out[b]).all(), (name, b)
            continue
        args = (depth[b:b + 1], poses[b:b + 1], intr, W, H, pix[None])
        want = fd.back_project(*args)[0].numpy()
        e32 = float(np.abs(fd.back_project(*args, dtype=torch.float32)[0].double().numpy() - want).max())
        written = np.zeros(out.shape[1], bool)
        at = (np.arange(n_out) * stride)[:, None] + np.arange(3)[None, :]
        written[at.reshape(-1)] = True
        assert np.isnan(out[b][~written]).all() and np.isfinite(out[b][written]).all(), (name, b)
        err = float(np.abs(out[b][at] - want).max())
        assert err <= 4 * e32, (name, b, err, e32)
        worst, e32_all = max(worst, err), max(e32_all, e32)
    figure(name, f"W={W} H={H} n_out={n_out} counts={count.tolist()} e32={e32_all:.3g} atol={4 * e32_all:.3g} "
                 f"gpu_err={worst:.3g}")
    return rows


def test_select_on_rendered_depths_equals_oracle(oracle):
    """S1: the R1 depths, n_out = 64: the subset and its order are oracle.depth_select's, the points the back-projection."""
    c = fd.cases()["r1_scenes"]
    depth = launch_render(c, device_scene(c["scn"])[0], None)
    out, count = launch_select(depth, c["poses"], c["intr"], 64, 48, 64, 77)
    rows = judge_select("s1", out, count, depth, c["poses"], c["intr"], 64, 48, 64, 77)
    opts, ocount = oracle.depth_select(depth, c["poses"], c["intr"], 64, 48, 64, 77)
    assert np.array_equal(count, ocount) and all(r is not None for r in rows)
    # the hit points of distinct pixels are centimetres apart: equal points to 2e-6 are equal pixels in equal order
    assert np.abs(out.reshape(3, 64, 3) - opts).max() <= 2e-6


@pytest.mark.parametrize("W,H,n_out", [(5, 3, 1), (33, 17, 100), (64, 64, 4096)])
def test_select_population_edges(W, H, n_out):
    """S2: rows with exactly n_out, n_out - 1, 0 and 2 n_out (or all) valid pixels in one call.  With n_out = 4096 on 64 x 64
    every pixel of the full rows is valid and the n_out-th key is the largest."""
    counts = (n_out, n_out - 1, 0, min(2 * n_out, W * H))
    depth = fd.populations(W, H, counts, 3)
    poses, intr = fd.tilted_poses(4, 2), fd.intrinsics(W, H)
    out, count = launch_select(depth, poses, intr, W, H, n_out, 2024)
    rows = judge_select(f"s2_n{n_out}", out, count, depth, poses, intr, W, H, n_out, 2024)
    assert count.tolist() == list(counts) and [r is None for r in rows] == [False, True, True, False]
    assert sorted(rows[0].tolist()) == np.flatnonzero(depth[0] >= 0).tolist()  # exactly n_out valid: all of them


@pytest.mark.parametrize("W,H,n_out,valid", [(4099, 1, 3, (4096, 4097, 4098)), (4099, 1, 2, (4096, 4098)), (3, 1, 2, (0, 2)),
                                             (3, 1, 3, (0, 1, 2)), (1, 1, 1, (0,)), (33, 17, 7, tuple(range(553, 561)))])
def test_select_ragged_images(W, H, n_out, valid):
    """S3: pixel counts that are no multiple of 4, the only valid pixels in the last, partial group of four; images of fewer
    than four pixels.  Row 1 is the same image with its first pixel valid too."""
    depth = np.full((2, W * H), -1.0, np.float32)
    depth[:, list(valid)] = 1.0 + 0.001 * np.arange(len(valid), dtype=np.float32)
    depth[1, 0] = 2.0
    poses, intr = fd.tilted_poses(2, 3), fd.intrinsics(W, H)
    out, count = launch_select(depth, poses, intr, W, H, n_out, 5)
    rows = judge_select(f"s3_{W}x{H}_n{n_out}", out, count, depth, poses, intr, W, H, n_out, 5)
    assert count[0] == len(valid) and set(rows[0].tolist()) <= set(valid)


def test_select_pixel_values():
    """S4: 0.0 and -0.0 are valid, -1 and NaN are not; a depth of zero is the camera's own origin."""
    W, H, n_out = 33, 17, 40
    depth = np.full((2, W * H), -1.0, np.float32)
    rng = np.random.default_rng(9)
    where = rng.permutation(W * H)[:80]
    depth[0, where[:20]], depth[0, where[20:40]], depth[0, where[40:60]] = 0.0, -0.0, float("nan")
    depth[1] = float("nan")
    depth[1, where[:25]], depth[1, where[25:50]] = -0.0, 1.5
    poses, intr = fd.tilted_poses(2, 4), fd.intrinsics(W, H)
    out, count = launch_select(depth, poses, intr, W, H, n_out, 11)
    rows = judge_select("s4", out, count, depth, poses, intr, W, H, n_out, 11)
    assert count.tolist() == [40, 50] and sorted(rows[0].tolist()) == sorted(where[:40].tolist())
    assert np.array_equal(out[0].reshape(n_out, 3), np.repeat(poses[0, :3, 3][None], n_out, 0))


@pytest.mark.parametrize("stride,extra", [(4, 0), (7, 0), (3, 11), (7, 5)])
def test_select_output_strides(stride, extra):
    """S5: point strides 4 and 7, a batch stride larger than n_out * stride: the triples are the bits of the packed call and
    every other float keeps its sentinel (judge_select)."""
    W, H, n_out = 33, 17, 100
    depth = fd.populations(W, H, (300, 99, 561), 6)
    poses, intr = fd.tilted_poses(3, 5), fd.intrinsics(W, H)
    packed, count0 = launch_select(depth, poses, intr, W, H, n_out, 31)
    out, count = launch_select(depth, poses, intr, W, H, n_out, 31, stride=stride, batch_stride=n_out * stride + extra)
    judge_select(f"s5_stride{stride}_extra{extra}", out, count, depth, poses, intr, W, H, n_out, 31, stride=stride)
    assert np.array_equal(count, count0)
    at = (np.arange(n_out) * stride)[:, None] + np.arange(3)[None, :]
    for b in (0, 2):
        assert np.array_equal(out[b][at].view(np.int32), packed[b].reshape(n_out, 3).view(np.int32))


@pytest.mark.parametrize("offset", [5, 0xFFFFFFFF - 3])
def test_select_env_offset(offset):
    """S6: a B = 3 call at offset e equals three B = 1 calls at e, e + 1, e + 2, up to the last offset the entry accepts."""
    W, H, n_out = 33, 17, 100
    depth = np.repeat(fd.populations(W, H, (400,), 8), 3, 0)  # the same image three times: only the environment id differs
    poses, intr = np.repeat(fd.tilted_poses(1, 6), 3, 0), fd.intrinsics(W, H)
    out, count = launch_select(depth, poses, intr, W, H, n_out, 99, env_offset=offset)
    rows = judge_select(f"s6_offset{offset}", out, count, depth, poses, intr, W, H, n_out, 99, env_offset=offset)
    assert rows[0].tolist() != rows[1].tolist() != rows[2].tolist()
    for b in range(3):
        one, n = launch_select(depth[b:b + 1], poses[b:b + 1], intr, W, H, n_out, 99, env_offset=offset + b)
        assert n[0] == count[b] and np.array_equal(one[0].view(np.int32), out[b].view(np.int32))
