"""GPU: ``mpx_cloud_field_build`` and ``mpx_cloud_field_sample`` (csrc/cloud_field.hip) against their restatement
(tests/float64_cloud_field.py), at the shapes where the build takes another path (empty, one point, around one tile,
several tiles; one brick, partial bricks on every axis) and on the device's own field for the sampler."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float64_cloud_field as fcf  # noqa: E402
from test_cloud_field_host import SAMPLE_DIST_REFERENCE, SAMPLE_GRAD_REFERENCE  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 12345.0


def dev():
    return torch.device("cuda:0")


def c_grid(grid):
    from mpinets_amd import _lib

    return _lib.FieldGrid((ctypes.c_float * 3)(*[float(v) for v in grid["lo"]]), float(grid["h"]), grid["nx"], grid["ny"],
                          grid["nz"], float(grid["trunc"]))


def device_build(cloud, counts, grid, slab=False, guarded=True):
    """-> field float32 numpy [B,nz,ny,nx]; with ``slab`` the cloud is passed as the [B,6272,4][:, 2048:2048+N, :3] view;
    guard words in front of and behind the field must keep their fill."""
    from mpinets_amd.field import CloudField

    torch.cuda.set_device(0)
    B, N = cloud.shape[:2]
    if slab:
        whole = torch.full((B, 6272, 4), 7.0, dtype=torch.float32, device=dev())  # (7 m: inside no test grid's reach)
        whole[:, 2048:2048 + N, :3] = torch.from_numpy(cloud).to(dev())
        view = whole[:, 2048:2048 + N, :3]
    else:
        view = torch.from_numpy(cloud).to(dev())
    cn = None if counts is None else torch.from_numpy(counts).to(dev())
    nodes = grid["nz"] * grid["ny"] * grid["nx"]
    buf = torch.full((B * nodes + 128,), GUARD, dtype=torch.float32, device=dev())
    out = buf[64:64 + B * nodes].view(B, grid["nz"], grid["ny"], grid["nx"])
    f = CloudField.build(view, cn, grid=c_grid(grid), out=out)
    assert f.values.data_ptr() == out.data_ptr()
    assert bool((buf[:64] == GUARD).all()) and bool((buf[64 + B * nodes:] == GUARD).all())
    return f


@pytest.mark.parametrize("case", fcf.BUILD_CASES, ids=fcf.case_id)
def test_build_against_float64(case):
    """Every node: inside the band of the float64 minimum below trunc, exactly trunc above it, either in between; an
    environment without a usable row is trunc everywhere; guard words untouched; a second build is bit-equal."""
    cloud, counts, grid = fcf.make_build_case(case)
    B, N, g, tr, extras = case
    f = device_build(cloud, counts, grid, slab="slab" in extras)
    field = f.values.cpu().numpy()
    d2 = fcf.build_restate(cloud, counts, grid)
    below, above, mid = fcf.check_field(field, d2, grid["trunc"])
    print(f"{fcf.case_id(case)}: {below} nodes below trunc, {above} above, {mid} in the band")
    if N == 0 or "empty" in extras:
        assert (field[0] == grid["trunc"]).all()
    again = device_build(cloud, counts, grid, slab="slab" in extras).values.cpu().numpy()
    assert np.array_equal(field.view(np.uint32), again.view(np.uint32))


def test_build_exact_cases():
    grid = fcf.make_grid((9, 8, 5), trunc=10.0)
    x, y, z = fcf.node_coordinates(grid)
    cloud = np.array([[[x[3], y[7], z[4]], [x[8], y[0], z[0]]]], np.float32)
    field = device_build(cloud, None, grid).values.cpu().numpy()
    assert field[0, 4, 7, 3] == 0.0 and field[0, 0, 0, 8] == 0.0 and (field > 0).sum() == field.size - 2
    s = np.float32(2.0 ** -5)
    p = np.array([[[x[2] + 3 * s, y[3] - 4 * s, z[1]]]], np.float32)
    field = device_build(p, None, grid).values.cpu().numpy()
    assert field[0, 1, 3, 2] == np.float32(5 * s)


def test_build_does_not_depend_on_the_batch_it_is_launched_in():
    """Environment b of a batch of 3 equals the same cloud built alone (another grid of workgroups, another launch)."""
    case = fcf.BUILD_CASES[6]
    cloud, counts, grid = fcf.make_build_case(case)
    whole = device_build(cloud, counts, grid).values.cpu().numpy()
    for b in range(cloud.shape[0]):
        alone = device_build(cloud[b:b + 1], counts[b:b + 1], grid).values.cpu().numpy()
        assert np.array_equal(whole[b].view(np.uint32), alone[0].view(np.uint32))


@pytest.fixture(scope="module")
def sampled():
    grid, cloud, pts = fcf.make_sample_case()
    f = device_build(cloud, None, grid)
    p = torch.from_numpy(pts).to(dev())
    dist, grad = f.sample(p, return_grad=True)
    only = f.sample(p)
    return grid, f, pts, dist.cpu().numpy(), grad.cpu().numpy(), only.cpu().numpy()


def test_samples_on_nodes_return_the_node_values(sampled):
    grid, f, pts, dist, grad, only = sampled
    field = f.values.cpu().numpy()
    x, y, z = fcf.node_coordinates(grid)
    Z, Y, X = np.meshgrid(z[:-1], y[:-1], x[:-1], indexing="ij")
    nodes = np.ascontiguousarray(np.broadcast_to(np.stack([X, Y, Z], -1).reshape(1, -1, 3), (field.shape[0], X.size, 3))).astype(np.float32)
    d = f.sample(torch.from_numpy(nodes).to(dev())).cpu().numpy().reshape(field.shape[0], *X.shape)
    assert np.array_equal(d.view(np.uint32), field[:, :-1, :-1, :-1].view(np.uint32))


def test_samples_outside_nan_and_on_the_last_node(sampled):
    grid, f, pts, dist, grad, only = sampled
    field = f.values.cpu().numpy()
    trunc = np.float32(grid["trunc"])
    assert np.array_equal(dist.view(np.uint32), only.view(np.uint32))  # with and without the gradient: the same value
    _, _, inside = fcf.sample(field, grid, pts, torch.float32)
    inside = inside.numpy()
    assert (dist[~inside] == trunc).all() and (grad[~inside] == 0).all()
    for row in (0, 1, 4):  # NaN, infinite, far away
        assert (dist[:, row] == trunc).all() and (grad[:, row] == 0).all()
    # u == n - 1 on every axis (row 2) and on x alone (row 3): inside, the value of the last node to the two roundings of fx = 1
    assert np.abs(dist[:, 2] - field[:, -1, -1, -1]).max() <= 4 * SAMPLE_DIST_REFERENCE
    assert np.abs(dist[:, 3] - field[:, 0, 0, -1]).max() <= 4 * SAMPLE_DIST_REFERENCE
    assert (dist[:, 3] != trunc).any() or (field[:, 0, 0, -1] == trunc).all()


def test_interior_samples_against_float64(sampled):
    """On the device's own field: dist within 4 x SAMPLE_DIST_REFERENCE and grad within 4 x SAMPLE_GRAD_REFERENCE of the
    float64 restatement (tests/test_cloud_field_host.py records both: 5.9e-8 m and 1.2e-6), samples within 1e-5 cells of
    a cell face left out of the gradient comparison (at most 1 %)."""
    grid, f, pts, dist, grad, only = sampled
    field = f.values.cpu().numpy()
    d64, g64, inside, near = fcf.sample(field, grid, pts, torch.float64, want_face=True)
    inside, near = inside.numpy(), near.numpy()
    dd = np.abs(dist.astype(np.float64) - d64.numpy())[inside].max()
    dg = np.abs(grad.astype(np.float64) - g64.numpy()).max(-1)[inside & ~near].max()
    print(f"sampler against float64: dist {dd:.3e} m (bar {4 * SAMPLE_DIST_REFERENCE:.2e}), grad {dg:.3e} "
          f"(bar {4 * SAMPLE_GRAD_REFERENCE:.2e}), near a face {near.mean():.5f}, inside {inside.mean():.3f}")
    assert near.mean() <= fcf.FACE_CAP
    assert inside.mean() > 0.3
    assert dd <= 4 * SAMPLE_DIST_REFERENCE
    assert dg <= 4 * SAMPLE_GRAD_REFERENCE


def test_sample_reads_strided_points_and_large_batches_of_points():
    """A [B,P,4] view (point stride 4) gives what the packed points give; P past one workgroup."""
    grid, cloud, pts = fcf.make_sample_case()
    f = device_build(cloud, None, grid)
    wide = torch.zeros((pts.shape[0], pts.shape[1], 4), dtype=torch.float32, device=dev())
    wide[..., :3] = torch.from_numpy(pts).to(dev())
    a, ga = f.sample(wide[..., :3], return_grad=True)
    b, gb = f.sample(torch.from_numpy(pts).to(dev()), return_grad=True)
    assert torch.equal(a, b) and torch.equal(ga, gb)
