"""GPU: ``mpx_franka_cloud_collision`` (csrc/cloud_collision.hip) against its float64 restatement, its exact properties
device against device, ties and non-finite points, one-way consistency with the primitive check, and the evaluator /
rollout methods built on it.

Bands (tests/float64_cloud_collision.py): the device's squared distance is within ``BAND = 4 * 2^-24`` relative of the
float64 one (three roundings of ``mpx_sqdist`` on non-negative terms), so
  * flags must agree on every environment the restatement decides, and at most 2 % of a case's environments may be
    undecided (tests/test_cloud_collision_host.py shows the restatement alone gives 0);
  * ``nearest`` must be a point whose float64 d2 is within BAND of the minimum;
  * ``min_dist`` is checked as a DISTANCE: the entry point returns ``sqrtf(best) - point_radius``, not ``best``.  A band
    of BAND on ``best`` is BAND / 2 on its square root; ``sqrtf`` and the subtraction each add half an ulp (2^-24
    relative) of their own results.  Hence ``|min_dist + point_radius - sqrt(d2_min)| <= (BAND / 2 + 2^-24) sqrt(d2_min) +
    2^-24 |sqrt(d2_min) - point_radius|`` plus the float64 noise of this very expression.
"""
import functools

import numpy as np
import pytest
import torch

import float64_cloud_collision as f64
from mpinets_amd import _lib, scenes
from mpinets_amd import franka_tables as ft
from mpinets_amd.robot import FrankaCollisionSampler

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP = 2.0 ** -24
VARIANT_CLOUD_CULL = 3  # MPX_VARIANT_CLOUD_CULL


@functools.lru_cache(maxsize=None)
def sampler(with_base_link=False):
    return FrankaCollisionSampler(DEV, with_base_link=with_base_link)


def three_forms(s, q, cloud, **kw):
    """-> (flags, min_dist, nearest) of the full form, flags of the flags-only form with the cull, and without it."""
    full = s.check_cloud(q, cloud, return_distance=True, return_nearest=True, **kw)
    culled = s.check_cloud(q, cloud, **kw)
    lib = _lib.load()
    assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 0) == 0
    try:
        plain = s.check_cloud(q, cloud, **kw)
    finally:
        assert lib.mpx_set_variant(VARIANT_CLOUD_CULL, 1) == 0
    return full, culled, plain


@functools.lru_cache(maxsize=None)
def run_case(case):
    """One device run of every form plus the restatement, shared by the tests below (inputs and results are not modified)."""
    B, T, base, N, pr, cl = case
    qn, cn = f64.make_case(case)
    s = sampler(base)
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    full, culled, plain = three_forms(s, q, cloud, point_radius=pr, clearance=cl)
    centres = s.sphere_centers(q.reshape(B * T, 7)).reshape(B, T, -1, 3).cpu().numpy()
    ref = f64.restate(centres, cn, s.radii.cpu().numpy(), pr, cl)
    torch.cuda.synchronize()
    return full, culled, plain, ref


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_device_against_float64(case):
    B, T, base, N, pr, cl = case
    (flags, dist, near), _, _, ref = run_case(case)
    flags, dist, near = flags.cpu().numpy(), dist.cpu().numpy().astype(np.float64), near.cpu().numpy()
    decided = ~ref["env_undecided"]
    share = 1.0 - decided.mean()
    root = np.sqrt(ref["d2_min"])
    err = np.abs(dist + pr - root)
    bound = (f64.BAND / 2 + ULP) * root + ULP * np.abs(root - pr) + 1e-12
    print(f"{f64.case_id(case)}: hits {int(ref['env_hit'].sum())}/{B}, undecided {int((~decided).sum())}, "
          f"max dist err / bound {float((err / bound).max()):.3f}")
    assert share <= f64.UNDECIDED_CAP
    assert (flags[decided] == ref["env_hit"][decided]).all()
    assert np.isfinite(root).all() and (err <= bound).all()
    for b in range(B):
        assert ref["in_band"](b, near[b]).all()


@pytest.mark.parametrize("case", f64.CASES, ids=f64.case_id)
def test_flags_only_forms_equal_the_full_form(case):
    (flags, _, _), culled, plain, _ = run_case(case)
    assert torch.equal(culled, flags) and torch.equal(plain, flags)


def _hitting_points(s, q):
    """[B,S,3]: the sphere centres of every environment's first waypoint -- points that certainly hit."""
    return s.sphere_centers(q[:, 0].contiguous())


def test_every_environment_in_collision():
    B, T, N = 5, 50, 300
    qn, cn = f64.make_case((B, T, False, N, 0.0, 0.0), seed=21)
    s = sampler()
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    cloud[:, 280:280 + 4] = _hitting_points(s, q)[:, :4]  # in the second tile
    (flags, dist, near), culled, plain = three_forms(s, q, cloud)
    assert flags.all() and torch.equal(culled, flags) and torch.equal(plain, flags)
    assert (dist[:, 0, :4] == 0).all() and torch.equal(near[:, 0, :4], torch.arange(280, 284, device=DEV, dtype=torch.int32).expand(B, 4))


def test_slab_view_equals_a_contiguous_copy():
    B, T = 3, 50
    qn, cn = f64.make_case((B, T, False, 4096, 0.0, 0.0), seed=22)
    s = sampler()
    q = torch.from_numpy(qn).to(DEV)
    xyz = torch.empty((B, 6272, 4), device=DEV)
    xyz[..., 3] = torch.rand((B, 6272), device=DEV) * 3 - 1  # other data in the label column
    # neighbouring rows: points that WOULD hit (a kernel that strays outside the scene rows changes its answer)
    hit = _hitting_points(s, q)
    xyz[:, :2048, :3] = hit[:, torch.arange(2048, device=DEV) % s.num_spheres]
    xyz[:, 6144:, :3] = hit[:, torch.arange(128, device=DEV) % s.num_spheres]
    # scene rows: the case's cloud
    xyz[:, 2048:6144, :3] = torch.from_numpy(cn).to(DEV)
    view = xyz[:, 2048:6144, :3]
    assert not view.is_contiguous() and view.stride() == (6272 * 4, 4, 1)
    a = three_forms(s, q, view, point_radius=0.0)
    b = three_forms(s, q, view.contiguous(), point_radius=0.0)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[1], a[0][0]) and torch.equal(a[2], a[0][0])
    # and a sparse scene (first 40 rows real, the rest far away) whose flags are not all set
    far = view.clone()
    far[:, 40:] = 50.0
    xyz[:, 2048:6144, :3] = far
    c, d = three_forms(s, q, view), three_forms(s, q, far)
    assert torch.equal(c[0][0], d[0][0]) and torch.equal(c[0][1], d[0][1]) and torch.equal(c[0][2], d[0][2])
    assert torch.equal(c[1], d[1]) and torch.equal(c[2], d[2]) and torch.equal(c[1], c[0][0])
    assert (c[0][2] < 40).all()


def test_trajectory_equals_its_waypoints_one_by_one():
    B, T, N = 3, 50, 300
    qn, cn = f64.make_case((B, T, True, N, 0.01, 0.005), seed=23)
    s = sampler(True)
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    kw = dict(point_radius=0.01, clearance=0.005)
    (flags, dist, near), culled, plain = three_forms(s, q, cloud, **kw)
    each = cloud.repeat_interleave(T, dim=0)
    (f1, d1, n1), c1, p1 = three_forms(s, q.reshape(B * T, 1, 7), each, **kw)
    assert torch.equal(f1.view(B, T).any(dim=1), flags)
    assert torch.equal(c1, f1) and torch.equal(p1, f1)
    assert torch.equal(d1.view(B, T, -1), dist) and torch.equal(n1.view(B, T, -1), near)
    # [B,7] is [B,1,7]
    g = s.check_cloud(q[:, 0], cloud, return_distance=True, **kw)
    assert torch.equal(g[1], dist[:, :1]) and g[1].shape == (B, 1, 57)


@pytest.mark.parametrize("N", [65, 300])
def test_counts_equal_a_truncated_cloud(N):
    B, T = 4, 10
    qn, cn = f64.make_case((B, T, False, N, 0.0, 0.0), seed=24)
    s = sampler()
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    hit = _hitting_points(s, q)
    for k in (0, 1, N - 1, N):
        padded = cloud.clone()
        padded[:, k:] = hit[:, torch.arange(N - k, device=DEV) % s.num_spheres]  # rows past k would hit
        counts = torch.full((B,), k, dtype=torch.int32, device=DEV)
        a, b = three_forms(s, q, padded, counts=counts), three_forms(s, q, cloud[:, :k])
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y), k
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[1], a[0][0]) and torch.equal(a[2], a[0][0])
        if k == 0:
            assert not a[0][0].any() and torch.isinf(a[0][1]).all() and (a[0][1] > 0).all() and (a[0][2] == -1).all()
    # a different count per environment (int64 counts are accepted), counts above N mean N
    ks = [0, 1, N - 1, N + 7]
    padded = cloud.clone()
    for b, k in enumerate(ks):
        padded[b, k:] = hit[b, torch.arange(max(N - k, 0), device=DEV) % s.num_spheres]
    a = three_forms(s, q, padded, counts=torch.tensor(ks, device=DEV))
    for b, k in enumerate(ks):
        one = three_forms(s, q[b:b + 1], cloud[b:b + 1, :min(k, N)])
        for x, y in zip(a[0], one[0]):
            assert torch.equal(x[b:b + 1], y), (b, k)
        assert torch.equal(a[1][b:b + 1], one[1]) and torch.equal(a[2][b:b + 1], one[2])


def test_ties_go_to_the_lower_index():
    B, T, N = 3, 10, 200
    qn, cn = f64.make_case((B, T, False, N, 0.0, 0.0), seed=25)
    s = sampler()
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    _, dist, near = s.check_cloud(q, cloud, return_distance=True, return_nearest=True)
    # every point again N rows later (another tile), and every point twice in a row (the same tile)
    _, d2, n2 = s.check_cloud(q, torch.cat([cloud, cloud], dim=1), return_distance=True, return_nearest=True)
    assert torch.equal(n2, near) and torch.equal(d2, dist)
    _, d3, n3 = s.check_cloud(q, cloud.repeat_interleave(2, dim=1), return_distance=True, return_nearest=True)
    assert torch.equal(n3, 2 * near) and torch.equal(d3, dist)
    # one point duplicated at two indices: some sphere's nearest point copied to the LAST row of its environment
    t, k = [int(v[0]) for v in torch.nonzero(near[0] < N - 1, as_tuple=True)]
    j = int(near[0, t, k])
    dup = cloud.clone()
    dup[0, N - 1] = dup[0, j]
    _, d4, n4 = s.check_cloud(q, dup, return_distance=True, return_nearest=True)
    assert int(n4[0, t, k]) == j and d4[0, t, k] == dist[0, t, k]


def test_non_finite_points_equal_their_deletion():
    B, T, N = 3, 10, 300
    qn, cn = f64.make_case((B, T, False, N, 0.0, 0.0), seed=26)
    s = sampler()
    q, cloud = torch.from_numpy(qn).to(DEV), torch.from_numpy(cn).to(DEV)
    rng = np.random.default_rng(26)
    rows = np.sort(rng.choice(N, 45, replace=False))
    bad = cloud.clone()
    for i, r in enumerate(rows):
        bad[:, r, i % 3] = (float("nan"), float("inf"), float("-inf"))[(i // 3) % 3]
    bad[:, rows[0]] = float("nan")  # a row with every coordinate NaN
    keep = np.ones(N, bool)
    keep[rows] = False
    clean = cloud[:, torch.from_numpy(keep).to(DEV)]
    renumber = torch.from_numpy(np.cumsum(keep) - 1).to(DEV)
    for kw in (dict(), dict(point_radius=0.01, clearance=0.005)):
        a, b = three_forms(s, q, bad, **kw), three_forms(s, q, clean, **kw)
        assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1])
        assert torch.from_numpy(keep).to(DEV)[a[0][2].long()].all()  # never a deleted row
        assert torch.equal(renumber[a[0][2].long()].int(), b[0][2])
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[1], a[0][0])
    # an environment whose every point is NaN
    bad[1] = float("nan")
    (flags, dist, near), culled, plain = three_forms(s, q, bad)
    assert not flags[1] and not culled[1] and not plain[1]
    assert torch.isinf(dist[1]).all() and (dist[1] > 0).all() and (near[1] == -1).all()


def test_cloud_hit_implies_primitive_hit():
    """Scene clouds drawn ON the primitives' surfaces (yaw-only scenes: orthonormal frames): a sphere that reaches a surface
    point reaches the surface, so ``d(centre, point) <= r`` implies ``sdf(centre) <= r`` up to the engine's fp32 parity bar."""
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders

    B, T = 48, 50
    scn = {k: torch.from_numpy(v).to(DEV) for k, v in scenes.make_scenes(B, 3, kinds=("tabletop", "cubby", "dresser"), M1=40, M2=16).items()}
    cloud = scenes.sample_scene_clouds(scn, 4096, seed=3)
    q = torch.from_numpy(scenes.linear_trajectories(B, T, 31)).to(DEV)
    s = sampler()
    cub = TorchCuboids(scn["cuboid_centers"], scn["cuboid_dims"], scn["cuboid_quats"])
    cyl = TorchCylinders(scn["cylinder_centers"], scn["cylinder_radii"], scn["cylinder_heights"], scn["cylinder_quats"])
    (flags, dist, near), culled, plain = three_forms(s, q, cloud)
    has, msdf = s.check(q, cub, cyl, return_sdf=True)
    assert torch.equal(culled, flags) and torch.equal(plain, flags)
    pair_hit = dist <= s.radii[None, None, :]
    print(f"cloud hits {int(flags.sum())}/{B}, primitive hits {int(has.sum())}/{B}, hit pairs {int(pair_hit.sum())}")
    assert 0 < int(flags.sum())
    assert (msdf[pair_hit] <= s.radii[None, None, :].expand_as(msdf)[pair_hit] + 1e-5).all()
    assert ((msdf - s.radii[None, None, :]).amin(dim=(1, 2))[flags] <= 1e-5).all()


def test_evaluator_without_and_with_a_cloud():
    from mpinets_amd.geometry import TorchCuboids, TorchCylinders
    from mpinets_amd.metrics import BatchedEvaluator
    from mpinets_amd.robot import frames_to_matrix, franka_fk

    B, T = 16, 20
    scn = {k: torch.from_numpy(v).to(DEV) for k, v in scenes.make_scenes(B, 4).items()}
    cub = TorchCuboids(scn["cuboid_centers"], scn["cuboid_dims"], scn["cuboid_quats"])
    cyl = TorchCylinders(scn["cylinder_centers"], scn["cylinder_radii"], scn["cylinder_heights"], scn["cylinder_quats"])
    traj = torch.from_numpy(scenes.linear_trajectories(B, T, 41)).to(DEV)
    lengths = torch.randint(1, T + 1, (B,), device=DEV, dtype=torch.int32)
    lengths[0], lengths[1] = 1, T
    targets = frames_to_matrix(franka_fk(traj[:, -1].contiguous())[:, ft.LINK_ID["right_gripper"]])
    ev = BatchedEvaluator(DEV)
    for ln in (None, lengths):
        res = ev.evaluate_trajectories(traj, targets, lengths=ln, cuboids=cub, cylinders=cyl)
        # recomputed through check and mpx_trajectory_metrics directly
        f = lambda: torch.empty(B, dtype=torch.float32, device=DEV)
        i = lambda: torch.zeros(B, dtype=torch.int32, device=DEV)
        pos, ori, pp, po, jl, sc = f(), f(), f(), f(), i(), i()
        _lib.call("mpx_trajectory_metrics", _lib.ptr(traj), _lib.ptr(ln), _lib.ptr(targets), _lib.ptr(ev.limits), B, T,
                  ev.finger, _lib.ptr(pos), _lib.ptr(ori), _lib.ptr(pp), _lib.ptr(po), _lib.ptr(jl), _lib.ptr(sc))
        frozen = traj
        if ln is not None:
            t_idx = torch.minimum(torch.arange(T, device=DEV)[None, :], (ln.long() - 1)[:, None])
            frozen = torch.gather(traj, 1, t_idx[:, :, None].expand(-1, -1, 7)).contiguous()
        coll = ev.collision_sampler.check(frozen, cub, cyl)
        viol = coll | (jl != 0) | (sc != 0)
        want = {"position_error": pos, "orientation_error": ori, "eff_position_path_length": pp,
                "eff_orientation_path_length": po, "joint_limit_violation": jl != 0, "self_collision": sc != 0,
                "collision": coll, "physical_violations": viol, "correct_final_region": torch.ones(B, dtype=torch.bool, device=DEV),
                "success": (pos < 1) & (ori < 15) & ~viol,
                "num_steps": ln if ln is not None else torch.full((B,), T, dtype=torch.int32, device=DEV)}
        assert list(res) == list(want)
        for k in want:
            assert res[k].dtype == want[k].dtype and torch.equal(res[k], want[k]), k
        # with a cloud: the OR of both checks, on the frozen trajectory; primitives may be absent
        cloud = scenes.sample_scene_clouds(scn, 1024, seed=4)
        cloud[:, 1000:] = ev.collision_sampler.sphere_centers(traj[:, -1].contiguous())[:, :24]  # hit only by the LAST waypoint
        rc = ev.evaluate_trajectories(traj, targets, lengths=ln, cuboids=cub, cylinders=cyl, scene_cloud=cloud,
                                      cloud_point_radius=0.005)
        cc = ev.collision_sampler.check_cloud(frozen, cloud, point_radius=0.005)
        assert list(rc) == list(want) + ["cloud_collision"]
        assert torch.equal(rc["cloud_collision"], cc) and torch.equal(rc["collision"], coll | cc)
        assert torch.equal(rc["physical_violations"], coll | cc | (jl != 0) | (sc != 0))
        if ln is None:
            assert cc.all()
        only = ev.evaluate_trajectories(traj, targets, lengths=ln, scene_cloud=cloud, cloud_point_radius=0.005)
        assert torch.equal(only["collision"], cc) and torch.equal(only["cloud_collision"], cc)
        counts = torch.full((B,), 1000, dtype=torch.int32, device=DEV)
        rk = ev.evaluate_trajectories(traj, targets, lengths=ln, scene_cloud=cloud, scene_cloud_counts=counts)
        assert torch.equal(rk["cloud_collision"], ev.collision_sampler.check_cloud(frozen, cloud[:, :1000]))


def test_rollout_engine_checks_its_own_slab():
    from mpinets_amd.model import MotionPolicyNetwork
    from mpinets_amd.rollout import RolloutEngine

    torch.manual_seed(0)
    np.random.seed(0)
    B = 4
    prob = scenes.make_problem_batch(B, seed=0, device=DEV)
    mdl = MotionPolicyNetwork().to(DEV).eval()
    eng = RolloutEngine(mdl, prob)
    traj = eng.rollout(3)
    assert traj.shape == (B, 4, 7) and eng.xyz.shape[1:] == (6272, 4)
    got = eng.cloud_collision(traj, point_radius=0.01)
    rows = eng.xyz[:, 2048:6144, :3].clone()
    assert torch.equal(got, eng.collision.check_cloud(traj, rows, point_radius=0.01)) and got.shape == (B,)
    # a trajectory through the scene rows themselves certainly hits
    assert torch.equal(eng.cloud_collision(traj), eng.collision.check_cloud(traj, rows))


def test_argument_errors_launch_nothing():
    s = sampler()
    q = torch.zeros((2, 3, 7), device=DEV)
    cloud = s.sphere_centers(q[:, 0].contiguous()).contiguous()  # would hit
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    dist = torch.full((2, 3, s.num_spheres), -7.0, device=DEV)
    lib = _lib.load()

    def call(S=s.num_spheres, N=cloud.size(1), stride=3, pr=0.0, B=2):
        return lib.mpx_franka_cloud_collision(q.data_ptr(), B, 3, s.finger, s.centers.data_ptr(), s.radii.data_ptr(),
                                              s.links.data_ptr(), S, cloud.data_ptr(), cloud.stride(0), stride, N, None, pr, 0.0,
                                              flags.data_ptr(), dist.data_ptr(), None, _lib.stream_ptr())

    for kw, text in ((dict(S=65), b"64"), (dict(N=-1), b"negative"), (dict(B=-2), b"negative"), (dict(pr=-0.5), b"point_radius"),
                     (dict(stride=2), b"cloud_point_stride")):
        assert call(**kw) != 0 and text in lib.mpx_last_error(), kw
    torch.cuda.synchronize()
    assert not flags.any() and (dist == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert flags.all() and (dist[:, 0] == 0).all()
    with pytest.raises(_lib.MpxError):
        s.check_cloud(q, cloud.cpu())
    with pytest.raises(_lib.MpxError):
        s.check_cloud(q, cloud.double())
    with pytest.raises(_lib.MpxError):
        s.check_cloud(q, cloud.transpose(1, 2).contiguous().transpose(1, 2))  # last stride is not 1
