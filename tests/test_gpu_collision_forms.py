"""Every launch form of the primitive collision sweep (csrc/franka.hip, ``mpx_franka_collision``) against a float64
restatement (tests/float64_collision.py): the one-wave form, each pairs-per-thread instantiation of the 256-thread
per-environment kernel at both ends of its range, as a single chunk and with a ragged last chunk, and the general kernel
by sphere count, by primitive count and by frame alignment -- distances, flags, the flags-only shortcut, the OR into
the caller's buffer, and the decision boundary inside the 256-thread forms.

The reference works from the device's own sphere centres (``mpx_franka_spheres``) and inverse frames
(``TorchCuboids.inv_frames``), so what is left between it and the kernel is the sweep's arithmetic alone; the bar
(``SDF_BAR``) is the float32 run of the reference against its float64 run, never the kernel's own output.
tests/test_collision_host.py shows on the CPU that the cases reach every route and that the conditions below are
satisfiable."""
import numpy as np
import pytest
import torch

import float64_collision as fc

pytestmark = pytest.mark.gpu

_RUNS = {}


def dev():
    return torch.device("cuda:0")


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _shifted(t):
    """The same values one float further into a larger buffer: a pointer that is not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=t.device)
    out = buf[1:].view_as(t)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


class Run:
    """One case on the device: inputs, the full call, the flags-only call and the float64 reference, made once."""

    def __init__(self, case):
        from mpinets_amd import franka_tables as ft
        from mpinets_amd.geometry import TorchCuboids, TorchCylinders

        self.case, self.S = case, fc.num_spheres(case)
        q, scn, (c, r, l) = fc.make_case(case)
        self.q = D(q)
        self.centers, self.radii, self.links = D(c), D(r), D(l)
        self.finger = float(ft.FINGER_OPENING)
        self.cub = TorchCuboids(D(scn["cuboid_centers"]), D(scn["cuboid_dims"]), D(scn["cuboid_quats"]))
        self.cyl = TorchCylinders(D(scn["cylinder_centers"]), D(scn["cylinder_radii"]), D(scn["cylinder_heights"]),
                                  D(scn["cylinder_quats"]))
        self.cf, self.cd = self.cub.inv_frames, self.cub.dims.contiguous()
        self.yf, self.yr, self.yh = self.cyl.inv_frames, self.cyl.radii.contiguous(), self.cyl.heights.contiguous()
        assert self.cf.data_ptr() % 16 == 0 and self.yf.data_ptr() % 16 == 0
        self.flags, self.msdf = self.call(True)
        self.flags_only, _ = self.call(False)
        # the reference: float64, from the device's own centres and frames
        from mpinets_amd import _lib
        cen = torch.empty((case.B * case.T, self.S, 3), dtype=torch.float32, device=dev())
        _lib.call("mpx_franka_spheres", _lib.ptr(self.q), case.B * case.T, self.finger, _lib.ptr(self.centers),
                  _lib.ptr(self.links), self.S, _lib.ptr(cen))
        self.centres_np = cen.cpu().numpy().reshape(case.B, case.T, self.S, 3)
        self.ref64 = fc.restate(self.centres_np, self.cf.cpu().numpy(), self.cd.cpu().numpy(), self.yf.cpu().numpy(),
                                self.yr.cpu().numpy(), self.yh.cpu().numpy(), dtype=np.float64)
        self.hit, self.undecided = fc.decide(self.ref64, r)

    def call(self, want_sdf, radii=None, flags=None, env=None, cf=None, yf=None):
        """The raw entry point on the whole case or on environment ``env`` alone (same T and S: the same route)."""
        from mpinets_amd import _lib

        case = self.case
        sl = slice(None) if env is None else slice(env, env + 1)
        B = case.B if env is None else 1
        q = self.q[sl]
        cf = (self.cf if cf is None else cf)[sl]
        yf = (self.yf if yf is None else yf)[sl]
        radii = self.radii if radii is None else radii
        if flags is None:
            flags = torch.zeros(B, dtype=torch.int32, device=dev())
        msdf = torch.full((B, case.T, self.S), float("nan"), dtype=torch.float32, device=dev()) if want_sdf else None
        _lib.call("mpx_franka_collision", _lib.ptr(q), B, case.T, self.finger, _lib.ptr(self.centers), _lib.ptr(radii),
                  _lib.ptr(self.links), self.S, _lib.ptr(cf), _lib.ptr(self.cd[sl]), case.M1, _lib.ptr(yf), _lib.ptr(self.yr[sl]),
                  _lib.ptr(self.yh[sl]), case.M2, _lib.ptr(flags), _lib.ptr(msdf))
        return flags, msdf


def run_of(case):
    if case not in _RUNS:
        _RUNS[case] = Run(case)
    return _RUNS[case]


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_distances_within_the_bar_of_float64(case):
    """Every finite entry within SDF_BAR of the float64 restatement, the +inf pattern identical, nothing left unwritten."""
    r = run_of(case)
    got = r.msdf.cpu().numpy()
    bad, worst = fc.offending_envs(got, r.ref64)
    print(f"FORMS {fc.case_id(case)} route {fc.case_route(case)} worst {worst:.3e} bar {fc.SDF_BAR:.1e} ratio {worst / fc.SDF_BAR:.3f} "
          f"hit {int(r.hit.sum())} undecided {int(r.undecided.sum())} of {case.B}")
    assert not np.isnan(got).any()
    assert np.array_equal(np.isposinf(got), np.isposinf(r.ref64))
    assert bad == set(), (sorted(bad), worst)
    if case.table in ("S56", "S57"):  # the same call through the class
        from mpinets_amd.robot import FrankaCollisionSampler

        cs = FrankaCollisionSampler(dev(), with_base_link=case.table == "S57")
        has, msdf = cs.check(r.q, r.cub, r.cyl, return_sdf=True)
        assert torch.equal(msdf, r.msdf) and torch.equal(has, r.flags != 0)
        assert torch.equal(cs.sphere_centers(r.q.reshape(-1, 7)).reshape(r.centres_np.shape).cpu(), torch.from_numpy(r.centres_np))


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_flags_equal_the_float64_decision(case):
    r = run_of(case)
    keep = ~r.undecided
    assert r.undecided.mean() <= fc.UNDECIDED_CAP, int(r.undecided.sum())
    flags = r.flags.cpu().numpy()
    assert set(np.unique(flags).tolist()) <= {0, 1}
    assert np.array_equal(flags[keep] != 0, r.hit[keep])
    assert np.array_equal(r.flags_only.cpu().numpy()[keep] != 0, r.hit[keep])


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_flags_only_form_equals_the_full_form_exactly(case):
    """``min_sdf == NULL`` decides behind two bounds without the square root; the kernel claims the same flags as
    ``min_sdf <= radius`` from its own distances -- every environment, no band."""
    r = run_of(case)
    own = (r.msdf <= r.radii[None, None, :]).reshape(case.B, -1).any(dim=1).to(torch.int32)
    assert torch.equal(r.flags, own)
    assert torch.equal(r.flags_only, own)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_per_environment_kernel_equals_the_general_kernel_bit_for_bit(case):
    """The same case with both frame tables one float off alignment takes the general kernel: equal distances, equal
    flags, in both forms."""
    r = run_of(case)
    assert fc.case_route(case, aligned=False)[0] == "general"
    cf, yf = _shifted(r.cf), _shifted(r.yf)
    flags, msdf = r.call(True, cf=cf, yf=yf)
    flags_only, _ = r.call(False, cf=cf, yf=yf)
    same = float((msdf == r.msdf).float().mean())
    print(f"FORMS {fc.case_id(case)} route {fc.case_route(case)[0]} bit-equal share against the general kernel {same:.6f}")
    assert torch.equal(msdf, r.msdf)
    assert torch.equal(flags, r.flags) and torch.equal(flags_only, r.flags_only)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_flags_are_ored_into_the_callers_buffer(case):
    r = run_of(case)
    for want_sdf, mine in ((True, r.flags), (False, r.flags_only)):
        pre = torch.full((case.B,), 2, dtype=torch.int32, device=dev())
        pre[::2] = 1  # a flag that is already set stays set, another bit stays as it is
        expect = pre | mine
        got, _ = r.call(want_sdf, flags=pre.clone())
        assert torch.equal(got, expect)


def _owner(case, t, s):
    """(chunk, k): the waypoint chunk of pair (t, s) and which of its thread's pairs it is (franka_collision_env_kernel:
    p = threadIdx.x + k * BLOCK over the chunk's flattened pairs)."""
    S = fc.num_spheres(case)
    env_block, col_tc = fc.env_form()
    return t // col_tc, ((t % col_tc) * S + s) // env_block


def test_flags_only_boundary_in_the_256_thread_forms():
    """In the 256-thread forms a thread decides up to 16 pairs and steps (waypoint, sphere) itself.  For environments
    whose distances are all > 1e-3: every radius 0 except one sphere's, set to the smallest distance that sphere has
    over the trajectory (as the device computed it) -- the flag must be what ``min_sdf <= radius`` gives at that value,
    one float below and above, 1e-6 and 1 % off, and with all radii -1.  The sphere is the one of the closest pair; where
    the distances offer them also one whose deciding pair sits in the last chunk of a multi-chunk case and one whose
    deciding pair is its thread's last (k = PPT - 1)."""
    decided, per_route, last_chunk, last_pair = 0, {}, 0, 0
    f32 = np.float32
    for case in fc.CASES:
        name, chunks, _ = fc.case_route(case)
        if not name.startswith("ppt") or case.B > 5:
            continue
        ppt = int(name[3:])
        r = run_of(case)
        msdf = r.msdf.cpu().numpy()
        for b in range(case.B):
            d = msdf[b]  # [T,S]
            if not (np.isfinite(d).all() and (d > 1e-3).all()):
                continue  # (a sphere inside or on an obstacle: every non-negative radius collides; no live primitive: none does)
            fl, _ = r.call(False, radii=D(np.full(r.S, -1.0, f32)), env=b)
            assert fl.item() == 0
            tmin = d.argmin(axis=0)  # per sphere: the waypoint that decides it
            t_star, s_star = np.unravel_index(int(d.argmin()), d.shape)
            targets = [int(s_star)]
            own = [_owner(case, int(tmin[s]), s) for s in range(r.S)]
            in_last = [s for s in range(r.S) if chunks > 1 and own[s][0] == chunks - 1]
            is_last_k = [s for s in range(r.S) if own[s][1] == ppt - 1]
            targets += in_last[:1] + is_last_k[:1]
            for s in dict.fromkeys(targets):
                v = d[tmin[s], s]
                assert v == d[:, s].min()
                for rad, want in ((v, 1), (np.nextafter(v, f32(0)), 0), (np.nextafter(v, f32(9)), 1),
                                  (v * f32(1 - 1e-6), 0), (v * f32(1 + 1e-6), 1), (v * f32(0.99), 0), (v * f32(1.01), 1)):
                    radii = np.zeros(r.S, f32)
                    radii[s] = rad
                    fl, _ = r.call(False, radii=D(radii), env=b)
                    assert fl.item() == want, (fc.case_id(case), b, s, int(tmin[s]), float(v), float(rad), want)
                last_chunk += s in in_last
                last_pair += s in is_last_k
            decided += 1
            per_route[name] = per_route.get(name, 0) + 1
    print(f"FORMS boundary: {decided} environments decided, per route {per_route}, deciding pair in a last chunk {last_chunk}, "
          f"as a thread's last pair {last_pair}")
    assert decided >= 10
    assert set(per_route) == {"ppt%d" % p for p in range(2, 17, 2)}
    assert last_chunk >= 1 and last_pair >= 1


def test_comparator_flags_a_planted_chunk_tail_row():
    """Sensitivity control: in a copy of the device's distances the last waypoint of a multi-chunk case (the ragged
    chunk's tail) gets its neighbour's values -- the comparator flags exactly that environment."""
    for case in fc.CASES:
        name, chunks, last = fc.case_route(case)
        if chunks < 2 or not name.startswith("ppt") or fc.num_spheres(case) < 16:
            continue
        r = run_of(case)
        got = r.msdf.cpu().numpy().copy()
        assert fc.offending_envs(got, r.ref64)[0] == set()
        b = case.B - 1
        got[b, case.T - 1] = got[b, case.T - 2]
        assert fc.offending_envs(got, r.ref64)[0] == {b}, fc.case_id(case)
