"""The Franka solver wrappers and the three collision checks driven on CPU tensors with the library call recorded: what
each hands to C, over a fixed grid of argument forms.  Shared by tests/test_solvers_host.py (which asserts on the raw
arguments) and tools/solver_calls.py (which writes them as JSON, to compare two trees).  Everything is reached through
``mpinets_amd.robot``, so the grid also runs on a tree from before ``solvers.py``.

No kernel runs: ``_lib.call`` and ``_lib.require_cuda`` are replaced, the size queries (``*_scratch``) are host functions."""
import contextlib
import ctypes
import itertools
from types import SimpleNamespace

import torch

from mpinets_amd import _lib, robot
from mpinets_amd import franka_tables as ft
from mpinets_amd.field import CloudField

try:  # the module that owns PLAN_CLOUD_SCRATCH_BYTES (``robot`` itself on a tree from before the split)
    from mpinets_amd import solvers as OWNER
except ImportError:
    OWNER = robot

T = 6  # waypoints: small, the calls only size buffers with it
N = 5  # cloud rows


@contextlib.contextmanager
def recording():
    """-> the list that every ``_lib.call`` inside the block is appended to as (entry name, argument tuple)."""
    calls, saved = [], (_lib.call, _lib.require_cuda)
    _lib.call, _lib.require_cuda = (lambda name, *args: calls.append((name, args))), (lambda *tensors: None)
    try:
        yield calls
    finally:
        _lib.call, _lib.require_cuda = saved


def _fields(struct):
    return {n: (list(v) if isinstance(v := getattr(struct, n), ctypes.Array) else v) for n, _ in struct._fields_}


def describe(name, args, inputs):
    """One recorded call as JSON-able data: integers and floats as they are, an options or grid struct by its fields, a
    pointer as None (None or 0: NULL either way), ``input:<argument name>+<byte offset>`` inside a tensor of ``inputs``, or
    ``other`` (a table, an output, scratch)."""
    out = []
    for a, ctype in zip(args, _lib.PROTOTYPES[name]):
        if hasattr(a, "_obj"):
            a = _fields(a._obj)
        elif ctype is ctypes.c_void_p and a is not None:
            where = "other"
            for key, t in inputs.items():
                base, size = t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()
                if a and (base <= a < base + size or a == t.data_ptr()):
                    where = f"input:{key}+{a - t.data_ptr()}"
                    break
            a = where if a else None
        out.append(a)
    return {"entry": name, "args": out}


def _cuboids(B):
    return SimpleNamespace(centers=torch.zeros(B, 2, 3), inv_frames=torch.zeros(B, 2, 16), dims=torch.ones(B, 2, 3))


def _cylinders(B):
    return SimpleNamespace(centers=torch.zeros(B, 3, 3), inv_frames=torch.zeros(B, 3, 16), radii=torch.ones(B, 3, 1),
                           heights=torch.ones(B, 3, 1))


def sampler():
    """A ``FrankaCollisionSampler`` with its tables on the CPU (the constructor asks for a GPU)."""
    s = object.__new__(robot.FrankaCollisionSampler)
    c, r, l, s.groups = ft.collision_sphere_table(False)
    s.centers, s.radii, s.links = (torch.from_numpy(a) for a in (c, r, l))
    s.num_spheres, s.finger, s.device = int(c.shape[0]), float(ft.FINGER_OPENING), torch.device("cpu")
    return s


def _tensors(prefix, obj):
    return {} if obj is None else {f"{prefix}.{k}": v for k, v in vars(obj).items()}


def cloud_forms(B):
    """name -> a cloud [B,N,3]: contiguous, a view of rows 2..6 of a [B,9,4] slab, and one without rows."""
    return {"contiguous": torch.zeros(B, N, 3), "view": torch.zeros(B, 9, 4)[:, 2:7, :3], "empty": torch.zeros(B, 0, 3)}


def cases():
    """-> (case id, thunk that makes the wrapper call, {argument name: tensor the call passes}) over the fixed grid."""
    flags, both = (False, True), itertools.product
    ik_opts, plan_opts, rm_opts = dict(iterations=7, damping=0.25, check_self=False), dict(candidates=3, substeps=2, clearance=0.01), \
        dict(nodes=8, connect_radius=2.0, check_self=False)
    s = sampler()
    for B in (0, 1, 3):
        poses, q0, q1, qi = torch.eye(4).repeat(B, 1, 1), torch.zeros(B, 7), torch.ones(B, 7) * 0.1, torch.full((B, 7), 0.2)
        traj, counts, active = torch.zeros(B, T, 7), torch.full((B,), 4, dtype=torch.int32), torch.ones(B, T, dtype=torch.int32)
        seeds = torch.zeros(B, 1, T, 7)
        for with_cub, with_cyl in both(flags, flags):
            cub, cyl = _cuboids(B) if with_cub else None, _cylinders(B) if with_cyl else None
            prims = dict(_tensors("cuboids", cub), **_tensors("cylinders", cyl))
            tag = f"B{B} cub{int(with_cub)} cyl{int(with_cyl)}"
            for init, every, opts in both(flags, flags, flags):
                o = ik_opts if opts else {}
                yield (f"franka_ik {tag} init{int(init)} all{int(every)} opts{int(opts)}",
                       lambda cub=cub, cyl=cyl, init=init, every=every, o=o: robot.franka_ik(
                           poses, cub, cyl, q_init=qi if init else None, seed=7, env_offset=3, return_all=every, **dict(o)),
                       dict(prims, target_poses=poses, **({"q_init": qi} if init else {})))
            for seeded, every, opts in both(flags, flags, flags):
                o = plan_opts if opts else {}
                yield (f"franka_plan {tag} seeds{int(seeded)} all{int(every)} opts{int(opts)}",
                       lambda cub=cub, cyl=cyl, seeded=seeded, every=every, o=o: robot.franka_plan(
                           q0, q1, cub, cyl, T=T, seed=7, env_offset=3, return_all=every, seeds=seeds if seeded else None, **o),
                       dict(prims, q_start=q0, q_goal=q1, **({"seeds": seeds} if seeded else {})))
            for graph, opts in both(flags, flags):
                o = rm_opts if opts else {}
                yield (f"franka_roadmap {tag} graph{int(graph)} opts{int(opts)}",
                       lambda cub=cub, cyl=cyl, graph=graph, o=o: robot.franka_roadmap(
                           q0, q1, cub, cyl, T=T, seed=7, env_offset=3, return_graph=graph, **o),
                       dict(prims, q_start=q0, q_goal=q1))
            for every, opts in both(flags, flags):
                o, rm = (plan_opts, rm_opts) if opts else ({}, None)
                yield (f"franka_plan_global {tag} all{int(every)} opts{int(opts)}",
                       lambda cub=cub, cyl=cyl, every=every, o=o, rm=rm: robot.franka_plan_global(
                           q0, q1, cub, cyl, T=T, seed=7, env_offset=3, return_all=every, roadmap=rm, **o),
                       dict(prims, q_start=q0, q_goal=q1))
            for sdf in flags:
                yield (f"check {tag} sdf{int(sdf)}", lambda cub=cub, cyl=cyl, sdf=sdf: s.check(traj, cub, cyl, return_sdf=sdf),
                       dict(prims, q=traj))
        for form, cloud in cloud_forms(B).items():
            with recording():
                field = CloudField.build(cloud)
            for cnt in flags:
                cn = counts if cnt else None
                tag, given = f"B{B} cloud:{form} counts{int(cnt)}", dict({"cloud": cloud}, **({"counts": counts} if cnt else {}))
                for init, every, opts in both(flags, flags, flags):
                    o = ik_opts if opts else {}
                    yield (f"franka_ik_cloud {tag} init{int(init)} all{int(every)} opts{int(opts)}",
                           lambda cloud=cloud, cn=cn, init=init, every=every, o=o: robot.franka_ik_cloud(
                               poses, cloud, cn, 0.01, q_init=qi if init else None, seed=7, env_offset=3, return_all=every,
                               **dict(o)),
                           dict(given, target_poses=poses, **({"q_init": qi} if init else {})))
                for own, every, opts in both(flags, flags, flags):
                    o = plan_opts if opts else {}
                    yield (f"franka_plan_cloud {tag} field{int(own)} all{int(every)} opts{int(opts)}",
                           lambda cloud=cloud, cn=cn, own=own, every=every, o=o, field=field: robot.franka_plan_cloud(
                               q0, q1, cloud, cn, field=field if own else None, point_radius=0.01, T=T, seed=7, env_offset=3,
                               return_all=every, **o),
                           dict(given, q_start=q0, q_goal=q1, **({"field.values": field.values} if own else {})))
                for dist, near in both(flags, flags):
                    yield (f"check_cloud {tag} dist{int(dist)} near{int(near)}",
                           lambda cloud=cloud, cn=cn, dist=dist, near=near: s.check_cloud(
                               traj, cloud, cn, 0.01, 0.02, return_distance=dist, return_nearest=near),
                           dict(given, q=traj))
                for act in flags:
                    yield (f"check_cloud_each {tag} active{int(act)}",
                           lambda cloud=cloud, cn=cn, act=act: s.check_cloud_each(traj, cloud, cn, 0.01, 0.02,
                                                                                  active=active if act else None),
                           dict(given, q=traj, **({"active": active} if act else {})))


SLAB_B, SLAB_ROWS = 12, 5  # ``slabbed_plan_cloud``: 12 problems under a bound of 5 problems' scratch -> slabs of 5, 5 and 2


def slabbed_plan_cloud():
    """-> the calls of one ``franka_plan_cloud`` over 12 problems with the scratch bound at 5 problems', and its inputs."""
    q0, q1, cloud = torch.zeros(SLAB_B, 7), torch.ones(SLAB_B, 7) * 0.1, torch.zeros(SLAB_B, 9, 4)[:, 2:7, :3]
    counts = torch.full((SLAB_B,), 4, dtype=torch.int32)
    per = int(_lib.load().mpx_franka_plan_cloud_scratch(1, T, robot.PLAN_DEFAULTS["candidates"], robot.PLAN_DEFAULTS["substeps"]))
    saved = OWNER.PLAN_CLOUD_SCRATCH_BYTES
    OWNER.PLAN_CLOUD_SCRATCH_BYTES = SLAB_ROWS * per
    try:
        with recording() as calls:
            out = robot.franka_plan_cloud(q0, q1, cloud, counts, point_radius=0.01, T=T, seed=7, return_all=True)
    finally:
        OWNER.PLAN_CLOUD_SCRATCH_BYTES = saved
    inputs = dict(q_start=q0, q_goal=q1, cloud=cloud, counts=counts)
    return calls, inputs, out
