"""Generates tests/golden/scene_reference_golden.npz by IMPORTING AND RUNNING the reference's scene construction:
mpinets/data_pipeline/environments/cubby_environment.py (``Cubby.cuboids``, ``Cubby.support_volumes``, the merge rule of
``MergedCubbyEnvironment.gen``, :679-686) and tabletop_environment.py (``TabletopEnvironment.place_objects`` :129-153 and
``setup_tables`` :215-324).

Runs only where the reference is checked out (``MPINETS_REFERENCE`` or /root/reference); only the .npz is committed.  The
modules import absent packages; each stub supplies only what the executed lines touch:

* ``geometrout.primitive``: ``Cuboid`` / ``Cylinder`` below, backed by this repo's ``mpinets_amd.primitives`` for ``sdf``,
  with the attributes ``setup_tables`` reads and mutates (``_pose._xyz``, ``_dims``, ``dims``, ``center``, ``corners``,
  ``half_extents``) and ``Cuboid.random`` drawing uniformly between its bounds (recalled, not pinned: geometrout is absent);
* ``geometrout.transform.SE3`` (``.xyz``, ``.so3.wxyz``) / ``SO3`` and ``pyquaternion.Quaternion(matrix=)`` (``.w .x .y .z``);
* robofin.*, pybullet and the like: empty modules whose attributes are placeholders (imported, never touched here).

What executes is the reference's own: the seven plates and their pivot about the cabinet's centre, the four branches of
``support_volumes`` under the four thickness states, the merge rule on the twelve ordered pocket pairs, the greedy walk of
``place_objects`` (with ``random_points_on_table`` and ``random_object`` scripted: points and objects are inputs, the
accepted indices and the clearances handed over are the outputs), and ``setup_tables`` under a recorded random source.

    python tests/golden/gen_scene_reference_golden.py
"""
import math
import os
import sys
import types

sys.dont_write_bytecode = True  # importing the reference must not leave __pycache__ in it

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("MPINETS_REFERENCE", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "motion-policy-networks_amd"), REFERENCE]

from mpinets_amd import primitives  # noqa: E402


def quat_of(R):
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = np.zeros(4)
    q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q


class Quaternion:
    def __init__(self, matrix=None):
        self.w, self.x, self.y, self.z = quat_of(np.asarray(matrix)[:3, :3])


class SO3:
    def __init__(self, wxyz):
        self.wxyz = np.asarray(wxyz, float)

    @classmethod
    def from_rpy(cls, r, p, y):
        assert r == 0 and p == 0
        return cls([math.cos(y / 2), 0, 0, math.sin(y / 2)])


class SE3:
    def __init__(self, matrix=None, xyz=None, so3=None):
        if matrix is not None:
            xyz, so3 = np.asarray(matrix)[:3, 3], SO3(quat_of(np.asarray(matrix)[:3, :3]))
        self._xyz, self._so3 = np.array(xyz, float), so3

    @property
    def xyz(self):
        return self._xyz

    @property
    def so3(self):
        return self._so3


class Cuboid:
    def __init__(self, center, dims, quaternion=(1.0, 0.0, 0.0, 0.0)):
        self._pose, self._dims = SE3(xyz=center, so3=SO3(quaternion)), np.array(dims, float)

    dims = property(lambda self: self._dims)
    center = property(lambda self: self._pose._xyz)
    pose = property(lambda self: self._pose)
    half_extents = property(lambda self: self._dims / 2)

    @property
    def corners(self):
        assert np.allclose(self._pose._so3.wxyz, [1, 0, 0, 0])
        signs = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float)
        return self._pose._xyz + signs * self._dims / 2

    def sdf(self, point):
        return float(primitives.Cuboid(self.center, self.dims, self._pose._so3.wxyz).sdf(np.asarray(point, float)[None])[0])

    @classmethod
    def random(cls, center_range=None, dimension_range=None, quaternion=False):
        assert not quaternion
        return cls(np.random.uniform(*center_range), np.random.uniform(*dimension_range))


class Cylinder:
    def __init__(self, center, radius, height, quaternion=(1.0, 0.0, 0.0, 0.0)):
        self.center, self.radius, self.height, self.quaternion = np.array(center, float), radius, height, quaternion

    def sdf(self, point):
        return float(primitives.Cylinder(self.center, self.radius, self.height, self.quaternion).sdf(np.asarray(point, float)[None])[0])


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def install_stubs():
    for name in ("geometrout", "geometrout.primitive", "geometrout.transform", "pyquaternion", "robofin", "robofin.bullet",
                 "robofin.robots", "robofin.collision", "pybullet", "trimesh", "meshcat", "urchin", "yourdfpy", "ikfast_franka_panda"):
        sys.modules.setdefault(name, _Anything(name))
    sys.modules["geometrout.primitive"].Cuboid, sys.modules["geometrout.primitive"].Cylinder = Cuboid, Cylinder
    sys.modules["geometrout.primitive"].Sphere = type("Sphere", (), {})
    sys.modules["geometrout.transform"].SE3, sys.modules["geometrout.transform"].SO3 = SE3, SO3
    sys.modules["pyquaternion"].Quaternion = Quaternion


CUBBY_KEYS = ("cubby_left", "cubby_right", "cubby_bottom", "cubby_front", "cubby_back", "cubby_top", "cubby_mid_h_z",
              "cubby_mid_v_y", "thickness", "middle_shelf_thickness", "center_wall_thickness", "in_cabinet_rotation")


def boxes_of(cuboids, n):
    out = np.full((n, 10), np.nan)
    for i, c in enumerate(cuboids):
        out[i] = np.r_[c.center, c.dims, c.pose.so3.wxyz]
    return out


def cubbies(ce, n=16):
    rng = np.random.default_rng(7)
    params, plates, supports, counts = [], [], [], []
    for _ in range(n):
        cubby = ce.Cubby()  # (its own draws are overwritten: every parameter is set explicitly)
        front = rng.uniform(0.45, 0.65)
        values = dict(cubby_left=rng.uniform(0.6, 0.8), cubby_right=rng.uniform(-0.8, -0.6), cubby_bottom=rng.uniform(0.1, 0.3),
                      cubby_front=front, cubby_back=front + rng.uniform(0.15, 0.55), cubby_top=rng.uniform(0.6, 0.8),
                      cubby_mid_h_z=rng.uniform(0.35, 0.55), cubby_mid_v_y=rng.uniform(-0.1, 0.1), thickness=rng.uniform(0.01, 0.03),
                      in_cabinet_rotation=rng.uniform(-np.pi / 18, np.pi / 18))
        for k, v in values.items():
            setattr(cubby, k, float(v))
        for shelf_gone in (False, True):  # the four thickness states
            for wall_gone in (False, True):
                cubby.middle_shelf_thickness = 0.0 if shelf_gone else cubby.thickness
                cubby.center_wall_thickness = 0.0 if wall_gone else cubby.thickness
                params.append([getattr(cubby, k) for k in CUBBY_KEYS])
                cs, vs = cubby.cuboids, cubby.support_volumes
                plates.append(boxes_of(cs, 7)), supports.append(boxes_of(vs, 4)), counts.append([len(cs), len(vs)])
    return dict(cubby_params=np.array(params), cubby_plates=np.array(plates), cubby_supports=np.array(supports),
                cubby_counts=np.array(counts))


def merge_rule(ce):
    """``MergedCubbyEnvironment.gen`` on scripted candidates: which thickness it zeroes for each ordered pocket pair, and the
    support each of the two poses ends in (a point at the centre of its original pocket)."""
    rows = []
    for a in range(4):
        for b in range(4):
            if a == b:
                continue
            env = ce.MergedCubbyEnvironment.__new__(ce.MergedCubbyEnvironment)
            env.cubby = ce.Cubby()
            pockets = env.cubby.support_volumes
            cands = [types.SimpleNamespace(pocket_idx=p, pose=types.SimpleNamespace(xyz=np.array(pockets[p].center)),
                                           support_volume=pockets[p]) for p in (a, b)]
            env.demo_candidates = list(cands)
            parent = ce.CubbyEnvironment.gen
            ce.CubbyEnvironment.gen = lambda self, selfcc: True  # (the environment and its candidates are the scripted ones)
            try:
                assert ce.MergedCubbyEnvironment.gen(env, None)
            finally:
                ce.CubbyEnvironment.gen = parent
            rows.append([a, b, int(env.cubby.middle_shelf_thickness == 0.0), int(env.cubby.center_wall_thickness == 0.0),
                         env.demo_candidates[0].pocket_idx, env.demo_candidates[1].pocket_idx])
    return dict(merge_rule=np.array(rows))


def placements(te, n=24):
    rng = np.random.default_rng(11)
    out = dict(place_points=[], place_objects=[], place_K=[], place_accepted=[], place_clearance=[])
    for _ in range(n):
        K = int(rng.integers(3, 15))
        h = float(rng.uniform(0, 0.4))
        points = np.c_[rng.uniform(0.3, 1.3, 10 * K), rng.uniform(-0.7, 0.3, 10 * K), np.full(10 * K, h)]
        script = np.c_[rng.random(14) < 0.3, rng.uniform(0.3, 1.0, (14, 3)), rng.uniform(0, np.pi / 2, 14)]  # type, fractions, yaw
        env = te.TabletopEnvironment.__new__(te.TabletopEnvironment)
        env.objects = []
        accepted, clearance = [], []

        def random_object(x, y, z, dim_min, dim_max, script=script, accepted=accepted, clearance=clearance, points=points):
            i = len(clearance)
            accepted.append(int(np.flatnonzero((points[:, 0] == x) & (points[:, 1] == y))[0]))
            clearance.append(dim_max)
            xm = min(dim_max, 0.15)
            if script[i, 0]:
                hh = 0.05 + 0.3 * script[i, 2]
                return Cylinder([x, y, z + hh / 2], dim_min + script[i, 1] * (xm - dim_min), hh)
            d = [dim_min + script[i, 1] * (xm - dim_min), dim_min + script[i, 2] * (xm - dim_min), 0.05 + 0.3 * script[i, 3]]
            return Cuboid([x, y, z + d[2] / 2], d, [math.cos(script[i, 4] / 2), 0, 0, math.sin(script[i, 4] / 2)])

        env.random_points_on_table = lambda how_many, points=points: points[:how_many]
        env.random_object = random_object
        env.place_objects(K)
        objs = np.full((14, 6), np.nan)  # type (1 cylinder, 2 cuboid), x, y, radius or dx, dy, yaw
        for i, o in enumerate(env.objects):
            objs[i] = [1, o.center[0], o.center[1], o.radius, 0, 0] if isinstance(o, Cylinder) else \
                [2, o.center[0], o.center[1], o.dims[0], o.dims[1], 2 * math.atan2(o.pose.so3.wxyz[3], o.pose.so3.wxyz[0])]
        pad = lambda v, fill: np.r_[np.asarray(v, float), np.full(14 - len(v), fill)]  # noqa: E731
        out["place_points"].append(np.r_[points[:, :2], np.full((140 - len(points), 2), np.nan)])
        out["place_objects"].append(objs), out["place_K"].append(K)
        out["place_accepted"].append(pad(accepted, -1)), out["place_clearance"].append(pad(clearance, np.nan))
    return {k: np.array(v) for k, v in out.items()}


def tables(te, n=24):
    """``setup_tables`` under a recorded random source: the draws, by the order the reference makes them, and its tables."""
    out = dict(tables_params=[], tables_task=[], tables_free=[])
    uniform, choice = np.random.uniform, np.random.choice
    for seed in range(n):
        np.random.seed(100 + seed)
        log = []

        def recorded(*a, **k):
            v = uniform(*a, **k)
            log.append(v)
            return v

        def chosen(values, p=None, **k):
            log.append(("choice", choice(values, p=p, **k)))
            return log[-1][1]

        env = te.TabletopEnvironment.__new__(te.TabletopEnvironment)
        np.random.uniform, np.random.choice = recorded, chosen
        try:
            env.setup_tables()
        finally:
            np.random.uniform, np.random.choice = uniform, choice
        height = float(log[1][1])
        side = bool(log[5] < 0.5)
        rest = log[8:]
        p = dict(height=height, front_x_min=log[2], front_x_max=log[3], front_y_max=log[4], has_side_table=side, front_y_min=log[6],
                 front_task_scalar=log[7], side_y_max=np.nan, side_length=np.nan, side_task_scalar=np.nan)
        if side:  # (rest[2] is the unused side_x)
            p.update(side_y_max=rest[0], side_length=rest[1], side_task_scalar=rest[3])
            rest = rest[4:]
        p.update(mount_x=rest[0][0], mount_y=rest[0][1], mount_dim_y=rest[1][1])
        out["tables_params"].append([float(p[k]) for k in TABLE_KEYS])
        out["tables_task"].append(boxes_of(env.tables, 2)[:, :6]), out["tables_free"].append(boxes_of(env.clear_tables, 3)[:, :6])
    return {k: np.array(v) for k, v in out.items()}


TABLE_KEYS = ("height", "front_x_min", "front_x_max", "front_y_max", "has_side_table", "front_y_min", "front_task_scalar",
              "side_y_max", "side_length", "side_task_scalar", "mount_x", "mount_y", "mount_dim_y")


def main():
    install_stubs()
    from mpinets.data_pipeline.environments import cubby_environment as ce
    from mpinets.data_pipeline.environments import tabletop_environment as te

    np.random.seed(0)
    data = dict(cubby_keys=np.array(CUBBY_KEYS), table_keys=np.array(TABLE_KEYS))
    data.update(cubbies(ce)), data.update(merge_rule(ce)), data.update(placements(te)), data.update(tables(te))
    path = os.path.join(HERE, "scene_reference_golden.npz")
    np.savez_compressed(path, **data)
    print(path, {k: v.shape for k, v in data.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
