"""Synthetic planning problems for tests and benchmarks.

The reference's scene generators (``mpinets/data_pipeline/environments/*.py``) need PyBullet and
IK and are out of scope; this module restates their *distributions* with a seeded NumPy RNG.  Three LOOSE stand-ins, kept
bit for bit because benchmarks and goldens are drawn from them:

* tabletop -- ``tabletop_environment.py:215-324,406-441``: table height 0 w.p. 0.35 else U(0,0.4);
  front table x in [U(.275,.375), U(1.275,1.375)], width U(1.5,1.65); optional side table p=0.5;
  K ~ randint(3,15) objects, 30 % cylinders r in [.05,.15], h in [.05,.35], else cuboids
  xy in [.05,.15], z in [.05,.35], yaw U(0, pi/2);
* cubby -- ``cubby_environment.py:62-74``: a 2x2 shelf made of 7 thin cuboids (thickness
  U(.01,.03)), yaw +-pi/18;
* dresser-like -- ``dresser_environment.py:198-222``: up to 40 yaw-rotated cuboids.

and three restatements that follow the reference's construction draw by draw and plate by plate (each in two stages,
draws -> named parameters and parameters -> primitives and supports; the second stage is pinned by fixtures made by
running the reference, tests/golden/gen_scene_reference_golden.py):

* tabletop_reference -- ``setup_tables`` + ``place_objects`` + ``random_object`` (``tabletop_environment.py:129-153,
  215-324,406-441``): solid tables from z = -0.02 up, split into task and free parts, the mount table, and K = 3..14 objects
  placed greedily at least 5 cm from the objects before them, the clearance found bounding the new footprint;
* cubby_reference -- ``Cubby.__init__``, ``.cuboids``, ``.support_volumes`` (``cubby_environment.py:62-431``): twelve
  parameters, seven plates in the reference's order rotated about the cabinet's centre, four pockets;
* merged_cubby -- ``MergedCubbyEnvironment`` (``:660-704``): that cubby with the plates between two pockets removed.

Primitive sets are zero-padded to fixed M1 / M2 exactly like the dataset rows
(zero dims, identity quaternion, ``mpinets/data_loader.py:202,210-215``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import franka_tables as ft

NUM_ROBOT_POINTS = 2048
NUM_OBSTACLE_POINTS = 4096
NUM_TARGET_POINTS = 128


def _yaw_quat(yaw):
    q = np.zeros(np.shape(yaw) + (4,))
    q[..., 0] = np.cos(np.asarray(yaw) / 2)
    q[..., 3] = np.sin(np.asarray(yaw) / 2)
    return q


SUPPORT_PADDING, SUPPORT_SURFACE, SUPPORT_VOLUME = 0, 1, 2  # ``support_kind`` (``solvers.TASK_*``)


def _support(supports, kind, centre, dims, quat, approach, weight):
    """One row of ``make_task_scenes``' ``support_boxes`` / ``support_kind`` (``supports`` None: ``make_scenes``, nothing kept).
    Nothing here draws from an rng: the supports are read off what a generator has already placed."""
    if supports is not None:
        supports.append((kind, np.concatenate([np.asarray(centre, float), np.asarray(dims, float), np.asarray(quat, float),
                                               [float(approach), float(weight)]])))


def _tabletop(rng, M1, M2, supports=None):
    cc, cd, cq = np.zeros((M1, 3)), np.zeros((M1, 3)), np.tile([1.0, 0, 0, 0], (M1, 1))
    yc, yr, yh, yq = np.zeros((M2, 3)), np.zeros((M2, 1)), np.zeros((M2, 1)), np.tile([1.0, 0, 0, 0], (M2, 1))
    h = 0.0 if rng.random() < 0.35 else rng.uniform(0.0, 0.4)
    x0, x1 = rng.uniform(0.275, 0.375), rng.uniform(1.275, 1.375)
    w = rng.uniform(1.5, 1.65)
    thick = 0.05
    n = 0
    cc[n], cd[n] = [(x0 + x1) / 2, 0.0, h - thick / 2], [x1 - x0, w, thick]
    _support(supports, SUPPORT_SURFACE, cc[n], cd[n], cq[n], 0.0, cd[n][0] * cd[n][1])  # (weight: the top face's area)
    n += 1
    if rng.random() < 0.5:  # side table
        side = rng.choice([-1.0, 1.0])
        cc[n], cd[n] = [0.0, side * (w / 4 + 0.45), h - thick / 2], [0.9, w / 2, thick]
        _support(supports, SUPPORT_SURFACE, cc[n], cd[n], cq[n], 0.0, cd[n][0] * cd[n][1])
        n += 1
    cc[n], cd[n] = [-0.35, 0.0, -0.025], [0.6, 0.6, 0.05]  # mount table under the robot
    n += 1
    K = int(rng.integers(3, 15))
    m = 0
    for _ in range(K):
        px, py = rng.uniform(x0 + 0.1, x1 - 0.1), rng.uniform(-w / 2 + 0.1, w / 2 - 0.1)
        if rng.random() < 0.3 and m < M2:
            r, hh = rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.35)
            yc[m], yr[m], yh[m] = [px, py, h + hh / 2], r, hh
            m += 1
        elif n < M1:
            d = np.array([rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.15), rng.uniform(0.05, 0.35)])
            cc[n], cd[n], cq[n] = [px, py, h + d[2] / 2], d, _yaw_quat(rng.uniform(0, np.pi / 2))
            n += 1
    return cc, cd, cq, yc, yr, yh, yq


def _cubby(rng, M1, M2, supports=None):
    cc, cd, cq = np.zeros((M1, 3)), np.zeros((M1, 3)), np.tile([1.0, 0, 0, 0], (M1, 1))
    yc, yr, yh, yq = np.zeros((M2, 3)), np.zeros((M2, 1)), np.zeros((M2, 1)), np.tile([1.0, 0, 0, 0], (M2, 1))
    t = rng.uniform(0.01, 0.03)
    W, H, D = rng.uniform(0.7, 1.1), rng.uniform(0.5, 0.9), rng.uniform(0.2, 0.35)
    cx, cz = rng.uniform(0.55, 0.8), rng.uniform(0.1, 0.3)
    yaw = rng.uniform(-np.pi / 18, np.pi / 18)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    parts = [  # local centre, dims (x = depth, y = width, z = height)
        ([0, 0, 0], [D, W, t]), ([0, 0, H], [D, W, t]), ([0, 0, H / 2], [D, W, t]),  # bottom, top, mid shelf
        ([0, -W / 2, H / 2], [D, t, H]), ([0, W / 2, H / 2], [D, t, H]), ([0, 0, H / 2], [D, t, H]),  # sides, divider
        ([D / 2, 0, H / 2], [t, W, H]),  # back
    ]
    for i, (lc, dims) in enumerate(parts[:M1]):
        cc[i] = R @ np.array(lc) + np.array([cx, 0, cz])
        cd[i] = dims
        cq[i] = _yaw_quat(yaw)
    # the four pockets: the interior between the shelves, the walls and the back that bound each (the opening faces -x of
    # the cubby's frame, toward the robot: the gripper reaches along world x, approach 0, as the reference's does)
    for z0, z1 in ((t / 2, H / 2 - t / 2), (H / 2 + t / 2, H - t / 2)):
        for y0, y1 in ((-W / 2 + t / 2, -t / 2), (t / 2, W / 2 - t / 2)):
            lc = [-t / 4, (y0 + y1) / 2, (z0 + z1) / 2]  # (x from the opening at -D / 2 to the back plate's face)
            _support(supports, SUPPORT_VOLUME, R @ np.array(lc) + np.array([cx, 0, cz]), [D - t / 2, y1 - y0, z1 - z0],
                     _yaw_quat(yaw), 0.0, 1.0)
    return cc, cd, cq, yc, yr, yh, yq


def _dresser(rng, M1, M2, supports=None):
    cc, cd, cq = np.zeros((M1, 3)), np.zeros((M1, 3)), np.tile([1.0, 0, 0, 0], (M1, 1))
    yc, yr, yh, yq = np.zeros((M2, 3)), np.zeros((M2, 1)), np.zeros((M2, 1)), np.tile([1.0, 0, 0, 0], (M2, 1))
    W, D, H = 1.0 + rng.uniform(-0.2, 0.2), 0.3 + rng.uniform(-0.1, 0.1), 0.7 + rng.uniform(-0.15, 0.15)
    cx = 0.65 + rng.uniform(-0.1, 0.1)
    yaw = np.pi / 2 + rng.uniform(-np.pi / 3, np.pi / 3)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    n = min(M1, int(rng.integers(12, 41)))
    rows = int(np.ceil(np.sqrt(n)))
    for i in range(n):
        r_, c_ = divmod(i, rows)
        w_, h_ = W / rows, H / rows
        lc = np.array([(c_ + 0.5) * w_ - W / 2, rng.uniform(-0.02, 0.02), (r_ + 0.5) * h_])
        cc[i] = R @ lc + np.array([cx, 0, 0])
        cd[i] = [w_ * 0.95, D, h_ * 0.2]
        cq[i] = _yaw_quat(yaw)
        # the free space above the plate inside its cell (a stand-in: this dresser is not the reference's recursive one);
        # the reach runs along the plate's depth axis (local y), in the sense that has a positive world-x component
        depth_yaw = yaw + (np.pi / 2 if s < 0 else -np.pi / 2)  # (local y is (-s, c, 0) in the world)
        _support(supports, SUPPORT_VOLUME, R @ np.array([lc[0], lc[1], (r_ + 0.8) * h_]) + np.array([cx, 0, 0]),
                 [w_ * 0.95, D, h_ * 0.4], _yaw_quat(yaw), depth_yaw, 1.0)
    return cc, cd, cq, yc, yr, yh, yq


# ---- the reference's scenes, stage by stage ------------------------------------------------------------------------------------
MERGE_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))  # the six unordered pocket pairs, in the order they are drawn


def _tabletop_reference_parameters(rng) -> Dict[str, float]:
    """Stage 1 of ``setup_tables`` (tabletop_environment.py:215-324): the draws, named.  The reference also draws ``side_x``
    (:283), ``xdim`` (:315) and ``ydim`` (:321) and uses none of them: they are DROPPED here, not consumed."""
    p = dict(height=0.0 if rng.random() < 0.35 else rng.uniform(0.0, 0.4), front_x_min=rng.uniform(0.275, 0.375),
             front_x_max=rng.uniform(1.275, 1.375), front_y_max=rng.uniform(1.5, 1.65), has_side_table=bool(rng.random() < 0.5))
    p["front_y_min"] = rng.uniform(-1.0, -0.75) if p["has_side_table"] else rng.uniform(-0.75, -0.55)
    p["front_task_scalar"] = rng.uniform(0.55, 0.65)
    if p["has_side_table"]:
        p.update(side_y_max=rng.uniform(-0.325, -0.275), side_length=rng.uniform(0.0, 1.375), side_task_scalar=rng.uniform(0.55, 0.65))
    p.update(mount_x=rng.uniform(-0.02, 0.02), mount_y=rng.uniform(-0.02, 0.02), mount_dim_y=rng.uniform(0.9, 0.94))
    return p


def _tabletop_reference_tables(p):
    """Stage 2: -> (task tables, free tables + the mount table), each a list of (centre, dims): the reference's ``tables`` and
    ``clear_tables``.  Every table is a solid block from z = -0.02 to the table height."""
    z, dz = (p["height"] - 0.02) / 2, p["height"] + 0.02
    x0, x1, y0, y1 = p["front_x_min"], p["front_x_max"], p["front_y_min"], p["front_y_max"]
    ty = p["front_task_scalar"] * (y1 - y0)
    task = [([(x0 + x1) / 2, ty / 2 + y0, z], [x1 - x0, ty, dz])]
    free = [([(x0 + x1) / 2, (y1 + (y0 + ty)) / 2, z], [x1 - x0, (y1 - y0) - ty, dz])]
    mount_dim_y = p["mount_dim_y"]
    if p["has_side_table"]:
        sy1, L = p["side_y_max"], p["side_length"]
        sdx = L * p["side_task_scalar"]
        task.append(([x0 - sdx / 2, (sy1 + y0) / 2, z], [sdx, sy1 - y0, dz]))
        free.append(([((x0 - L) + (x0 - sdx)) / 2, (sy1 + y0) / 2, z], [L - sdx, sy1 - y0, dz]))
        mount_dim_y = 2 * (p["mount_y"] - sy1)
    free.append(([p["mount_x"], p["mount_y"], -0.01], [2 * (x0 - p["mount_x"]), mount_dim_y, 0.02]))
    return task, free


def _footprint_distance(obj, x, y) -> float:
    """Distance of (x, y) to the footprint of ``obj`` = ("cylinder", cx, cy, radius) or ("cuboid", cx, cy, dx, dy, yaw): what the
    reference's 3-D ``sdf`` gives for a point in the plane of the objects' bottom faces wherever it is positive."""
    dx, dy = x - obj[1], y - obj[2]
    if obj[0] == "cylinder":
        return math.hypot(dx, dy) - obj[3]
    c, s = math.cos(obj[5]), math.sin(obj[5])
    qx, qy = abs(c * dx + s * dy) - obj[3] / 2, abs(c * dy - s * dx) - obj[4] / 2
    return math.hypot(max(qx, 0.0), max(qy, 0.0)) + min(max(qx, qy), 0.0)


def _place_objects(points, how_many: int, new_object, distance=_footprint_distance):
    """``place_objects`` (tabletop_environment.py:129-153): walk the candidate points in order while fewer than ``how_many``
    objects stand; a candidate is accepted when every object's distance to it is above 0.05, and ``new_object(x, y, m)`` is
    handed the least of them (1000 with nothing placed); None from it: the object found no row, is not counted and blocks
    nothing.  -> (objects, accepted candidate indices, the clearances handed over)."""
    objects, accepted, clearances = [], [], []
    for i, (x, y) in enumerate(points):
        if len(objects) >= how_many:
            break
        d = [distance(o, x, y) for o in objects]
        if all(v > 0.05 for v in d):
            m = min(d, default=1000.0)
            o = new_object(x, y, m)
            if o is not None:
                objects.append(o), accepted.append(i), clearances.append(m)
    return objects, accepted, clearances


def _tabletop_reference(rng, M1, M2, supports=None):
    assert M1 >= 7, "the reference's scenes need M1 >= 7 (five tables; a cubby's seven plates)"
    cc, cd, cq = np.zeros((M1, 3)), np.zeros((M1, 3)), np.tile([1.0, 0, 0, 0], (M1, 1))
    yc, yr, yh, yq = np.zeros((M2, 3)), np.zeros((M2, 1)), np.zeros((M2, 1)), np.tile([1.0, 0, 0, 0], (M2, 1))
    p = _tabletop_reference_parameters(rng)
    task, free = _tabletop_reference_tables(p)
    for n, (c, d) in enumerate(task + free):  # (the reference's ``obstacles`` order: task tables, free tables, mount table)
        cc[n], cd[n] = c, d
        if n < len(task):
            _support(supports, SUPPORT_SURFACE, c, d, cq[n], 0.0, d[0] * d[1])
    T = len(task) + len(free)
    K = int(rng.integers(3, 15))
    area = np.array([d[0] * d[1] for _, d in task])
    which = (rng.random(10 * K)[:, None] * area.sum() >= np.cumsum(area)[None]).sum(1).clip(max=len(task) - 1)
    uv = rng.random((10 * K, 2))
    lo = np.array([[c[0] - d[0] / 2, c[1] - d[1] / 2] for c, d in task])[which]
    points = lo + uv * np.array([d[:2] for _, d in task])[which]
    count = {"cuboid": T, "cylinder": 0}

    def new_object(x, y, m):
        xy_max = min(m, 0.15)
        if rng.random() < 0.3:
            r, hh = rng.uniform(0.05, xy_max), rng.uniform(0.05, 0.35)
            if count["cylinder"] >= M2:
                return None
            i = count["cylinder"]
            yc[i], yr[i], yh[i] = [x, y, p["height"] + hh / 2], r, hh
            count["cylinder"] += 1
            return ("cylinder", x, y, r)
        d = np.array([rng.uniform(0.05, xy_max), rng.uniform(0.05, xy_max), rng.uniform(0.05, 0.35)])
        yaw = rng.uniform(0, np.pi / 2)
        if count["cuboid"] >= M1:
            return None
        i = count["cuboid"]
        cc[i], cd[i], cq[i] = [x, y, p["height"] + d[2] / 2], d, _yaw_quat(yaw)
        count["cuboid"] += 1
        return ("cuboid", x, y, d[0], d[1], yaw)

    _place_objects(points, K, new_object)
    return cc, cd, cq, yc, yr, yh, yq


def _cubby_reference_parameters(rng) -> Dict[str, float]:
    """Stage 1 of ``Cubby.__init__`` (cubby_environment.py:62-74): the twelve parameters (the two plate thicknesses a merge
    zeroes start as the cubby's)."""
    p = dict(left=rng.uniform(0.6, 0.8), right=rng.uniform(-0.8, -0.6), bottom=rng.uniform(0.1, 0.3), front=rng.uniform(0.45, 0.65))
    p["back"] = p["front"] + rng.uniform(0.15, 0.55)
    p.update(top=rng.uniform(0.6, 0.8), mid_h_z=rng.uniform(0.35, 0.55), mid_v_y=rng.uniform(-0.1, 0.1),
             thickness=rng.uniform(0.01, 0.03))
    p.update(middle_shelf_thickness=p["thickness"], center_wall_thickness=p["thickness"],
             rotation=rng.uniform(-np.pi / 18, np.pi / 18))
    return p


def check_merge_pockets(pair):
    """(-1, -1): unmerged; otherwise a pair of distinct pockets in 0..3 -- anything else is refused."""
    a, b = int(pair[0]), int(pair[1])
    if (a, b) != (-1, -1) and not (0 <= a <= 3 and 0 <= b <= 3 and a != b):
        raise ValueError(f"merge_pockets must be (-1, -1) or a pair of distinct pockets in 0..3, got {(a, b)}")
    return a, b


def merged_cubby_parameters(p: Dict[str, float], pair) -> Dict[str, float]:
    """``MergedCubbyEnvironment.gen``'s rule (cubby_environment.py:679-686): the middle shelf goes when the two pockets lie on
    different levels, the centre wall when they lie on different sides."""
    a, b = check_merge_pockets(pair)
    p = dict(p)
    if a >= 0 and (a >> 1) != (b >> 1):
        p["middle_shelf_thickness"] = 0.0
    if a >= 0 and (a & 1) != (b & 1):
        p["center_wall_thickness"] = 0.0
    return p


def merged_support_index(pocket: int, p: Dict[str, float]) -> int:
    """The support row an original pocket (2 level + side) lies in after the merge ``p`` carries."""
    no_shelf, no_wall = p["middle_shelf_thickness"] == 0.0, p["center_wall_thickness"] == 0.0
    return 0 if no_shelf and no_wall else pocket >> 1 if no_wall else pocket & 1 if no_shelf else pocket


def _cubby_reference_primitives(p: Dict[str, float]):
    """Stage 2: -> (plates, supports), each a list of (centre, dims) in the world, and the yaw all of them share.  Plates in
    the reference's order -- back, bottom, top, right, left, centre wall, middle shelf -- with a plate of thickness 0 DROPPED
    (the reference keeps a zero-thickness cuboid that its own consumers mask); supports: ``support_volumes``' branches."""
    L, R, Bo, F, Ba, To, mz, my, t = (p[k] for k in ("left", "right", "bottom", "front", "back", "top", "mid_h_z", "mid_v_y", "thickness"))
    px, py, pz = (F + Ba) / 2, (L + R) / 2, (To + Bo) / 2
    yaw = p["rotation"]
    c, s = np.cos(yaw), np.sin(yaw)

    def world(l):
        ax, ay = l[0] - px, l[1] - py
        return [(c * ax - s * ay) + px, (s * ax + c * ay) + py, l[2]]

    plates = [([Ba, py, To / 2], [t, L - R, To]), ([px, py, Bo], [Ba - F, L - R, t]), ([px, py, To], [Ba - F, L - R, t]),
              ([px, R, pz], [Ba - F, t, (To - Bo) + t]), ([px, L, pz], [Ba - F, t, (To - Bo) + t])]
    no_wall, no_shelf = p["center_wall_thickness"] == 0.0, p["middle_shelf_thickness"] == 0.0
    if not no_wall:
        plates.append(([px, my, pz], [Ba - F, p["center_wall_thickness"], (To - Bo) + t]))
    if not no_shelf:
        plates.append(([px, py, mz], [Ba - F, L - R, p["middle_shelf_thickness"]]))
    levels = [(Bo, To)] if no_shelf else [(mz, To), (Bo, mz)]
    sides = [(R, L)] if no_wall else [(my, L), (R, my)]
    pockets = [([px, (ya + yb) / 2, (za + zb) / 2], [Ba - F, yb - ya, zb - za]) for za, zb in levels for ya, yb in sides]
    return [(world(l), d) for l, d in plates], [(world(l), d) for l, d in pockets], yaw


def _cubby_reference(rng, M1, M2, supports=None, merge=(-1, -1)):
    """``merge``: the pocket pair of a merged cubby ((-1, -1): unmerged); None: drawn from the six unordered pairs with one
    more uniform, AFTER the cubby's own draws (so the cubby of a seed does not depend on it)."""
    assert M1 >= 7, "a cubby has seven plates: M1 >= 7"
    cc, cd, cq = np.zeros((M1, 3)), np.zeros((M1, 3)), np.tile([1.0, 0, 0, 0], (M1, 1))
    yc, yr, yh, yq = np.zeros((M2, 3)), np.zeros((M2, 1)), np.zeros((M2, 1)), np.tile([1.0, 0, 0, 0], (M2, 1))
    p = _cubby_reference_parameters(rng)
    if merge is None:
        merge = MERGE_PAIRS[min(int(rng.random() * 6), 5)]
    plates, pockets, yaw = _cubby_reference_primitives(merged_cubby_parameters(p, merge))
    for i, (c, d) in enumerate(plates):
        cc[i], cd[i], cq[i] = c, d, _yaw_quat(yaw)
    for c, d in pockets:
        _support(supports, SUPPORT_VOLUME, c, d, _yaw_quat(yaw), 0.0, 1.0)
    return cc, cd, cq, yc, yr, yh, yq


def _merged_cubby(rng, M1, M2, supports=None, merge=None):
    return _cubby_reference(rng, M1, M2, supports, merge)


_GENERATORS = {"tabletop": _tabletop, "cubby": _cubby, "dresser": _dresser, "tabletop_reference": _tabletop_reference,
               "cubby_reference": _cubby_reference, "merged_cubby": _merged_cubby}
REFERENCE_KINDS = ("tabletop_reference", "cubby_reference", "merged_cubby")


def _scene_arrays(B: int, seed: int, kinds, M1: int, M2: int, S: Optional[int] = None, merge_pockets=None) -> Dict[str, np.ndarray]:
    """``make_scenes`` (``S`` None) and ``make_task_scenes``: one rng, one walk over the generators."""
    if merge_pockets is not None:
        merge_pockets = [check_merge_pockets(pair) for pair in np.asarray(merge_pockets).reshape(B, 2)]
    rng = np.random.default_rng(seed)
    out = [[] for _ in range(7)]
    boxes = np.zeros((B, S or 0, 12), np.float32)
    boxes[..., 6] = 1.0  # (padding: zero dims, the identity quaternion, weight 0)
    kind = np.zeros((B, S or 0), np.int32)
    for b in range(B):
        supports = None if S is None else []
        name = kinds[b % len(kinds)]
        if name == "merged_cubby":  # (the pair of scene b; None: the scene draws its own)
            parts = _merged_cubby(rng, M1, M2, supports, None if merge_pockets is None else merge_pockets[b])
        else:
            parts = _GENERATORS[name](rng, M1, M2, supports)
        for o, p in zip(out, parts):
            o.append(p)
        for i, (k, row) in enumerate((supports or [])[:S]):
            kind[b, i], boxes[b, i] = k, row
    names = ["cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii",
             "cylinder_heights", "cylinder_quats"]
    arrays = {k: np.asarray(v, dtype=np.float32) for k, v in zip(names, out)}
    if S is not None:
        arrays.update(support_boxes=boxes, support_kind=kind)
    return arrays


def make_scenes(B: int, seed: int = 0, kinds=("tabletop",), M1: int = 16, M2: int = 16, merge_pockets=None) -> Dict[str, np.ndarray]:
    """-> float32 arrays cuboid_{centers,dims,quats} [B,M1,*], cylinder_{centers,radii,heights,quats} [B,M2,*].
    ``merge_pockets`` (int [B,2]; read by "merged_cubby" scenes alone): the pocket pair of scene b, (-1, -1) unmerged; None:
    every merged cubby draws its pair."""
    return _scene_arrays(B, seed, kinds, M1, M2, merge_pockets=merge_pockets)


def make_task_scenes(B: int, seed: int = 0, kinds=("tabletop",), M1: int = 16, M2: int = 16, S: int = 8,
                     merge_pockets=None) -> Dict[str, np.ndarray]:
    """``make_scenes``' arrays, bit for bit (the supports cost no draw of the rng), plus where each scene can be worked on:
    ``support_boxes`` float32 [B,S,12] -- centre (3), dims (3), quaternion w x y z (4), ``approach`` (the world yaw of the axis
    the gripper reaches along) and ``weight`` -- and ``support_kind`` int32 [B,S]: 0 padding (zero dims, the identity
    quaternion, weight 0, like the primitive padding), 1 a surface (the top face of the box), 2 a volume.  What
    ``solvers.task_candidates`` draws from, and what the reference's ``check_final_region`` judges by.

    * tabletop: the front table and the side table, when present, are surfaces (the reference's ``clear_tables``; the mount
      table under the robot is not one); weight = the top face's area, ``approach`` unused (0).
    * cubby: the four pockets are volumes, each the interior between the shelves and walls that bound it; the quaternion is
      the cubby's yaw, weight 1, ``approach`` 0: the world x axis, which the reference uses and this cubby's opening faces.
    * dresser: a STAND-IN with no reference counterpart (this dresser is "dresser-like", not the reference's recursive one):
      one volume per plate, the free space above it inside its cell; ``approach`` is the horizontal direction along the
      plate's depth axis that has a positive world-x component (the reach runs from the robot inward), weight 1.  With more
      plates than ``S`` the first ``S`` are kept.
    * tabletop_reference: the TASK tables (front, then side where it stands) are surfaces, weight = the top face's area; the
      free tables and the mount table are not supports.
    * cubby_reference: the four pockets of ``support_volumes``' last branch in its order, pocket 2 level + side with level 0
      the top and side 0 the +y side: volumes, ``approach`` 0, weight 1.
    * merged_cubby: the matching branch -- one whole volume, or [top row, bottom row], or [left column, right column];
      ``merged_support_index`` maps an original pocket to its row."""
    assert S >= 1
    return _scene_arrays(B, seed, kinds, M1, M2, S, merge_pockets)


# ``scene_kind``: 0..2 are ``mpx_scene_generate``'s, 3..5 ``mpx_scene_generate_reference``'s
SCENE_KIND_CODES = {"tabletop": 0, "cubby": 1, "dresser": 2, "tabletop_reference": 3, "cubby_reference": 4, "merged_cubby": 5}


def make_scenes_device(B: int, seed: int = 0, kinds=("tabletop",), M1: int = 16, M2: int = 16, S: Optional[int] = None,
                       device="cuda:0", env_offset: int = 0, scene_ids: Optional[torch.Tensor] = None,
                       merge_pockets=None) -> Dict[str, torch.Tensor]:
    """The scenes of ``make_scenes`` (``S`` None) or ``make_task_scenes`` (``S`` >= 1) drawn ON THE DEVICE
    (csrc/scene_gen.hip, ``mpx_scene_generate``): the same keys, shapes, dtypes, padding and DISTRIBUTIONS, as tensors on
    ``device``, every scene a function of ``(seed, scene id, kind, M1, M2, S)`` alone -- Philox stream 19 keyed by the scene
    id -- where the host generators walk one sequential rng.  A second source beside the host's, not a port of its stream:
    the same seed gives other scenes of the same distribution.  Scene b has id ``env_offset + b``, or ``scene_ids[b]``
    (int64 [B], any order, repeats allowed: the rows of a shard, the tiles of a ``scene_pool``); the kind of scene id g is
    ``kinds[g % len(kinds)]``, the host's rule.  3 <= M1 <= 64, 0 <= M2 <= 64, S <= 64.  Every element is written by the
    kernel; nothing is generated for a row that is not asked for.

    The kinds "tabletop_reference", "cubby_reference" and "merged_cubby" come from a second entry
    (csrc/scene_gen_reference.hip, ``mpx_scene_generate_reference``; they need M1 >= 7): a batch of old kinds alone calls the
    first entry alone, as before; one of new kinds alone the second alone; a mixed one the first, then the second on the same
    arrays (it leaves the rows of the old kinds untouched).  ``merge_pockets`` (int [B,2], read by "merged_cubby" rows alone):
    the pocket pair of row b, (-1, -1) unmerged; None: every merged cubby draws its pair.  Host values (a list, an array, a
    CPU tensor) that are neither are refused with a ``ValueError``; a tensor already on the device is not read back, and the
    kernel treats such a row as unmerged."""
    from . import _lib

    dev = torch.device(device)
    if merge_pockets is not None and not (isinstance(merge_pockets, torch.Tensor) and merge_pockets.is_cuda):
        merge_pockets = torch.as_tensor(np.asarray(merge_pockets)).reshape(-1, 2)
        for pair in merge_pockets.tolist():
            check_merge_pockets(pair)
    codes = torch.tensor([SCENE_KIND_CODES[k] for k in kinds], dtype=torch.int32)
    if scene_ids is None:
        ids = None
        kind = codes[(int(env_offset) + torch.arange(B, dtype=torch.int64)) % len(kinds)].to(dev)
    else:
        ids = scene_ids.to(device=dev, dtype=torch.int64).contiguous()
        if ids.shape != (B,):
            raise _lib.MpxError(f"make_scenes_device: scene_ids must be [B] = [{B}], got {tuple(ids.shape)}")
        kind = codes.to(dev)[ids % len(kinds)]
    _lib.require_cuda(kind, ids)

    def empty(*shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)

    out = {"cuboid_centers": empty(B, M1, 3), "cuboid_dims": empty(B, M1, 3), "cuboid_quats": empty(B, M1, 4),
           "cylinder_centers": empty(B, M2, 3), "cylinder_radii": empty(B, M2, 1), "cylinder_heights": empty(B, M2, 1),
           "cylinder_quats": empty(B, M2, 4)}
    if S is not None:
        out.update(support_boxes=empty(B, S, 12), support_kind=empty(B, S, dtype=torch.int32))
    tail = (B, M1, M2, 0 if S is None else S, int(seed) & (2 ** 64 - 1), int(env_offset),
            *(_lib.ptr(out[k]) for k in ("cuboid_centers", "cuboid_dims", "cuboid_quats", "cylinder_centers", "cylinder_radii",
                                         "cylinder_heights", "cylinder_quats")),
            _lib.ptr(out.get("support_boxes")), _lib.ptr(out.get("support_kind")))
    new = [k in REFERENCE_KINDS for k in kinds]
    if not all(new):
        _lib.call("mpx_scene_generate", _lib.ptr(kind), _lib.ptr(ids), *tail)
    if any(new):
        pockets = None
        if merge_pockets is not None:
            pockets = merge_pockets.to(device=dev, dtype=torch.int32).contiguous()
            if pockets.shape != (B, 2):
                raise _lib.MpxError(f"make_scenes_device: merge_pockets must be [B,2] = [{B},2], got {tuple(pockets.shape)}")
            _lib.require_cuda(pockets)
        _lib.call("mpx_scene_generate_reference", _lib.ptr(kind), _lib.ptr(ids), _lib.ptr(pockets), *tail)
    return out


def sample_scene_clouds_host(scn: Dict[str, np.ndarray], num_points: int, seed: int = 0) -> np.ndarray:
    """Vectorised area-proportional surface sampling of every environment's primitives (NumPy).

    Distributionally equivalent to ``construct_mixed_point_cloud`` (geometry.py:571-608): each
    point picks an unmasked primitive with probability proportional to its surface area and is
    uniform on that surface.  -> float32 [B, num_points, 3].  Host-side set-up code (the batched
    device sampler is part of the S3 row).  All uniforms come from ONE array drawn scene by scene,
    so the cloud of scene b does not depend on how many scenes follow it (a shard that generates a prefix of the
    scenes gets the same clouds as a process that generates them all).
    """
    rng = np.random.default_rng(seed)
    U = rng.random((scn["cuboid_dims"].shape[0], num_points, 10))
    cd, yr, yh = scn["cuboid_dims"].astype(np.float64), scn["cylinder_radii"][..., 0].astype(np.float64), \
        scn["cylinder_heights"][..., 0].astype(np.float64)
    B, M1 = cd.shape[:2]
    M2 = yr.shape[1]
    cub_area = 2 * (cd[..., 0] * cd[..., 1] + cd[..., 0] * cd[..., 2] + cd[..., 1] * cd[..., 2])
    cub_area[(np.abs(cd) <= 1e-8).any(-1)] = 0
    cyl_area = 2 * np.pi * yr * yh + 2 * np.pi * yr**2
    cyl_area[(np.abs(yr) <= 1e-8) | (np.abs(yh) <= 1e-8)] = 0
    area = np.concatenate([cub_area, cyl_area], axis=1)
    cdf = np.cumsum(area, axis=1)
    u = U[..., 0] * cdf[:, -1:]
    prim = np.minimum((u[:, :, None] >= cdf[:, None, :]).sum(-1), M1 + M2 - 1)  # [B,P]
    bi = np.arange(B)[:, None]
    is_cyl = prim >= M1
    ci = np.minimum(prim, M1 - 1)
    yi = np.clip(prim - M1, 0, M2 - 1)
    # cuboid samples
    d = cd[bi, ci]
    face_area = np.stack([d[..., 1] * d[..., 2], d[..., 0] * d[..., 2], d[..., 0] * d[..., 1]], -1)
    fc = np.cumsum(face_area, -1)
    uf = U[..., 1] * fc[..., -1]
    axis = np.minimum((uf[..., None] >= fc).sum(-1), 2)
    p = (U[..., 2:5] - 0.5) * d
    sign = np.where(U[..., 5] < 0.5, -0.5, 0.5)
    np.put_along_axis(p, axis[..., None], (sign * np.take_along_axis(d, axis[..., None], -1)[..., 0])[..., None], -1)
    # cylinder samples
    r, h = yr[bi, yi], yh[bi, yi]
    side, cap = 2 * np.pi * r * h, np.pi * r**2
    uc = U[..., 6] * (side + 2 * cap + 1e-30)
    th = U[..., 7] * 2 * np.pi
    rho = np.where(uc < side, r, r * np.sqrt(U[..., 8]))
    z = np.where(uc < side, (U[..., 9] - 0.5) * h, np.where(uc < side + cap, -0.5 * h, 0.5 * h))
    pc = np.stack([rho * np.cos(th), rho * np.sin(th), z], -1)
    local = np.where(is_cyl[..., None], pc, p)
    quat = np.where(is_cyl[..., None], scn["cylinder_quats"][bi, yi], scn["cuboid_quats"][bi, ci]).astype(np.float64)
    ctr = np.where(is_cyl[..., None], scn["cylinder_centers"][bi, yi], scn["cuboid_centers"][bi, ci]).astype(np.float64)
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    w, x, y, zq = quat[..., 0], quat[..., 1], quat[..., 2], quat[..., 3]
    R = np.stack([
        np.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y)], -1),
        np.stack([2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x)], -1),
        np.stack([2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    world = np.einsum("bpij,bpj->bpi", R, local) + ctr
    return world.astype(np.float32)


def sample_scene_clouds(prims: Dict[str, torch.Tensor], num_points: int, seed: int, out: Optional[torch.Tensor] = None,
                        write_label: bool = False, return_aux: bool = False, scratch: Optional[tuple] = None,
                        env_offset: int = 0):
    """Device-side batched ``construct_mixed_point_cloud`` (geometry.py:571-608; csrc/scene.hip).

    ``prims``: cuboid_{centers,dims,quats} [B,M1,*], cylinder_{centers,radii,heights,quats} [B,M2,*] on the
    GPU (zero-volume rows are skipped like data_loader.py:248,256).  Writes ``out[:, :num_points, :3]``
    (``out`` may be a slab view ``xyz[:, 2048:6144]``; default: a fresh [B,N,3] tensor), plus the
    shuffled obstacle label in column 3 when ``write_label``.  Deterministic in (seed, GLOBAL environment id =
    ``env_offset`` + row): rank r of a sharded batch passes the id of its first environment and draws exactly what a
    single process would draw for those environments.
    """
    from . import _lib

    cc, cd, cq = (_lib.f32c(prims[k]) for k in ("cuboid_centers", "cuboid_dims", "cuboid_quats"))
    yc, yr, yh, yq = (_lib.f32c(prims[k]) for k in ("cylinder_centers", "cylinder_radii", "cylinder_heights",
                                                    "cylinder_quats"))
    _lib.require_cuda(cc, yc)
    B, M1 = cd.shape[:2]
    M2 = yr.shape[1]
    dev = cc.device
    if out is None:
        out = torch.empty((B, num_points, 4 if write_label else 3), dtype=torch.float32, device=dev)
    assert out.ndim == 3 and out.size(0) == B and out.size(1) >= num_points and out.stride(2) == 1
    if scratch is None:  # (assign, labels, nobs): callers that re-render every step keep them
        scratch = (torch.empty((B, num_points), dtype=torch.int16, device=dev),
                   torch.zeros((B, M1 + M2), dtype=torch.uint8, device=dev),
                   torch.zeros(B, dtype=torch.int32, device=dev))
    assign, labels, nobs = scratch
    for b0 in range(0, B, 65535):
        nb = min(65535, B - b0)
        sl = slice(b0, b0 + nb)
        _lib.call("mpx_scene_cloud", _lib.ptr(cc[sl]), _lib.ptr(cd[sl]), _lib.ptr(cq[sl]), M1, _lib.ptr(yc[sl]),
                  _lib.ptr(yr[sl]), _lib.ptr(yh[sl]), _lib.ptr(yq[sl]), M2, nb, num_points, int(seed) & (2 ** 64 - 1),
                  int(env_offset) + b0,
                  _lib.ptr(assign[sl]), _lib.ptr(labels[sl]), _lib.ptr(nobs[sl]), _lib.ptr(out[sl]), out.stride(0),
                  out.stride(1), int(write_label))
    if return_aux:
        return out, assign, labels, nobs
    return out


def random_configurations(B: int, seed: int = 0) -> np.ndarray:
    """q ~ U(joint limits), float32 [B,7] (C2 of BASELINE.json)."""
    rng = np.random.default_rng(seed + 1000003)
    lim = ft.JOINT_LIMITS_REAL
    return (lim[:, 0] + rng.random((B, 7)) * (lim[:, 1] - lim[:, 0])).astype(np.float32)


def linear_trajectories(B: int, T: int, seed: int = 0) -> np.ndarray:
    """[B,T,7]: straight joint-space lines between two random configurations (C4)."""
    a, b = random_configurations(B, seed), random_configurations(B, seed + 1)
    s = np.linspace(0.0, 1.0, T, dtype=np.float32)[None, :, None]
    return (a[:, None] * (1 - s) + b[:, None] * s).astype(np.float32)


def _collision_free_problems(prims: Dict[str, torch.Tensor], q_draw: torch.Tensor, q_target: torch.Tensor, seed: int,
                             env_offset: int, max_redraws: int):
    """``make_problem_batch(collision_free=True)``: -> start q, the configuration whose FK is the goal pose, the goal's
    collision-free solution and the ``valid`` mask.  Every draw is keyed by (seed, attempt, GLOBAL row), so a shard
    gets the rows one process would get."""
    from .geometry import TorchCuboids, TorchCylinders
    from .robot import franka_fk, franka_ik, frames_to_matrix

    B, dev = q_draw.size(0), q_draw.device
    cub = TorchCuboids(prims["cuboid_centers"], prims["cuboid_dims"], prims["cuboid_quats"])
    cyl = TorchCylinders(prims["cylinder_centers"], prims["cylinder_radii"], prims["cylinder_heights"],
                         prims["cylinder_quats"])

    def pose(qq):
        return frames_to_matrix(franka_fk(qq)[:, ft.LINK_ID["right_gripper"]])

    q_start, q_goal, q_pose = q_draw.clone(), torch.full_like(q_target, float("nan")), q_target.clone()
    valid = torch.zeros(B, dtype=torch.bool, device=dev)
    # (every attempt solves all B rows, not only the still invalid ones: the draws are keyed by the global row, a launch
    # over 8192 problems takes 1.4 ms, and a gather would have to carry the row ids into the kernel)
    for a in range(max_redraws + 1):
        s_a = seed + 7919 * a
        src_start = q_draw if a == 0 else torch.from_numpy(random_configurations(env_offset + B, s_a)[env_offset:]).to(dev)
        src_goal = q_target if a == 0 else torch.from_numpy(random_configurations(env_offset + B, s_a + 7)[env_offset:]).to(dev)
        qs, ss = franka_ik(pose(src_start), cub, cyl, seed=s_a, env_offset=env_offset)
        qg, sg = franka_ik(pose(src_goal), cub, cyl, seed=s_a + 7, env_offset=env_offset)
        ok = (ss == 0) & (sg == 0) & ~valid
        q_start[ok], q_goal[ok], q_pose[ok] = qs[ok], qg[ok], src_goal[ok]
        valid |= ok
        if B == 0 or bool(valid.all()):
            break
    return q_start, q_pose, q_goal, valid


TASK_CANDIDATES = 8  # free gripper poses per start and per goal that ``problems="task"`` hands to the IK, in draw order


def _task_problems(prims: Dict[str, torch.Tensor], support_boxes: torch.Tensor, support_kind: torch.Tensor, q_draw: torch.Tensor,
                   q_target: torch.Tensor, seed: int, env_offset: int):
    """``make_problem_batch(problems="task")``: start and goal are the reference's task-oriented candidates -- per role the
    first of ``solvers.task_candidates``' free gripper poses (draw order) that ``franka_ik`` solves against the scene: "the
    first free gripper pose that has an IK solution" of up to 100 draws.  In a scene of volumes the goal is drawn with the
    start's support excluded (different pockets).  Every draw is keyed by (seed, role, candidate, GLOBAL row): shards agree.
    -> start q, goal q (NaN rows where invalid), ``valid``, and per role the chosen pose [B,4,4] (NaN) and support (-1)."""
    from .geometry import TorchCuboids, TorchCylinders
    from .solvers import franka_ik, task_candidates

    B, dev = q_draw.size(0), q_draw.device
    cub = TorchCuboids(prims["cuboid_centers"], prims["cuboid_dims"], prims["cuboid_quats"])
    cyl = TorchCylinders(prims["cylinder_centers"], prims["cylinder_radii"], prims["cylinder_heights"],
                         prims["cylinder_quats"])
    eye = torch.eye(4, dtype=torch.float32, device=dev)

    def first_solved(role, exclude):
        poses, _, support, count = task_candidates(support_boxes, support_kind, cub, cyl, C=TASK_CANDIDATES, seed=seed,
                                                   env_offset=env_offset, role=role, exclude=exclude)
        q = torch.full((B, 7), float("nan"), dtype=torch.float32, device=dev)
        pose = torch.full((B, 4, 4), float("nan"), dtype=torch.float32, device=dev)
        chosen = torch.full((B,), -1, dtype=torch.int32, device=dev)
        found = torch.zeros(B, dtype=torch.bool, device=dev)
        for c in range(TASK_CANDIDATES):
            live = count > c  # (a row past ``count`` is NaN: the IK is handed the identity there and its answer dropped)
            target = torch.where(live[:, None, None], poses[:, c], eye).contiguous()
            qc, sc = franka_ik(target, cub, cyl, seed=seed + 7919 * (1 + TASK_CANDIDATES * role + c), env_offset=env_offset)
            ok = live & (sc == 0) & ~found
            q[ok], pose[ok], chosen[ok] = qc[ok], poses[ok, c], support[ok, c]
            found |= ok
            if B == 0 or bool((found | (count <= c + 1)).all()):
                break
        return q, pose, chosen, found

    q_s, pose_s, sup_s, ok_s = first_solved(0, None)
    volumes = (support_kind == SUPPORT_VOLUME).any(1)
    q_g, pose_g, sup_g, ok_g = first_solved(1, torch.where(volumes & ok_s, sup_s, torch.full_like(sup_s, -1)))
    valid = ok_s & ok_g
    nan = float("nan")
    q_start = torch.where(valid[:, None], q_s, q_draw)  # (invalid rows keep their unchecked uniform draw, as "uniform" does)
    q_goal = torch.where(valid[:, None], q_g, torch.full_like(q_g, nan))
    start_pose = torch.where(valid[:, None, None], pose_s, torch.full_like(pose_s, nan))
    goal_pose = torch.where(valid[:, None, None], pose_g, torch.full_like(pose_g, nan))
    target_support = torch.where(valid, sup_g, torch.full_like(sup_g, -1))
    return q_start, q_goal, valid, start_pose, goal_pose, target_support


def _merge_task_rows(out: Dict[str, torch.Tensor], kinds, sid: np.ndarray, valid: torch.Tensor, start_pose: torch.Tensor,
                     goal_pose: torch.Tensor, target_support: torch.Tensor, seed: int, M1: int, M2: int, dev) -> torch.Tensor:
    """``MergedCubbyEnvironment.gen`` per row (cubby_environment.py:666-704): the merged-cubby rows of the batch were generated
    UNMERGED and their start and goal drawn in different pockets; here every VALID one of them is generated again with those
    two pockets as its pair -- the same cubby (same id and seed) without the plates between them -- and written over the
    row's primitives and supports in ``out``.  Invalid rows stay unmerged.  The pockets are found as the reference finds
    them, by which unmerged support holds the pose's position.  -> ``target_support`` mapped to the merged supports.
    Everything computed afterwards (the region keys, the experts, the followers, the scene cloud) sees the merged scene; the
    reference leaves its candidates' negative volumes stale after the merge, here they follow from the merged supports."""
    S = out["support_kind"].shape[1]
    is_merged = torch.from_numpy(np.asarray([kinds[g % len(kinds)] == "merged_cubby" for g in sid], bool)).to(dev)
    rows = is_merged & valid
    boxes = out["support_boxes"]

    def pocket_of(pose):  # the unmerged pocket that holds the position (-1: none; the goal's is ``target_support``)
        local = pose[:, None, :3, 3] - boxes[..., :3]
        c, s = 1 - 2 * boxes[..., 9] ** 2, 2 * boxes[..., 6] * boxes[..., 9]  # (cos, sin of the yaw of (w, 0, 0, z))
        lx, ly = c * local[..., 0] + s * local[..., 1], c * local[..., 1] - s * local[..., 0]
        inside = (lx.abs() <= boxes[..., 3] / 2) & (ly.abs() <= boxes[..., 4] / 2) & (local[..., 2].abs() <= boxes[..., 5] / 2)
        inside &= out["support_kind"] == SUPPORT_VOLUME
        return torch.where(inside.any(1), inside.float().argmax(1), torch.full_like(inside[:, 0], -1, dtype=torch.int64))

    a, b = pocket_of(start_pose), target_support.long()
    rows &= (a >= 0) & (b >= 0) & (a != b) & (a < 4) & (b < 4)
    pair = torch.where(rows[:, None], torch.stack([a, b], 1), torch.full((len(sid), 2), -1, dtype=torch.int64, device=dev)).int()
    merged = make_scenes_device(len(sid), seed, kinds, M1, M2, S=S, device=dev, scene_ids=torch.from_numpy(sid), merge_pockets=pair)
    for key, v in merged.items():
        out[key] = torch.where(rows.reshape((-1,) + (1,) * (v.dim() - 1)), v, out[key])
    no_shelf, no_wall = (a >> 1) != (b >> 1), (a & 1) != (b & 1)
    mapped = torch.where(no_shelf & no_wall, torch.zeros_like(b), torch.where(no_wall, b >> 1, b & 1))
    return torch.where(rows, mapped.to(target_support.dtype), target_support)


def _task_region_keys(support_boxes: torch.Tensor, support_kind: torch.Tensor, target_support: torch.Tensor) -> Dict[str, torch.Tensor]:
    """What the reference's inference problems carry for ``check_final_region``: ``target_volume`` [B,10] (centre, dims,
    quaternion w x y z of the goal's support; NaN where it is a surface or the row is invalid) and
    ``target_negative_volumes`` [B,S,10] (the OTHER live volume supports of the scene; NaN rows elsewhere)."""
    B, S = support_kind.shape
    nan = float("nan")
    ts = target_support.long()
    at = ts.clamp(min=0)
    rows = torch.arange(B, device=support_kind.device)
    is_volume = (ts >= 0) & (support_kind[rows, at] == SUPPORT_VOLUME)
    volume = torch.where(is_volume[:, None], support_boxes[rows, at, :10], torch.full((B, 10), nan, device=support_boxes.device))
    other = (support_kind == SUPPORT_VOLUME) & (torch.arange(S, device=ts.device)[None] != ts[:, None]) & (ts >= 0)[:, None]
    negative = torch.where(other[..., None], support_boxes[..., :10], torch.full_like(support_boxes[..., :10], nan))
    return {"target_volume": volume, "target_negative_volumes": negative}


EXPERT_LENGTH = 50  # the reference's SEQUENCE_LENGTH (data_pipeline/gen_data.py)


def _expert_trajectories(prims: Dict[str, torch.Tensor], q_start: torch.Tensor, q_goal: torch.Tensor, valid: torch.Tensor,
                         seed: int, env_offset: int, roadmap: bool = False, shortcut: bool = False) -> Dict[str, torch.Tensor]:
    from .geometry import TorchCuboids, TorchCylinders
    from .solvers import franka_plan, franka_plan_global

    cub = TorchCuboids(prims["cuboid_centers"], prims["cuboid_dims"], prims["cuboid_quats"])
    cyl = TorchCylinders(prims["cylinder_centers"], prims["cylinder_radii"], prims["cylinder_heights"],
                         prims["cylinder_quats"])
    # (invalid rows have a NaN goal: the kernel reports status 2 and writes a NaN row for them)
    if roadmap:  # ``expert_from="roadmap"``: the same planner with the roadmap's path as one more candidate
        traj, status, _ = franka_plan_global(q_start, q_goal, cub, cyl, T=EXPERT_LENGTH, seed=seed, env_offset=env_offset,
                                             shortcut=True if shortcut else None)
    else:
        traj, status = franka_plan(q_start, q_goal, cub, cyl, T=EXPERT_LENGTH, seed=seed, env_offset=env_offset)
    return {"global_solutions": traj, "expert_valid": valid & (status == 0)}


EXPERT_CLOUD_POINT_RADIUS = 0.02  # [m] about half the spacing of 4096 points on a scene's surfaces


def _expert_trajectories_cloud(scene_cloud: torch.Tensor, q_start: torch.Tensor, q_goal: torch.Tensor, valid: torch.Tensor,
                               seed: int, env_offset: int, point_radius: float, roadmap: bool = False,
                               shortcut: bool = False) -> Dict[str, torch.Tensor]:
    """``expert_from="cloud"``: the demonstration is planned against the batch's own scene cloud (a view of the slab),
    with ``solvers.franka_plan_cloud``; valid means free by ``FrankaCollisionSampler.check_cloud`` at ``point_radius``.
    ``roadmap`` (``expert_from="cloud_roadmap"``): with ``solvers.franka_plan_global_cloud``, the same planner with a lazy
    roadmap's path as one more candidate; ``shortcut``: and that path shortcut as another, in front of it."""
    from .solvers import franka_plan_cloud, franka_plan_global_cloud

    if roadmap:
        traj, status, _ = franka_plan_global_cloud(q_start, q_goal, scene_cloud, point_radius=point_radius, T=EXPERT_LENGTH,
                                                   seed=seed, env_offset=env_offset, shortcut=True if shortcut else None)
    else:
        traj, status = franka_plan_cloud(q_start, q_goal, scene_cloud, point_radius=point_radius, T=EXPERT_LENGTH, seed=seed,
                                         env_offset=env_offset)
    return {"global_solutions": traj, "expert_valid": valid & (status == 0)}


HYBRID_GUIDE_POSES = 8  # guide poses handed to the follower: waypoints round(i * 49 / 8), i = 1..8, of the global plan


def _hybrid_trajectories(prims: Dict[str, torch.Tensor], q_start: torch.Tensor, global_solutions: torch.Tensor,
                         expert_valid: torch.Tensor, q_goal: Optional[torch.Tensor] = None, seed: int = 0,
                         env_offset: int = 0, gripper_guide: bool = False, shortcut=False) -> Dict[str, torch.Tensor]:
    """``hybrid=True``: the global plan steers, the follower produces.  ``solvers.franka_follow`` (a stand-in for the
    reference's Geometric Fabrics expert, NOT Lula: gen_data.py:156-307) follows the right_gripper poses of eight waypoints
    of ``global_solutions``, its dense path is retimed to 50 waypoints and judged; the target becomes the pose the
    trajectory actually ends at (hindsight goal revision, gen_data.py:303-306).  Rows without a global solution hand NaN
    poses to the follower and come back with status 2.

    ``gripper_guide`` (``hybrid_guide="gripper"``): the guide is not read off the global plan but planned for the free-flying
    gripper through the same primitives by ``solvers.gripper_roadmap`` (a stand-in for the reference's OMPL end-effector
    planner, gen_data.py:156-189, NOT a port of it), from the right_gripper pose of ``q_start`` to that of ``q_goal``, keyed
    by the batch's ``seed`` / ``env_offset``.  There is no fall-back to the global guide: a row without a gripper path hands
    NaN poses to the follower (the reference drops such rows too: "end effector path").  ``shortcut`` (True or a dict of
    ``solvers.gripper_shortcut``'s options; only with ``gripper_guide``): the roadmap's path is shortcut by
    ``solvers.gripper_plan`` before it is resampled to the guide poses."""
    from .geometry import TorchCuboids, TorchCylinders
    from .robot import franka_fk, frames_to_matrix
    from .solvers import franka_follow, gripper_plan, gripper_roadmap

    cub = TorchCuboids(prims["cuboid_centers"], prims["cuboid_dims"], prims["cuboid_quats"])
    cyl = TorchCylinders(prims["cylinder_centers"], prims["cylinder_radii"], prims["cylinder_heights"],
                         prims["cylinder_quats"])
    B = q_start.size(0)
    at = [int(round(i * (EXPERT_LENGTH - 1) / HYBRID_GUIDE_POSES)) for i in range(1, HYBRID_GUIDE_POSES + 1)]
    gripper = ft.LINK_ID["right_gripper"]
    extra = {}
    if gripper_guide:
        ends = frames_to_matrix(franka_fk(torch.cat([q_start, q_goal]))[:, gripper])  # (an invalid row's NaN goal: status 2)
        if shortcut:
            guide, guide_status = gripper_plan(ends[:B].contiguous(), ends[B:].contiguous(), cub, cyl, W=HYBRID_GUIDE_POSES,
                                               seed=seed, env_offset=env_offset, shortcut=shortcut)
        else:
            guide, guide_status = gripper_roadmap(ends[:B].contiguous(), ends[B:].contiguous(), cub, cyl, W=HYBRID_GUIDE_POSES,
                                                  seed=seed, env_offset=env_offset)
        extra = {"hybrid_guide_poses": guide, "hybrid_guide_status": guide_status}
    else:
        guide = frames_to_matrix(franka_fk(global_solutions[:, at].reshape(-1, 7))[:, gripper]).reshape(B, len(at), 4, 4)
    traj, status, _, _ = franka_follow(q_start, guide, cub, cyl, T=EXPERT_LENGTH)
    return dict(extra, hybrid_solutions=traj, hybrid_valid=expert_valid & (status == 0),
                hybrid_target_pose=frames_to_matrix(franka_fk(traj[:, -1].contiguous())[:, gripper]))


def _hybrid_trajectories_cloud(scene_cloud: torch.Tensor, q_start: torch.Tensor, global_solutions: torch.Tensor,
                               expert_valid: torch.Tensor, point_radius: float, q_goal: Optional[torch.Tensor] = None,
                               seed: int = 0, env_offset: int = 0, gripper_guide: bool = False,
                               shortcut=False) -> Dict[str, torch.Tensor]:
    """``hybrid_against="cloud"``: ``_hybrid_trajectories`` with ``solvers.franka_follow_cloud`` (still the stand-in for the
    reference's Geometric Fabrics expert, NOT Lula) following the same eight right_gripper poses of the cloud plan against
    the batch's own scene cloud, at the expert's ``point_radius``: the cloud's distance field steers, ``check_cloud``'s test
    judges, so ``hybrid_valid`` and ``expert_valid`` mean free by one and the same test.  One field is built here and
    handed to the follower.

    ``gripper_guide`` (``hybrid_guide="gripper_cloud"``): as in ``_hybrid_trajectories``, the guide is planned for the
    free-flying gripper, here by ``solvers.gripper_roadmap_cloud`` against the same scene cloud at the same ``point_radius``
    through that one field, from the right_gripper pose of ``q_start`` to that of ``q_goal``, keyed by the batch's ``seed`` /
    ``env_offset``.  No fall-back to the global guide: a row without a gripper path hands NaN poses to the follower.
    ``shortcut`` (True or a dict of ``solvers.gripper_shortcut_cloud``'s options; only with ``gripper_guide``): the roadmap's
    path is shortcut by ``solvers.gripper_plan_cloud``, through the same field, before it is resampled to the guide poses."""
    from .field import DEFAULT_VOXEL, CloudField
    from .robot import franka_fk, frames_to_matrix
    from .solvers import (FOLLOW_DEFAULTS, franka_follow_cloud, gripper_plan_cloud, gripper_roadmap_cloud,
                          plan_cloud_truncation)

    B = q_start.size(0)
    at = [int(round(i * (EXPERT_LENGTH - 1) / HYBRID_GUIDE_POSES)) for i in range(1, HYBRID_GUIDE_POSES + 1)]
    gripper = ft.LINK_ID["right_gripper"]
    field = CloudField.build(scene_cloud, None, truncation=plan_cloud_truncation(
        point_radius, FOLLOW_DEFAULTS["clearance"], FOLLOW_DEFAULTS["epsilon"], DEFAULT_VOXEL))
    extra = {}
    if gripper_guide:
        ends = frames_to_matrix(franka_fk(torch.cat([q_start, q_goal]))[:, gripper])  # (an invalid row's NaN goal: status 2)
        if shortcut:
            guide, guide_status = gripper_plan_cloud(ends[:B].contiguous(), ends[B:].contiguous(), scene_cloud, field=field,
                                                     point_radius=point_radius, W=HYBRID_GUIDE_POSES, seed=seed,
                                                     env_offset=env_offset, shortcut=shortcut)
        else:
            guide, guide_status = gripper_roadmap_cloud(ends[:B].contiguous(), ends[B:].contiguous(), scene_cloud, field=field,
                                                        point_radius=point_radius, W=HYBRID_GUIDE_POSES, seed=seed,
                                                        env_offset=env_offset)
        extra = {"hybrid_guide_poses": guide, "hybrid_guide_status": guide_status}
    else:
        guide = frames_to_matrix(franka_fk(global_solutions[:, at].reshape(-1, 7))[:, gripper]).reshape(B, len(at), 4, 4)
    traj, status, _, _ = franka_follow_cloud(q_start, guide, scene_cloud, field=field, point_radius=point_radius, T=EXPERT_LENGTH)
    return dict(extra, hybrid_solutions=traj, hybrid_valid=expert_valid & (status == 0),
                hybrid_target_pose=frames_to_matrix(franka_fk(traj[:, -1].contiguous())[:, gripper]))


_DATASET_KEYS = {"cuboid_dims": "cuboid_dims", "cuboid_centers": "cuboid_centers", "cuboid_quats": "cuboid_quaternions",
                 "cylinder_radii": "cylinder_radii", "cylinder_heights": "cylinder_heights",
                 "cylinder_centers": "cylinder_centers", "cylinder_quats": "cylinder_quaternions"}


def problems_to_dataset(prob: Dict[str, torch.Tensor], trajectory_key: str = "global_solutions") -> Dict[str, np.ndarray]:
    """The ``expert_valid`` rows of ``make_problem_batch(collision_free=True, expert=True)`` under the HDF5 key names of
    the reference's dataset (``data.PointCloudTrajectoryDataset(mapping, "global_solutions", ...)`` reads them): float32
    numpy arrays ``cuboid_{dims,centers,quaternions}``, ``cylinder_{radii,heights,centers,quaternions}``,
    ``global_solutions`` [N,50,7].  ``trajectory_key="hybrid_solutions"`` (a batch made with ``hybrid=True``; the key the
    reference's training job reads, jobconfig.yaml:28): the kept rows are ``hybrid_valid`` and both ``global_solutions``
    and ``hybrid_solutions`` are written, as the reference's files hold both."""
    if trajectory_key not in ("global_solutions", "hybrid_solutions"):
        raise ValueError(f"trajectory_key must be 'global_solutions' or 'hybrid_solutions', got {trajectory_key!r}")
    assert "expert_valid" in prob, "problems_to_dataset needs make_problem_batch(collision_free=True, expert=True)"
    hybrid = trajectory_key == "hybrid_solutions"
    assert not hybrid or "hybrid_valid" in prob, "trajectory_key='hybrid_solutions' needs make_problem_batch(..., hybrid=True)"
    keep = prob["hybrid_valid" if hybrid else "expert_valid"]
    out = {dst: prob[src][keep].detach().cpu().numpy().astype(np.float32) for src, dst in _DATASET_KEYS.items()}
    out["global_solutions"] = prob["global_solutions"][keep].detach().cpu().numpy().astype(np.float32)
    if hybrid:
        out["hybrid_solutions"] = prob["hybrid_solutions"][keep].detach().cpu().numpy().astype(np.float32)
    return out


def make_problem_batch(B: int, seed: int = 0, device="cuda:0", kinds=("tabletop",), M1: int = 16, M2: int = 16,
                       scene_pool: Optional[int] = None, device_clouds: bool = False, env_offset: int = 0,
                       total_envs: Optional[int] = None, collision_free: bool = False,
                       max_redraws: int = 4, expert: bool = False, expert_from: str = "primitives",
                       expert_point_radius: float = EXPERT_CLOUD_POINT_RADIUS, hybrid: bool = False,
                       hybrid_guide: str = "global", hybrid_against: str = "primitives",
                       problems: str = "uniform", expert_shortcut: bool = False,
                       hybrid_shortcut=False, scene_source: str = "host") -> Dict[str, torch.Tensor]:
    """A batch of planning problems on ``device``: primitives, start configuration, target pose and
    the ``[B, 2048+4096+128, 4]`` slab (robot | scene | target rows, label column 0/1/2 --
    ``mpinets/data_loader.py:261-278``).  ``scene_pool`` bounds the number of distinct scenes
    generated on the host (they are tiled over the batch) to keep set-up time short.

    Sharding: the batch is rows ``[env_offset, env_offset + B)`` of a GLOBAL batch of ``total_envs`` problems
    (default ``env_offset + B``) that depends on ``seed`` only -- every rank passes the same seed and its own offset
    and gets exactly the rows one process would generate (scenes, configurations, targets and, with
    ``device_clouds``, the scene clouds, whose draws are keyed by the global environment id).

    ``collision_free`` (default off: start and goal are plain uniform draws, tested against nothing): the problem the
    reference's generators pose.  The goal is the drawn pose SOLVED against the scene by ``robot.franka_ik`` (``q_goal``),
    the start is ``franka_ik`` of a second drawn pose; a problem whose start or goal has no collision-free solution is
    redrawn, up to ``max_redraws`` times, each time from fresh draws and the next Philox stream.  ``valid`` (bool [B])
    marks the problems that ended with both; the others keep their unchecked first draws as start and target pose, and
    their ``q_goal`` row is NaN.

    ``expert`` (with ``collision_free``): also plans a demonstration from ``q`` to ``q_goal`` with ``robot.franka_plan``
    (a local optimiser standing in for the reference's AIT* + Geometric Fabrics; valid by this engine's sphere model):
    ``global_solutions`` [B,50,7] and ``expert_valid`` = ``valid`` & planned (bool [B]); the other rows are NaN.  The
    candidate draws are keyed by the global row, so shards agree.  ``expert_from="cloud"`` plans against the batch's own
    scene cloud (the scene rows of ``xyz``) with ``solvers.franka_plan_cloud`` at ``expert_point_radius`` instead of against
    the primitives: what a depth or captured cloud, which has no primitives, allows.  Valid then means free by
    ``FrankaCollisionSampler.check_cloud`` at that radius, which is not the primitive test.
    ``expert_from="roadmap"`` plans against the primitives with ``robot.franka_plan_global``: a lazy roadmap's path seeds one
    more candidate, so a problem whose straight line is blocked is not silently dropped; every row ``franka_plan`` solves
    is returned as ``expert_from="primitives"`` returns it.  ``expert_from="cloud_roadmap"`` is the ``"cloud"`` branch with
    ``robot.franka_plan_global_cloud``: the roadmap reads the cloud's distance field, the exact cloud test still judges, and
    every row ``"cloud"`` solves is returned as ``"cloud"`` returns it.  ``expert_shortcut`` (default off; only with the two
    roadmap forms) passes ``shortcut=True`` to those planners: the roadmap's path, shortcut by ``robot.franka_shortcut`` /
    ``franka_shortcut_cloud``, seeds one candidate more, in front of the roadmap's own.

    ``hybrid`` (with ``expert``; default off, which leaves every key as it was): also ``hybrid_solutions`` [B,50,7], the
    demonstration of ``solvers.franka_follow`` along eight right_gripper poses of ``global_solutions`` (a reactive follower
    standing in for the reference's Geometric Fabrics expert, NOT Lula), retimed to constant speed and judged against the
    primitives; ``hybrid_valid`` = ``expert_valid`` & followed and valid (bool [B]; the other rows are NaN); and
    ``hybrid_target_pose`` [B,4,4], the pose the hybrid trajectory ends at (the reference's hindsight goal revision).
    Refused with ``expert_from="cloud"`` and ``"cloud_roadmap"`` unless ``hybrid_against="cloud"``: ``hybrid_valid`` would mix the
    cloud test of the plan with the primitive test of the follower.

    ``hybrid_against`` (with ``hybrid``; default "primitives", which leaves every key and every bit as it was): "cloud" needs
    ``expert_from`` "cloud" or "cloud_roadmap" and ``hybrid_guide`` "global" or "gripper_cloud" ("gripper" plans through the
    primitives).  The follower is then ``solvers.franka_follow_cloud`` (the same stand-in controller) along the same eight poses of the cloud
    plan, against the same scene cloud at ``expert_point_radius`` through one shared distance field; ``hybrid_valid`` =
    ``expert_valid`` & followed and free by ``check_cloud``'s test, the test the plan was judged by.  The keys are the same
    three, and ``problems_to_dataset(prob, "hybrid_solutions")`` reads them unchanged.

    ``hybrid_guide`` (with ``hybrid``; default "global", which leaves every key and every bit as it was): "gripper" takes the
    follower's guide not from ``global_solutions`` but from ``solvers.gripper_roadmap``, a roadmap planner for the
    free-flying gripper in SE(3) from the right_gripper pose of ``q`` to that of ``q_goal`` through the same primitives, at
    eight poses, keyed by ``seed`` / ``env_offset`` so that shards agree -- the stage the reference runs before its fabric
    (gen_data.py:156-189); a stand-in for that OMPL planner, not a port, valid by this engine's sphere model.  No fall-back
    between the guides: a row without a gripper path is not ``hybrid_valid``, which still requires ``expert_valid`` as the
    reference requires the global plan.  Also ``hybrid_guide_poses`` [B,8,4,4] (NaN rows without a path) and
    ``hybrid_guide_status`` int32 [B] (``gripper_roadmap``'s).  "gripper_cloud" (only with ``hybrid_against="cloud"``) is the
    same stage against the scene cloud: ``solvers.gripper_roadmap_cloud`` at ``expert_point_radius``, through the one field
    the cloud follower reads, with the same two extra keys; its verdicts come from the field, which approximates, so the
    exact judge stays ``check_cloud``'s test on the follower's trajectory.  "gripper" with ``hybrid_against="cloud"`` is
    refused.  ``hybrid_shortcut`` (default off, which leaves every key and every bit as it was; True or a dict of
    ``solvers.gripper_shortcut``'s options; only with ``hybrid_guide`` "gripper" or "gripper_cloud"): the gripper roadmap's
    path is shortcut on the device (``solvers.gripper_plan`` / ``gripper_plan_cloud``, the cloud form through the same one
    field) before it is resampled, and ``hybrid_guide_poses`` are the shortcut's; ``hybrid_guide_status`` stays the
    roadmap's.  A shorter guide hugs the obstacle: whether the follower does better with it is measured in
    profiles/gripper_shortcut_timing.md, not promised.

    ``problems`` (default "uniform", which leaves every key and every bit as it was: start and goal are the forward
    kinematics of uniform draws over the joint limits, poses anywhere in the air).  "task" (needs ``collision_free``): the
    problems the reference's generators pose.  Start and goal are TASK-ORIENTED candidates drawn on the scene's supports
    (``make_task_scenes``) by ``solvers.task_candidates`` -- above a table top or an object on it with the gripper pointing
    down, inside a cubby pocket with the gripper reaching in, start and goal in different pockets -- and per role the first
    free candidate, of up to 100 draws, that ``franka_ik`` solves against the scene.  Free means free by this engine's
    sphere model, not by PyBullet's meshes, and the dresser's supports are a stand-in with no reference counterpart.
    ``valid`` = both were found (no redraws: ``max_redraws`` is not used); ``q``, ``q_goal``, ``target_pose`` and the 128
    target rows of the slab come from the chosen candidates, and ``expert``, ``hybrid`` and every ``expert_from`` /
    ``hybrid_guide`` / ``hybrid_against`` run unchanged on them.  New keys: ``support_boxes`` / ``support_kind`` (the scene's),
    ``start_pose`` [B,4,4], ``target_support`` int32 [B] (the goal's support row, -1 where invalid), ``target_volume`` [B,10]
    (centre, dims, quaternion of the goal's support; NaN for a surface) and ``target_negative_volumes`` [B,S,10] (the other
    live volume supports; NaN rows elsewhere): what the reference's inference problems carry for ``check_final_region``
    (``metrics.BatchedEvaluator``).  Invalid rows keep their uniform draws as start and target pose, a NaN ``q_goal`` and NaN /
    -1 in the new keys.  The reference's neutral starts (``random_neutral``) need robofin's constants, which are not in the
    tree: out of scope.

    ``scene_source`` (default "host", which leaves every key and every bit as it was: ``make_scenes`` / ``make_task_scenes``,
    one sequential numpy rng, which has to generate every scene up to the batch's last one).  "device": the scenes come from
    ``make_scenes_device`` (csrc/scene_gen.hip) -- the same distributions, supports included, but OTHER scenes than the host
    draws from the same seed: numpy's stream cannot be reproduced by a counter rng.  The scene of global row ``gid`` has id
    ``gid % nscene`` (``scene_pool`` keeps its meaning; without it every row has its own scene) and depends on
    ``(seed, id, kind, M1, M2, S)`` alone, so ONLY this batch's rows are generated: the last shard of a 65536-row batch draws
    its 8192 scenes, not 65536.  ``S`` follows ``problems`` as on the host.  Needs ``device_clouds=True``: the host cloud
    sampler reads host arrays, which this source never makes.  Everything behind the scenes runs unchanged.

    ``kinds`` may name the reference's own scenes, "tabletop_reference", "cubby_reference" and "merged_cubby" (M1 >= 7), under
    both sources.  With ``problems="uniform"`` a merged cubby is the one with its drawn pocket pair.  With ``problems="task"``
    a merged-cubby row follows ``MergedCubbyEnvironment``: the scene is generated unmerged, start and goal are picked in
    different pockets as for any cubby, then every VALID such row is generated again with those two pockets as its pair and
    ``target_support`` is mapped to the merged support; ``target_volume``, the experts, the followers and the scene cloud all
    see the merged primitives (``target_negative_volumes`` are recomputed from the merged supports, where the reference leaves
    its own stale); invalid rows stay unmerged.  The merge is per ROW, not per scene, so this needs
    ``scene_source="device"`` and ``device_clouds=True`` and anything else raises a ``ValueError``."""
    from .robot import FrankaSampler, franka_fk, frames_to_matrix

    assert collision_free or not expert, "expert trajectories need collision_free=True (checked start and goal)"
    assert expert or not hybrid, "hybrid trajectories follow the expert's: they need expert=True"
    if hybrid_against not in ("primitives", "cloud"):
        raise ValueError(f"hybrid_against must be 'primitives' or 'cloud', got {hybrid_against!r}")
    if hybrid_against == "cloud":
        assert hybrid, "hybrid_against='cloud' chooses the follower's environment: it needs hybrid=True"
        if expert_from not in ("cloud", "cloud_roadmap"):
            raise ValueError("hybrid_against='cloud' needs expert_from='cloud' or 'cloud_roadmap': a plan judged against the "
                             f"primitives is not what the cloud follower would be judged by, got {expert_from!r}")
        if hybrid_guide == "gripper":
            raise ValueError("hybrid_against='cloud' needs hybrid_guide='global' or 'gripper_cloud': 'gripper' plans through "
                             "the primitives, and that gripper roadmap has no cloud form: use 'gripper_cloud'")
    elif hybrid and expert_from in ("cloud", "cloud_roadmap"):  # (``hybrid_valid`` would mix two tests)
        raise ValueError("hybrid=True needs expert_from='primitives' or 'roadmap': the follower runs against the primitives, "
                         "a plan judged against the point cloud is not what it would be judged by "
                         "(hybrid_against='cloud' follows against the cloud instead)")
    if hybrid_guide not in ("global", "gripper", "gripper_cloud"):
        raise ValueError(f"hybrid_guide must be 'global', 'gripper' or 'gripper_cloud', got {hybrid_guide!r}")
    if hybrid_guide == "gripper_cloud" and hybrid_against != "cloud":
        raise ValueError("hybrid_guide='gripper_cloud' plans the gripper against the scene cloud: it needs "
                         "hybrid_against='cloud' ('gripper' plans it through the primitives)")
    if expert_from not in ("primitives", "cloud", "roadmap", "cloud_roadmap"):
        raise ValueError(f"expert_from must be 'primitives', 'cloud', 'roadmap' or 'cloud_roadmap', got {expert_from!r}")
    if expert_shortcut and expert_from not in ("roadmap", "cloud_roadmap"):
        raise ValueError("expert_shortcut=True needs expert_from='roadmap' or 'cloud_roadmap': there is no roadmap path to shortcut")
    if hybrid_shortcut and not (hybrid and hybrid_guide in ("gripper", "gripper_cloud")):
        raise ValueError("hybrid_shortcut needs hybrid=True and hybrid_guide='gripper' or 'gripper_cloud': there is no gripper "
                         "roadmap path to shortcut")
    if problems not in ("uniform", "task"):
        raise ValueError(f"problems must be 'uniform' or 'task', got {problems!r}")
    if scene_source not in ("host", "device"):
        raise ValueError(f"scene_source must be 'host' or 'device', got {scene_source!r}")
    if scene_source == "device" and not device_clouds:
        raise ValueError("scene_source='device' needs device_clouds=True: the host cloud sampler reads the host generator's "
                         "arrays, and the device source makes none")
    task = problems == "task"
    if task and not collision_free:
        raise ValueError("problems='task' poses checked starts and goals: it needs collision_free=True")
    unknown = [k for k in kinds if k not in SCENE_KIND_CODES]
    if unknown:
        raise ValueError(f"kinds must be among {tuple(SCENE_KIND_CODES)}, got {unknown}")
    if any(k in REFERENCE_KINDS for k in kinds) and M1 < 7:
        raise ValueError(f"the kinds {REFERENCE_KINDS} need M1 >= 7 (a cubby has seven plates), got M1 = {M1}")
    merge_rows = task and "merged_cubby" in kinds
    if merge_rows and not (scene_source == "device" and device_clouds):
        raise ValueError("kinds with 'merged_cubby' under problems='task' need scene_source='device' and device_clouds=True: "
                         "the plates between the start's and the goal's pocket are removed PER ROW, after the problem is "
                         "drawn, and the host source makes one scene (and one host cloud) for all the rows that share it")

    dev = torch.device(device)
    total = env_offset + B if total_envs is None else int(total_envs)
    assert 0 <= env_offset and env_offset + B <= total
    nscene = total if scene_pool is None else min(total, scene_pool)
    gid = env_offset + np.arange(B)  # global environment ids of this batch's rows
    sid = gid % nscene  # environment g sits in scene g mod nscene
    if scene_source == "device":  # (this batch's rows and nothing else; S is ``make_task_scenes``' default)
        cloud = None
        unmerged = torch.full((B, 2), -1, dtype=torch.int32, device=dev) if merge_rows else None
        out = make_scenes_device(B, seed, kinds, M1, M2, S=8 if task else None, device=dev, scene_ids=torch.from_numpy(sid),
                                 merge_pockets=unmerged)
    else:
        scn = (make_task_scenes if task else make_scenes)(nscene if scene_pool is not None else int(sid.max()) + 1 if B else 0,
                                                          seed, kinds, M1, M2)
        cloud = None if device_clouds else sample_scene_clouds_host(scn, NUM_OBSTACLE_POINTS, seed)
        out = {k: torch.from_numpy(np.ascontiguousarray(v[sid])).to(dev) for k, v in scn.items()}
    q = torch.from_numpy(random_configurations(env_offset + B, seed)[env_offset:]).to(dev)
    q_target = torch.from_numpy(random_configurations(env_offset + B, seed + 7)[env_offset:]).to(dev)
    lim = torch.as_tensor(ft.JOINT_LIMITS_REAL, dtype=torch.float32, device=dev)
    task_pose = None
    if task:
        q, q_goal, valid, start_pose, task_pose, target_support = _task_problems(out, out["support_boxes"], out["support_kind"],
                                                                                 q, q_target, seed, env_offset)
        if merge_rows:
            target_support = _merge_task_rows(out, kinds, sid, valid, start_pose, task_pose, target_support, seed, M1, M2, dev)
        out.update(q_goal=q_goal, valid=valid, start_pose=start_pose, target_support=target_support,
                   **_task_region_keys(out["support_boxes"], out["support_kind"], target_support))
    elif collision_free:
        q, q_target, q_goal, valid = _collision_free_problems(out, q, q_target, seed, env_offset, max_redraws)
        out.update(q_goal=q_goal, valid=valid)
    if collision_free:
        if expert and expert_from in ("primitives", "roadmap"):
            out.update(_expert_trajectories(out, q, q_goal, valid, seed, env_offset, roadmap=expert_from == "roadmap",
                                            shortcut=expert_shortcut))
    state = np.random.get_state()
    np.random.seed(seed)
    sampler = FrankaSampler(dev)
    xyz = torch.zeros((B, NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS + NUM_TARGET_POINTS, 4), dtype=torch.float32,
                      device=dev)
    xyz[:, NUM_ROBOT_POINTS:NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS, 3] = 1
    xyz[:, NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS:, 3] = 2
    subset = sampler.draw_subset(NUM_ROBOT_POINTS)  # (one column subset for the whole global batch: same seed, same draw)
    sampler.sample_into(q, xyz, subset)
    if device_clouds:  # every environment gets its own draw, even when the primitives are tiled
        sample_scene_clouds(out, NUM_OBSTACLE_POINTS, seed, out=xyz[:, NUM_ROBOT_POINTS:NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS],
                            env_offset=env_offset)
    else:
        xyz[:, NUM_ROBOT_POINTS:NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS, :3] = torch.from_numpy(cloud[sid]).to(dev)
    if expert and expert_from in ("cloud", "cloud_roadmap"):
        scene_cloud = xyz[:, NUM_ROBOT_POINTS:NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS, :3]
        out.update(_expert_trajectories_cloud(scene_cloud, q, q_goal, valid, seed, env_offset, expert_point_radius,
                                              roadmap=expert_from == "cloud_roadmap", shortcut=expert_shortcut))
    target_pose = frames_to_matrix(franka_fk(q_target)[:, ft.LINK_ID["right_gripper"]])
    if task:  # (valid rows: the chosen goal candidate; the others keep the pose of their uniform draw)
        target_pose = torch.where(out["valid"][:, None, None], task_pose, target_pose)
    xyz[:, NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS:, :3] = sampler.sample_end_effector(target_pose, NUM_TARGET_POINTS)
    np.random.set_state(state)
    if hybrid and hybrid_against == "cloud":
        out.update(_hybrid_trajectories_cloud(xyz[:, NUM_ROBOT_POINTS:NUM_ROBOT_POINTS + NUM_OBSTACLE_POINTS, :3], q,
                                              out["global_solutions"], out["expert_valid"], expert_point_radius, q_goal, seed,
                                              env_offset, gripper_guide=hybrid_guide == "gripper_cloud",
                                              shortcut=hybrid_shortcut))
    elif hybrid:
        out.update(_hybrid_trajectories(out, q, out["global_solutions"], out["expert_valid"], q_goal, seed, env_offset,
                                        gripper_guide=hybrid_guide == "gripper", shortcut=hybrid_shortcut))
    out.update(q=q, q_norm=(q - lim[:, 0]) / (lim[:, 1] - lim[:, 0]) * 2 - 1, xyz=xyz, target_pose=target_pose,
               target_position=target_pose[:, :3, 3].contiguous(), robot_subset=subset, env_offset=int(env_offset))
    return out
