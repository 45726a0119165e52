"""The plan check's contract (include/neo_mpc.h, neo_mpc_plan_check_batch) transcribed line by line in plain Python -- nav2
is not a dependency of this repository, so this transcription IS the reference of K15 (k_plan_check).  The closest pose is
tests/carrot_reference.py's min_by over the float64 hypot, the outline cost tests/footprint_gate_reference.py's
footprint_cost; the decisions below are `if`s on Python ints, one pose after the other.  Helper module: no tests in here."""
import math

import numpy as np

from neo_mpc_planner2_amd import abi
from tests import carrot_reference as cref
from tests import footprint_gate_reference as fref


def closest(poses, robot):
    """K4's rule to the letter (cpp:83-88): min_by over euclidean_distance, libm's hypot with its NaN / infinity behaviour."""
    return cref.min_by([math.hypot(float(p[0]) - float(robot[0]), float(p[1]) - float(robot[1])) for p in poses])


def point_value(cells, res, ox, oy, x, y, outside_value):
    """Point mode: the vertex rule against the map's true size; off the map the value is `outside_value`."""
    size_y, size_x = cells.shape
    cell = fref.world_to_map(float(x), float(y), size_x, size_y, res, ox, oy)
    if cell is None:
        return int(outside_value)
    return int(cells[cell[1], cell[0]])


def outline_value(cells, res, ox, oy, pose, footprint):
    """Footprint mode: neo_mpc_footprint_batch's outline cost at the pose."""
    return int(fref.footprint_cost(cells, res, ox, oy, fref.oriented(pose, footprint)))


def blocks(v, max_cost, unknown_blocks):
    if v == 255:
        return bool(unknown_blocks)
    return v >= max_cost


def check_one(cells, res, ox, oy, poses, robot, footprint, max_cost, unknown_blocks, outside_value, max_poses):
    """One robot -> (begin, end, first_blocked, status, value)."""
    n = len(poses)
    if n == 0:
        return 0, 0, 0, 2, 0
    begin = 0 if robot is None else closest(poses, robot)
    end = n
    if max_poses != 0:
        end = min(n, begin + max_poses)
    widest = 0
    for k in range(begin, end):
        if footprint is None:
            v = point_value(cells, res, ox, oy, poses[k][0], poses[k][1], outside_value)
        else:
            v = outline_value(cells, res, ox, oy, poses[k], footprint)
        if blocks(v, max_cost, unknown_blocks):
            return begin, end, k, 1, v
        if v < 255 and v > widest:
            widest = v
    return begin, end, end, 0, widest


def check_plans(cells, res, ox, oy, plan_poses, plan_offsets, robot_poses=None, footprint=None, max_cost=253,
                unknown_blocks=False, outside_value=255, max_poses=0):
    """The batch -> records (abi.PLAN_CHECK_DTYPE [count]), `reserved` 0."""
    cells = np.asarray(cells)
    plan_poses = np.asarray(plan_poses, dtype=np.float64).reshape(-1, 3)
    count = len(plan_offsets) - 1
    out = np.zeros(count, dtype=abi.PLAN_CHECK_DTYPE)
    for i in range(count):
        poses = plan_poses[int(plan_offsets[i]):int(plan_offsets[i + 1])]
        robot = None if robot_poses is None else robot_poses[i]
        r = check_one(cells, float(res), float(ox), float(oy), poses, robot, footprint, int(max_cost), bool(unknown_blocks),
                      int(outside_value), int(max_poses))
        out[i] = r + (0,)
    return out


def assemble(plans):
    """A list of plans ([n, 3] arrays, n may be 0) -> (poses [total, 3], offsets [count + 1] uint32)."""
    offsets = np.zeros(len(plans) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(p) for p in plans])
    poses = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in plans] + [np.zeros((0, 3))])
    return poses, offsets


def record(begin, end, first_blocked, status, value):
    """One expected record, written out by hand in a test."""
    return (begin, end, first_blocked, status, value, 0)
