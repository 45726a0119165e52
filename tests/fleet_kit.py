"""The kit of the fleet-layer tests (K7 .. K14): device helpers, the readers of a handle's layer state, the HIP-graph harness
and the fleets that several test files share, one copy of each.  No tests here; generators of whole cases live in
tests/world_scan_cases.py."""
import contextlib
import types

import numpy as np

from neo_mpc_planner2_amd import synthetic

RECT = tuple(synthetic.RECT_FOOTPRINT)
F32 = np.float32
#: ranges that drop nothing
FAR = dict(obstacle_max_range=100.0, obstacle_min_range=0.0, raytrace_max_range=100.0, raytrace_min_range=0.0)


# ------------------------------------------------------------------------------------------ plain helpers
def gpu(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a).astype(dtype)
    return torch.from_numpy(a.copy()).to("cuda:0")


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def inflation_for(reach, res):
    """(inscribed_radius, inflation_radius, cost_scaling_factor) with ceil(inflation_radius / res) == reach."""
    radius = 0.0 if reach == 0 else (reach - 0.5) * res
    return min(radius, 1.5 * res), radius, 3.0 / (res * max(reach, 1))


def scanner(mount, angle_min, angle_increment, range_min, range_max, flags=0):
    return dict(mount_x=mount[0], mount_y=mount[1], mount_yaw=mount[2], angle_min=angle_min, angle_increment=angle_increment,
                range_min=range_min, range_max=range_max, flags=flags)


def rectangle(x0, y0, x1, y1, clockwise=False):
    p = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return np.array(p[::-1] if clockwise else p, dtype=np.float64)


def cell_centre(i, l, res=1.0, ox=0.0, oy=0.0):
    return (ox + (i + 0.5) * res, oy + (l + 0.5) * res)


def rolled_pool(s, sx, sy, res, origins, poses):
    """A roll on the host variant: (pool, origins)."""
    s.roll_costmap_pool(sx, sy, res, origins, poses=poses)
    return s.get_costmap_pool()


# ------------------------------------------------------------------------------------------ what a handle holds
def window_state(s):
    """The per-window layers (K10, K11): (layers, layer origins, pool, origins)."""
    import torch
    torch.cuda.synchronize()
    layers, layer_origins = s.get_scan_layer()
    pool, origins = s.get_costmap_pool()
    return layers, layer_origins, pool, origins


def world_state(s):
    """The fleet's shared layer (K12): (layer, live)."""
    import torch
    torch.cuda.synchronize()
    return s.get_world_scan_layer()


def denoised_of(s):
    import torch
    torch.cuda.synchronize()
    return s.get_world_scan_denoised()


# ------------------------------------------------------------------------------------------ the HIP-graph harness
def eager_on_side_stream(tick):
    """The eager call every capture needs -- it builds tables and allocates -- made on the stream the capture will use."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tick()
    torch.cuda.synchronize()
    return side


def capture(tick, stream):
    import torch
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        tick()
    return g


def capture_fleet(spread):
    """The fleet of the capture tests: 64 robots within `spread` cells of a 300 x 300 world, a 48 x 44 window each that
    starts 1 m below and left of its robot."""
    count = 64
    world, res, wox, woy = synthetic.make_costmap(300, seed=91)
    probs = synthetic.make_problems(count, spread, seed=92)
    probs["map_index"] = np.arange(count, dtype=np.int32)
    st, warm = synthetic.make_states(probs, 3)
    return types.SimpleNamespace(count=count, sx=48, sy=44, world=world, res=res, wox=wox, woy=woy, probs=probs, st=st,
                                 warm=warm, start=probs["cur_xy"] - 1.0)


class Side:
    """One handle of a capture test with its device buffers.  A tick is a tuple whose first member is the poses [count, 3];
    a test subclasses this with its tick(), its further inputs and the further fields of result()."""

    def __init__(self, fleet, tick):
        import torch
        from neo_mpc_planner2_amd.solver import DeviceBatch
        self.s = self.open_solver()
        self.s.set_world_map(gpu(fleet.world), fleet.res, fleet.wox, fleet.woy)
        self.b = DeviceBatch(fleet.probs, fleet.st, fleet.warm, "cuda:0")
        self.origins, self.poses = gpu(fleet.start), gpu(tick[0])
        self.costs = torch.zeros(fleet.count, dtype=torch.float64, device="cuda:0")
        self.xy = self.b.problems.view(torch.float64).reshape(fleet.count, -1)[:, 0:2]

    def open_solver(self):
        from neo_mpc_planner2_amd.solver import BatchSolver
        from oracle import mpc_oracle as orc
        return BatchSolver(orc.make_params())

    def set_inputs(self, tick):
        self.poses.copy_(gpu(tick[0]))
        self.xy.copy_(self.poses[:, :2])

    def result(self):
        """(commands, states, gate costs, window origins)"""
        import torch
        torch.cuda.synchronize()
        return (self.b.commands_host().tobytes(), self.b.states_host().tobytes(), self.costs.cpu().numpy().tolist(),
                self.origins.cpu().numpy().tolist())


@contextlib.contextmanager
def replay_against_direct(make_side, ticks, changed):
    """Two sides.  After one eager tick of `graphed` on the capture stream its tick is captured there, a linear chain, and
    replayed twice with the inputs of ticks[1] and ticks[2]; every result equals the same ticks made directly on `direct`,
    and the fields `changed` of it differ from the first tick's.  -> (direct, the last result, the first result) for the
    caller's own assertions; both handles are closed behind them."""
    import torch
    direct, graphed = make_side(), make_side()
    try:
        side = eager_on_side_stream(graphed.tick)
        direct.tick()
        first = direct.result()
        assert first == graphed.result()
        g = capture(graphed.tick, side)
        for k in (1, 2):
            for x in (direct, graphed):
                x.set_inputs(ticks[k])
            torch.cuda.synchronize()
            g.replay()
            direct.tick()
            a, b = graphed.result(), direct.result()
            assert a == b, k
            for i in changed:
                assert a[i] != first[i], (k, i)
        yield direct, a, first
    finally:
        direct.s.close()
        graphed.s.close()


# ------------------------------------------------------------------------------------------ the closed-loop fleets
def standing_fleet(count, xy, goals, seed=7, yaw=None):
    """Robots that stand still at `xy`, look along +x (or along `yaw`) and are sent straight ahead to `goals`:
    (problems, states, warm starts)."""
    probs = synthetic.make_problems(count, 200, seed=seed)
    probs["cur_xy"] = xy
    probs["cur_q"] = (0.0, 0.0, 0.0, 1.0) if yaw is None else synthetic.yaw_quat(yaw)
    probs["carrot_xy"] = (0.4, 0.0)
    probs["carrot_q"] = (0.0, 0.0, 0.0, 1.0)
    probs["goal_xyz"][:, :2] = goals
    probs["goal_q"] = probs["cur_q"]
    probs["cur_vel"] = 0.0
    probs["map_index"] = np.arange(count, dtype=np.int32)
    st, warm = synthetic.make_states(probs, 3)
    return probs, st, warm


def pairs_fleet(beams=41):
    """64 robots in 32 pairs, a 4 x 8 grid: the even robot of a pair -- the seer -- stands 1.5 m behind the odd one and looks
    at it through a front scanner of `beams` beams, whose angles are `angle`; 60 x 60 windows of 5 cm cells."""
    count, size, res = 64, 60, 0.05
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(8)), -1).reshape(-1, 2)
    seers = np.array([-8.0, -7.0]) + grid * (4.0, 2.0) + 0.011
    xy = np.empty((count, 2))
    xy[0::2], xy[1::2] = seers, seers + (1.5, 0.0)
    probs, st, warm = standing_fleet(count, xy, xy + (5.0, 0.0))
    front = scanner((0.1, 0.0, 0.0), -0.25, 0.5 / (beams - 1), 0.05, 8.0)
    angle = front["angle_min"] + np.arange(beams) * front["angle_increment"]
    return types.SimpleNamespace(count=count, size=size, res=res, beams=beams, probs=probs, st=st, warm=warm, xy=xy,
                                 origins=xy - size * res / 2 + 0.013, front=front, angle=angle)


def world_scan_callback(params, d_ranges, front):
    """closed_loop's `world_scan`: every tick the same ranges [count, 1, beams] on the device, from the scanner `front`."""
    def world_scan(t, poses):
        return dict(zip(("inscribed_radius", "inflation_radius", "cost_scaling_factor"), params), ranges=d_ranges, poses=poses,
                    scanners=[front])
    return world_scan
