"""Closed control loop of a fleet on one GPU -- the deployed mode of the hot path.

The reference runs one robot: `computeVelocityCommands` (src/NeoMpcPlanner.cpp:202-254) at `controller_frequency`,
each call warm-started from the previous solution shifted by one control step (py:397-400, 198-202).  Here a whole
fleet does that on the device: one K1 launch per tick over HBM-resident requests / state / warm starts; between ticks
the robots are moved by their own commands and the look-ahead point -- kept 0.4 m ahead of the robot along its initial
world bearing, as a carrot sliding along a straight plan would be -- is re-expressed in the base frame with torch ops
on the request records (plumbing: the tick itself goes through the C-ABI).  Used by bench.py (`warm_tick`) and
tools/bench_fleet_loop.py.
"""
import numpy as np

from . import abi


def closed_loop(solver, batch, ticks, hz=30.0, before_tick=None, after_tick=None, balance_every=0, footprint=None,
                rolling=None, stamp=None, scan=None, laser=None, world_scan=None):
    """Run `ticks` control ticks of `batch` (a solver.DeviceBatch) through `solver` (a BatchSolver with its costmap
    set).  Returns per-tick lists: kernel_ms (HIP events around the K1 launch), mean_iterations, max_iterations,
    stopped_fraction.  `before_tick(t, pos)` runs before tick t's launch (e.g. re-centre a costmap pool),
    `after_tick(t, commands)` after its commands are on the host.  `balance_every` = R > 0: every R-th tick the
    dispatch order of the following ticks is rebuilt from that tick's iteration counts (neo_mpc_balance_dispatch_device:
    one small kernel behind K1 on the same stream; `balance_ms` in the result is its own duration) -- results do not
    depend on it, only which robots share a SIMD.  `footprint` = a base-frame polygon ((x, y), ...), e.g.
    synthetic.RECT_FOOTPRINT: every tick runs the footprint gate (K6, neo_mpc_footprint_gate_device) at the loop's own
    poses in front of K1 and hands K1 the oriented polygons (`footprints`), so the collision latch of py:343-347 acts on
    the robots' real outlines; the result gains `footprint_lethal_fraction`, the share of robots whose gate cost is >= 254.
    None: no gate, no polygons -- the loop every caller had before.  `rolling` = (size_x, size_y, resolution, origins), `origins`
    a CUDA float64 [count, 2] tensor: every tick rolls the fleet's costmap windows over the solver's world map
    (BatchSolver.set_world_map) at the loop's own poses (K7, neo_mpc_roll_costmap_pool_device) in front of the gate and K1
    -- robot i reads window `map_index` = i of its request.  None: no roll, the loop is unchanged.  `stamp` =
    (inscribed_radius, inflation_radius, cost_scaling_factor), with `rolling` and `footprint`: between the roll and the gate
    every tick stamps the other robots' outlines, inflation ring included, into each window at the loop's own poses (K8,
    neo_mpc_stamp_fleet_device), so the gate and K1's collision latch see the fleet.  None: no stamp, the loop is unchanged.
    `scan` = a callable, with `rolling`: `scan(t, poses)` returns the keyword arguments of BatchSolver.update_scan_layer for
    tick t -- the inflation parameters, and on a tick with a new observation `points` and `sensor_origins` as CUDA tensors
    (without them: flags 0, the layer is rolled and applied again; pass on_device=True then) -- and the update (K10,
    neo_mpc_update_scan_layer_device) runs between the roll and the stamp, so the gate and K1 see what the sensors saw.
    None: no scan layer, the loop is unchanged.  `laser` = a callable, with `rolling` and instead of `scan`: `laser(t, poses)`
    returns the keyword arguments of BatchSolver.update_scan_layer_from_ranges for tick t -- the inflation parameters, `ranges`
    as a CUDA float32 tensor, `poses` (the loop's own, handed through, or the caller's) and `scanners` -- and the projection
    and the update over all scanners (K11, neo_mpc_update_scan_layer_from_ranges_device) run where `scan` runs.  None: the
    loop is unchanged.  `world_scan` = a callable, with `rolling`; it excludes nothing: `world_scan(t, poses)` returns the
    keyword arguments of BatchSolver.update_world_scan_layer -- or, when `ranges` is among them, of
    update_world_scan_layer_from_ranges -- and the update of the fleet's shared layer on the world map (K12) runs BEFORE the
    roll, so every window is cut from what the whole fleet saw.  None: the loop is unchanged."""
    assert stamp is None or (rolling is not None and footprint is not None), "stamp needs rolling and footprint"
    assert scan is None or rolling is not None, "scan needs rolling"
    assert laser is None or (rolling is not None and scan is None), "laser needs rolling and excludes scan"
    assert world_scan is None or rolling is not None, "world_scan needs rolling"
    import torch
    b = batch
    P = b.problems.view(torch.float64).reshape(b.count, -1)          # the 32 doubles of each request
    q = P[:, 2:6]
    yaw = torch.atan2(2 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]), 1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2)).clone()
    pos = P[:, 0:2].clone()
    c, sn = torch.cos(yaw), torch.sin(yaw)
    carrot_off = torch.stack([c * P[:, 6] - sn * P[:, 7], sn * P[:, 6] + c * P[:, 7]], 1)   # world frame
    cq = P[:, 8:12]
    carrot_yaw_w = yaw + torch.atan2(2 * (cq[:, 3] * cq[:, 2] + cq[:, 0] * cq[:, 1]),
                                     1 - 2 * (cq[:, 1] ** 2 + cq[:, 2] ** 2))
    P[:, 22] = 1.0 / hz
    P[:, 23] = 1.0 / hz
    # one event pair per tick, stamped by the dispatch of K1 itself (neo_mpc_solve_batch_device_timed): separate
    # event records around the launch would add their own barrier packets (~20 us) to what is read as kernel time
    stream = torch.cuda.current_stream()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ticks)]
    for e0, e1 in evs:
        e0.record(stream)
        e1.record(stream)
    torch.cuda.synchronize()
    out = {"kernel_ms": [], "mean_iterations": [], "max_iterations": [], "stopped_fraction": []}
    bal_evs = []
    polygons = None
    if footprint is not None:
        base = torch.tensor(np.asarray(footprint, dtype=np.float64).reshape(-1, 2), device=pos.device)
        gate_costs = torch.zeros(b.count, dtype=torch.float64, device=pos.device)
        polygons = torch.zeros((b.count, base.shape[0], 2), dtype=torch.float64, device=pos.device)
        out["footprint_lethal_fraction"] = []
    for t in range(ticks):
        if before_tick is not None:
            before_tick(t, pos)
        if rolling is not None or footprint is not None:
            poses = torch.cat([pos, yaw[:, None]], 1).contiguous()   # one array serves the roll and the gate
        if world_scan is not None:
            kw = world_scan(t, poses)
            (solver.update_world_scan_layer_from_ranges if "ranges" in kw else solver.update_world_scan_layer)(**kw)
        if rolling is not None:
            solver.roll_costmap_pool(rolling[0], rolling[1], rolling[2], rolling[3], poses=poses)
        if scan is not None:
            solver.update_scan_layer(**scan(t, poses))
        if laser is not None:
            solver.update_scan_layer_from_ranges(**laser(t, poses))
        if stamp is not None:
            solver.stamp_fleet(stamp[0], stamp[1], stamp[2], footprint=base, poses=poses)
        if footprint is not None:
            # (the requests ride along for their map_index -- a pool -- and get the normalised cost written)
            solver.footprint_gate_device(base, gate_costs, poses=poses, problems=b.problems, footprints_out=polygons)
        solver.solve_device(b.problems, b.states, b.warm, b.commands, velocities=b.vel, events=evs[t],
                            footprints=polygons)
        if balance_every and t % balance_every == 0:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            solver.balance_dispatch(b.commands)
            e1.record(stream)
            bal_evs.append((e0, e1))
        cmd = b.vel
        yaw = yaw + cmd[:, 2] / hz
        c, sn = torch.cos(yaw), torch.sin(yaw)
        pos = pos + torch.stack([c * cmd[:, 0] - sn * cmd[:, 1], sn * cmd[:, 0] + c * cmd[:, 1]], 1) / hz
        P[:, 0:2] = pos
        P[:, 2] = 0.0
        P[:, 3] = 0.0
        P[:, 4] = torch.sin(0.5 * yaw)
        P[:, 5] = torch.cos(0.5 * yaw)
        d = carrot_off
        P[:, 6] = c * d[:, 0] + sn * d[:, 1]
        P[:, 7] = -sn * d[:, 0] + c * d[:, 1]
        rel = carrot_yaw_w - yaw
        P[:, 8] = 0.0
        P[:, 9] = 0.0
        P[:, 10] = torch.sin(0.5 * rel)
        P[:, 11] = torch.cos(0.5 * rel)
        P[:, 19:22] = cmd
        torch.cuda.synchronize()
        cm = b.commands.cpu().numpy().view(abi.COMMAND_DTYPE).reshape(-1)
        out["mean_iterations"].append(float(cm["iterations"].mean()))
        out["max_iterations"].append(int(cm["iterations"].max()))
        out["stopped_fraction"].append(float(((cm["flags"] & abi.FLAG_STOPPED) != 0).mean()))
        if footprint is not None:
            out["footprint_lethal_fraction"].append(float((gate_costs >= 254.0).double().mean().item()))
        if after_tick is not None:
            after_tick(t, cm)
    out["kernel_ms"] = [a.elapsed_time(e) for a, e in evs]
    if bal_evs:
        out["balance_ms"] = [a.elapsed_time(e) for a, e in bal_evs]
        out["balance_every"] = balance_every
        solver.balance_dispatch(None)
    return out


def summary(loop, skip=5):
    """The figures bench.py reports for the warm ticks (everything after the first `skip`)."""
    ms, it, mx = loop["kernel_ms"], loop["mean_iterations"], loop["max_iterations"]
    return {"ticks": len(ms) - skip, "ms_per_tick_median": float(np.median(ms[skip:])),
            "ms_per_tick_max": float(np.max(ms[skip:])), "mean_iterations": float(np.mean(it[skip:])),
            "max_iterations_median": float(np.median(mx[skip:])), "max_iterations_max": int(np.max(mx[skip:])),
            "cold_tick_ms": float(ms[0]), "cold_tick_mean_iterations": float(it[0]),
            "stopped_fraction_last_tick": float(loop["stopped_fraction"][-1]),
            # balanced dispatch (closed_loop(balance_every=R)): the order kernel's own duration (events around it, launch
            # gaps included) and its share of a tick when it runs every R-th tick
            **({"balance_every": loop["balance_every"], "order_kernel_ms_median": float(np.median(loop["balance_ms"])),
                "ms_per_tick_median_incl_order": float(np.median(ms[skip:]) + np.median(loop["balance_ms"]) / loop["balance_every"])}
               if "balance_ms" in loop else {})}
