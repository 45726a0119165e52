"""Batched MPC solver handle: thin Python host side over the C-ABI (include/neo_mpc.h).

`BatchSolver` is what bench.py, the tests and `MpcOptimizationServer` (the mirror of
the reference's service node) drive.  Host (NumPy) batches go through
`neo_mpc_solve_batch`; device-resident batches (torch CUDA tensors, plumbing only)
through `neo_mpc_solve_batch_device` on torch's current stream.
"""
import ctypes as C

import numpy as np

from . import _lib, abi


def laser_beam_table(scanner, beams):
    """The beam table of one scanner (neo_mpc_laser_beam_table; the contract: neo_mpc_laser_batch in include/neo_mpc.h,
    step 4): float64 [beams, 2], (cos, sin) of every beam's angle in the base frame.  Pure host code.  `scanner`: what
    abi.scanner_array takes."""
    sc = abi.scanner_array(scanner)
    assert sc.shape == (1,), "one scanner"
    table = np.zeros((int(beams), 2), dtype=np.float64)
    _lib.check(_lib.load().neo_mpc_laser_beam_table(C.cast(sc.ctypes.data, C.POINTER(abi.NeoMpcScanner)), int(beams),
                                                    C.c_void_p(table.ctypes.data)))
    return table


class BatchSolver:
    """One solver configuration + one costmap on one GPU (a `neo_mpc_handle`)."""

    def __init__(self, params=None, device=0, **overrides):
        self._lib = _lib.load()
        self._abi = int(self._lib.neo_mpc_abi_version())
        self._handle = None
        self.params = dict(params or {})
        self.params.update(overrides)
        ps = abi.params_struct(self.params)
        self.control_steps = int(ps.control_steps)
        self.device = int(device)
        h = self._lib.neo_mpc_create(C.byref(ps), self.device)
        if not h:
            code = self._lib.neo_mpc_last_error_code() if hasattr(self._lib, "neo_mpc_last_error_code") else -1
            raise _lib.NeoMpcError(code, (self._lib.neo_mpc_last_error() or b"").decode())
        self._handle = C.c_void_p(h)
        self._keep = None
        self._last_call = None
        self._in_flight = {}    # ticket -> (batch struct, arrays): kept alive until solve_wait
        self._map_shape = None  # (maps, size_y, size_x) of the costmap(s) the handle holds (get_costmap_pool)
        self._world_device = None   # the torch device the world map was set from (None: from host cells)

    # -- lifecycle ------------------------------------------------------------------
    def close(self):
        if self._handle is not None:
            self._lib.neo_mpc_destroy(self._handle)
            self._handle = None
        # (the marshalled batches keep the caller's arrays alive: let go of them with the handle)
        self._last_call = None
        self._keep = None
        self._in_flight = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- marshalling: one path for NumPy arrays and CUDA tensors -----------------------
    @staticmethod
    def _array(a, on_host, dtype, shape=None, coerce=True):
        """One argument -> (array, address), by the same rule on both sides.  `on_host`: NumPy data, made contiguous and of
        `dtype` -- or, without `coerce`, asserted to be an array that is so already; else a torch tensor, asserted to be CUDA,
        contiguous and of `dtype` (uint32 as its int32 bits).  `dtype` None or a record dtype: the records as they are -- a
        tensor holds them as bytes, so only its leading dimension is compared.  `shape`: what the array's must be; None in it
        is any length."""
        records = dtype is None or np.dtype(dtype).names is not None
        if on_host:
            if coerce and dtype is not None:
                a = np.ascontiguousarray(a, dtype=dtype)
            assert isinstance(a, np.ndarray) and a.flags.c_contiguous and (dtype is None or a.dtype == dtype)
            address = a.ctypes.data
        else:
            import torch
            assert a.is_cuda and a.is_contiguous()
            assert records or a.dtype == getattr(torch, np.dtype(dtype).name.replace("uint32", "int32"))
            address = a.data_ptr()
        if shape is not None:
            got = tuple(a.shape)
            if records and not on_host:
                got, shape = got[:1], shape[:1]
            assert len(got) == len(shape) and all(w is None or w == g for w, g in zip(shape, got)), (got, shape)
        return a, address

    @staticmethod
    def _addresses(on_host, *arrays):
        """The addresses of NumPy arrays (`on_host`) or of torch tensors, taken as they are; None (a NULL pointer) stays None."""
        return [None if a is None else a.ctypes.data if on_host else a.data_ptr() for a in arrays]

    @staticmethod
    def _stream(on_host, where):
        """torch's current stream on the device of `where` (a tensor or a torch device); None for the host variant."""
        if on_host:
            return None
        import torch
        return torch.cuda.current_stream(getattr(where, "device", where)).cuda_stream

    def _call(self, name, stream, *args):
        """The entry point `name` without a stream, `name`_device on `stream` with one (0 is a stream: torch's default)."""
        if stream is None:
            _lib.check(getattr(self._lib, name)(self._handle, *args))
        else:
            _lib.check(getattr(self._lib, name + "_device")(self._handle, *args, C.c_void_p(stream)))

    # -- configuration --------------------------------------------------------------
    def set_params(self, **changes):
        """Dynamic reconfigure (reference: cb_params, mpc_optimization_server.py:405-439)."""
        new = dict(self.params)
        new.update(changes)
        ps = abi.params_struct(new)
        if int(ps.control_steps) != self.control_steps:
            raise ValueError("control_steps cannot change on a live handle (the reference bakes it at init, py:125-137)")
        _lib.check(self._lib.neo_mpc_set_params(self._handle, C.byref(ps)))
        self.params = new    # (a refused set keeps the old parameters, like the library does)

    def set_costmap(self, cells, resolution, origin_x, origin_y):
        """cells: uint8 [size_y, size_x] raw nav2 costs (NumPy) or a CUDA uint8 torch tensor."""
        on_host = isinstance(cells, np.ndarray)
        cells, address = self._array(cells, on_host, np.uint8)
        sy, sx = cells.shape
        self._call("neo_mpc_set_costmap", self._stream(on_host, cells), C.c_void_p(address), sx, sy, float(resolution),
                   float(origin_x), float(origin_y))
        self._map_shape = (1, int(sy), int(sx))

    def set_costmap_pool(self, cells, resolution, origins):
        """Fleet variant: cells uint8 [count, size_y, size_x] (NumPy or CUDA torch tensor), origins
        float64 [count, 2]; instances pick their map with `problems["map_index"]`.  With device
        tensors `origins` is read by every later solve and must stay alive (it may be updated in
        place between ticks, as rolling windows move)."""
        on_host = isinstance(cells, np.ndarray)
        cells, cells_at = self._array(cells, on_host, np.uint8)
        origins, origins_at = self._array(origins, on_host, np.float64)
        m, sy, sx = cells.shape
        assert tuple(origins.shape) == (m, 2)
        if not on_host:
            self._pool_origins = origins   # keep it alive
        self._call("neo_mpc_set_costmap_pool", self._stream(on_host, cells), C.c_void_p(cells_at), m, sx, sy, float(resolution),
                   C.c_void_p(origins_at))
        self._map_shape = (int(m), int(sy), int(sx))

    # -- rolling windows (the step before the gate) ----------------------------------------
    def set_world_map(self, cells, resolution, origin_x, origin_y):
        """The one world map a fleet's rolling windows are cut from (`roll_costmap_pool`): uint8 [size_y, size_x] raw
        nav2 costs, NumPy or a CUDA torch tensor.  The handle keeps its own device copy; the costmap(s) it holds are
        not touched."""
        on_host = isinstance(cells, np.ndarray)
        cells, address = self._array(cells, on_host, np.uint8)
        sy, sx = cells.shape
        self._call("neo_mpc_set_world_map", self._stream(on_host, cells), C.c_void_p(address), sx, sy, float(resolution),
                   float(origin_x), float(origin_y))
        self._world_device = None if on_host else cells.device

    def inflate_world_map(self, inscribed_radius, inflation_radius, cost_scaling_factor):
        """nav2's inflation layer on the handle's copy of the world map, in place (K9; the contract:
        neo_mpc_inflate_world_map in include/neo_mpc.h): set_world_map(raw) -> inflate_world_map -> rolls.  Like
        `set_world_map`: when the world map was set from a CUDA tensor the device call on torch's current stream,
        otherwise the synchronous host call."""
        self._call("neo_mpc_inflate_world_map", self._stream(self._world_device is None, self._world_device),
                   float(inscribed_radius), float(inflation_radius), float(cost_scaling_factor))

    def get_world_map(self):
        """The handle's copy of the world map as the last `set_world_map` or `inflate_world_map` left it: (cells uint8
        [size_y, size_x], resolution, origin_x, origin_y).  Synchronous; waits for the copy or inflation in flight."""
        sx, sy = C.c_uint32(), C.c_uint32()
        res, ox, oy = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self._lib.neo_mpc_get_world_map(self._handle, None, C.byref(sx), C.byref(sy), C.byref(res),
                                                  C.byref(ox), C.byref(oy)))
        cells = np.zeros((sy.value, sx.value), dtype=np.uint8)
        _lib.check(self._lib.neo_mpc_get_world_map(self._handle, C.c_void_p(cells.ctypes.data), None, None, None, None, None))
        return cells, res.value, ox.value, oy.value

    def roll_costmap_pool(self, size_x, size_y, resolution, origins, poses=None, problems=None, outside_value=255):
        """Moves `count` windows of size_x x size_y cells to their robots and fills them from the world map (K7;
        nav2's rolling local costmaps, the contract: neo_mpc_window_batch in include/neo_mpc.h).  Afterwards the
        handle's costmap is this pool.  `origins` float64 [count, 2] is state: read, moved by whole cells and written
        in place.  `poses` [count, 3] (x, y, yaw -- the gate's array) centre the windows; without them
        `problems["cur_xy"]`; without both the windows stay where they are and are filled again.  NumPy arrays go
        through the synchronous host call; CUDA tensors (float64; `problems` the request records as bytes) through
        the device call on torch's current stream, which retains `origins` -- every later solve and gate reads it."""
        b = abi.NeoMpcWindowBatch()
        b.size_x, b.size_y, b.resolution = int(size_x), int(size_y), float(resolution)
        b.outside_value = int(outside_value)
        on_host = isinstance(origins, np.ndarray)
        origins, b.origins = self._array(origins, on_host, np.float64, (None, 2), coerce=False)
        b.count = count = origins.shape[0]
        if poses is not None:
            if on_host:
                poses = np.reshape(poses, (-1, 3))
            poses, b.poses = self._array(poses, on_host, np.float64, (count, 3))
        if problems is not None:
            problems, b.problems = self._array(problems, on_host, abi.PROBLEM_DTYPE, (count,), coerce=False)
        if not on_host:
            self._pool_origins = origins   # keep it alive
        self._call("neo_mpc_roll_costmap_pool", self._stream(on_host, origins), C.byref(b))
        if count:
            self._map_shape = (int(count), int(size_y), int(size_x))

    def get_costmap_pool(self, first=0, count=None):
        """The raw cells of maps [first, first + count) of the pool (or of the single map: a pool of one) the handle
        holds, uint8 [count, size_y, size_x] without border and pitch, and their origins, float64 [count, 2].
        Synchronous; waits for the ingest or roll in flight."""
        return self._pool_cells(self._lib.neo_mpc_get_costmap_pool, first, count)

    def _pool_cells(self, getter, first, count):
        """Cells of the pool's shape read back through `getter`, maps [first, first + count) -> (cells, origins)."""
        assert self._map_shape is not None, "no costmap has been set through this BatchSolver"
        maps, sy, sx = self._map_shape
        if count is None:
            count = maps - first
        cells = np.zeros((count, sy, sx), dtype=np.uint8)
        origins = np.zeros((count, 2), dtype=np.float64)
        _lib.check(getter(self._handle, int(first), int(count), C.c_void_p(cells.ctypes.data), C.c_void_p(origins.ctypes.data)))
        return cells, origins

    # -- fleet stamp (the step behind the roll) -------------------------------------------
    @staticmethod
    def inflation_costs(resolution, inscribed_radius, inflation_radius, cost_scaling_factor):
        """The cost table of the fleet stamp (`neo_mpc_inflation_costs`: nav2's `InflationLayer::computeCost` by squared
        cell distance) for windows of `resolution`: (T uint8 [R * R + 1], R).  Pure host arithmetic, no device."""
        lib = _lib.load()
        cells = C.c_uint32()
        args = (float(resolution), float(inscribed_radius), float(inflation_radius), float(cost_scaling_factor))
        _lib.check(lib.neo_mpc_inflation_costs(*args, None, 0, C.byref(cells)))
        table = np.zeros(cells.value * cells.value + 1, dtype=np.uint8)
        _lib.check(lib.neo_mpc_inflation_costs(*args, C.c_void_p(table.ctypes.data), table.size, None))
        return table, int(cells.value)

    def stamp_fleet(self, inscribed_radius, inflation_radius, cost_scaling_factor, polygons=None, footprint=None,
                    poses=None, problems=None):
        """Stamps the fleet's robots into each other's windows (K8; the contract: neo_mpc_stamp_batch in
        include/neo_mpc.h): window k of the pool the handle holds belongs to robot k and gets every OTHER robot's outline
        as lethal cells with nav2's inflation ring around them.  Either `polygons` [count, points, 2] in the global frame
        (what the footprint gate writes as `footprints_out`), or a base-frame `footprint` ([points, 2] shared, or
        [count, points, 2]) with `poses` [count, 3] or `problems`.  NumPy arrays go through the synchronous host call;
        CUDA tensors (float64; `problems` the request records as bytes) through the device call on torch's current
        stream."""
        b = abi.NeoMpcStampBatch()
        b.inscribed_radius, b.inflation_radius = float(inscribed_radius), float(inflation_radius)
        b.cost_scaling_factor = float(cost_scaling_factor)
        shape = polygons if polygons is not None else footprint
        assert shape is not None, "polygons or footprint"
        on_host = isinstance(shape, np.ndarray) or not hasattr(shape, "data_ptr")
        if on_host:
            if polygons is None and poses is not None:
                poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
            assert polygons is not None or poses is not None or problems is None or problems.dtype == abi.PROBLEM_DTYPE
        else:
            for a in (polygons, footprint, poses, problems):
                assert a is None or (a.is_cuda and a.is_contiguous())
        b.count, keep = self._outlines(b, on_host, polygons, footprint, poses, problems)
        self._call("neo_mpc_stamp_fleet", self._stream(on_host, shape), C.byref(b))

    @staticmethod
    def _outlines(rec, on_host, polygons=None, footprint=None, poses=None, problems=None, count=None):
        """Marshals a fleet's outlines -- `polygons` [count, points, 2], or `footprint` ([points, 2] or [count, points, 2])
        with `poses` [count, 3] or `problems` -- into the fields of those names of `rec` (neo_mpc_stamp_batch,
        neo_mpc_fleet_clear), with footprint_points and per_robot_footprints: from NumPy arrays (`on_host`) or CUDA tensors
        (float64; `problems` the request records).  `count`: what the arrays must agree with, or None: what they give (0
        without any) -> (count, what must stay alive)."""
        keep = []

        def ptr(a, dims):   # (dims None: records, taken as they are)
            a, address = BatchSolver._array(a, on_host, None if dims is None else np.float64)
            assert dims is None or len(a.shape) in dims
            keep.append(a)
            return a, address

        given = None
        if polygons is not None:
            polygons, rec.polygons = ptr(polygons, (3,))
            assert polygons.shape[2] == 2
            given, rec.footprint_points = polygons.shape[0], polygons.shape[1]
        else:
            footprint, rec.footprint = ptr(footprint, (2, 3))
            assert footprint.shape[-1] == 2
            rec.footprint_points = footprint.shape[-2]
            rec.per_robot_footprints = 1 if len(footprint.shape) == 3 else 0
            if poses is not None:
                poses, rec.poses = ptr(poses, (2,))
                assert poses.shape[1] == 3
                given = poses.shape[0]
            elif problems is not None:
                problems, rec.problems = ptr(problems, None)
                given = problems.shape[0]
        if count is None:
            count = given or 0
        assert given is None or given == count
        assert polygons is not None or len(footprint.shape) == 2 or footprint.shape[0] == count
        return int(count), keep

    # -- scan obstacle layer (the step between the roll and the stamp) --------------------
    def update_scan_layer(self, inscribed_radius, inflation_radius, cost_scaling_factor, points=None, sensor_origins=None,
                          point_counts=None, flags=None, obstacle_max_range=2.5, obstacle_min_range=0.0,
                          raytrace_max_range=3.0, raytrace_min_range=0.0, unknown_value=255, on_device=None):
        """Updates the obstacle layer of every window of the pool from one observation per robot and puts the layers into
        the windows (K10; the contract: neo_mpc_scan_batch in include/neo_mpc.h).  `points` [count, max_points, 2] hit
        points and `sensor_origins` [count, 2], global frame; `point_counts` (uint32 [count]) for ragged clouds; `flags`
        abi.SCAN_CLEAR | abi.SCAN_MARK (the default with points) or 0 (the default without: no new observation, the layer
        is rolled and applied again; the range defaults are nav2's).  NumPy arrays go through the synchronous host call;
        CUDA tensors (float64, `point_counts` int32 holding the uint32 counts) through the device call on torch's current
        stream.  Without points `on_device` picks the variant (a torch device, or True for this solver's)."""
        assert self._map_shape is not None, "no costmap has been set through this BatchSolver"
        b, stream, _ = self._scan_batch(self._map_shape[0], inscribed_radius, inflation_radius, cost_scaling_factor, points,
                                        sensor_origins, point_counts, flags, obstacle_max_range, obstacle_min_range,
                                        raytrace_max_range, raytrace_min_range, unknown_value, on_device)
        self._call("neo_mpc_update_scan_layer", stream, C.byref(b))

    def _scan_batch(self, count, inscribed_radius, inflation_radius, cost_scaling_factor, points, sensor_origins, point_counts,
                    flags, obstacle_max_range, obstacle_min_range, raytrace_max_range, raytrace_min_range, unknown_value,
                    on_device):
        """-> (neo_mpc_scan_batch over `count` robots, the stream or None for the host variant, what must stay alive)."""
        b = abi.NeoMpcScanBatch()
        b.count = int(count)
        b.obstacle_max_range, b.obstacle_min_range = float(obstacle_max_range), float(obstacle_min_range)
        b.raytrace_max_range, b.raytrace_min_range = float(raytrace_max_range), float(raytrace_min_range)
        b.inscribed_radius, b.inflation_radius = float(inscribed_radius), float(inflation_radius)
        b.cost_scaling_factor, b.unknown_value = float(cost_scaling_factor), int(unknown_value)
        if flags is None:
            flags = (abi.SCAN_CLEAR | abi.SCAN_MARK) if points is not None else 0
        b.flags = int(flags)
        device = None
        if points is not None and hasattr(points, "data_ptr"):
            device = points.device
        elif points is None and on_device is not None and on_device is not False:
            import torch
            device = torch.device("cuda", self.device) if on_device is True else torch.device(on_device)
        on_host = device is None
        if points is not None:
            points, b.points = self._array(points, on_host, np.float64, (b.count, None, 2))
            sensor_origins, b.sensor_origins = self._array(sensor_origins, on_host, np.float64, (b.count, 2))
            b.max_points = points.shape[1]
            if point_counts is not None:
                point_counts, b.point_counts = self._array(point_counts, on_host, np.uint32, (b.count,))
        return b, self._stream(on_host, device), (points, sensor_origins, point_counts)

    # -- the scan step fed from LaserScan ranges -----------------------------------------
    def _laser_batch(self, ranges, poses, scanners, points_out, origins_out, need_out):
        """-> (the record with everything but the update's fields, what must stay alive, points_out, origins_out, the
        stream or None for the host variant)."""
        b = abi.NeoMpcLaserBatch()
        sc = abi.scanner_array(scanners)
        b.scanners, b.sources = sc.ctypes.data, sc.shape[0]
        on_host = not hasattr(ranges, "data_ptr")
        ranges, b.ranges = self._array(ranges, on_host, np.float32, (None, b.sources, None))
        count, _, beams = ranges.shape
        b.count, b.beams = count, beams
        poses, b.poses = self._array(poses, on_host, np.float64, (count, 3))

        def out(a, shape):   # an output: the caller's, taken as it is, or -- where the call needs one -- a fresh one
            if a is None and need_out:
                if on_host:
                    a = np.zeros(shape, dtype=np.float64)
                else:
                    import torch
                    a = torch.zeros(shape, dtype=torch.float64, device=ranges.device)
            return (None, None) if a is None else self._array(a, on_host, np.float64, shape, coerce=False)

        points_out, b.points_out = out(points_out, (count, b.sources, beams, 2))
        origins_out, b.origins_out = out(origins_out, (count, b.sources, 2))
        return b, (sc, ranges, poses), points_out, origins_out, self._stream(on_host, ranges)

    def _laser_update(self, ranges, poses, scanners, points_out, origins_out, flags, unknown_value, obstacle_max_range,
                      obstacle_min_range, raytrace_max_range, raytrace_min_range, inscribed_radius, inflation_radius,
                      cost_scaling_factor):
        """-> (`_laser_batch`'s record with the update's fields filled, what must stay alive, the stream or None)."""
        b, keep, _, _, stream = self._laser_batch(ranges, poses, scanners, points_out, origins_out, False)
        b.scan_flags = int(abi.SCAN_CLEAR | abi.SCAN_MARK if flags is None else flags)
        b.unknown_value = int(unknown_value)
        b.obstacle_max_range, b.obstacle_min_range = float(obstacle_max_range), float(obstacle_min_range)
        b.raytrace_max_range, b.raytrace_min_range = float(raytrace_max_range), float(raytrace_min_range)
        b.inscribed_radius, b.inflation_radius = float(inscribed_radius), float(inflation_radius)
        b.cost_scaling_factor = float(cost_scaling_factor)
        return b, keep, stream

    def project_laser(self, ranges, poses, scanners, points_out=None, origins_out=None):
        """Projects LaserScan `ranges` (float32 [count, sources, beams], as on the wire) of robots at `poses` (float64
        [count, 3]: x, y, yaw) into global-frame hit points [count, sources, beams, 2] -- (NaN, NaN) for a beam that is not
        valid -- and sensor origins [count, sources, 2], and returns the two (K11; the contract: neo_mpc_laser_batch in
        include/neo_mpc.h).  `scanners`: what abi.scanner_array takes, host configuration.  NumPy arrays go through the
        synchronous host call; CUDA tensors through the device call on torch's current stream.  Needs no costmap."""
        b, keep, points_out, origins_out, stream = self._laser_batch(ranges, poses, scanners, points_out, origins_out, True)
        self._call("neo_mpc_project_laser", stream, C.byref(b))
        return points_out, origins_out

    def update_scan_layer_from_ranges(self, inscribed_radius, inflation_radius, cost_scaling_factor, ranges, poses, scanners,
                                      flags=None, points_out=None, origins_out=None, obstacle_max_range=2.5,
                                      obstacle_min_range=0.0, raytrace_max_range=3.0, raytrace_min_range=0.0,
                                      unknown_value=255):
        """Projects the ranges as `project_laser` does and updates the obstacle layer of every window of the pool from all
        scanners: every clear of every scanner, then every mark (K11 and K10; the contract: neo_mpc_laser_batch).  `flags`
        abi.SCAN_CLEAR | abi.SCAN_MARK (the default) or one of them; a tick without a new scan is `update_scan_layer`
        without points.  `points_out` / `origins_out` receive what was projected when given.  NumPy arrays go through the
        synchronous host call; CUDA tensors through the device call on torch's current stream."""
        b, keep, stream = self._laser_update(ranges, poses, scanners, points_out, origins_out, flags, unknown_value,
                                             obstacle_max_range, obstacle_min_range, raytrace_max_range, raytrace_min_range,
                                             inscribed_radius, inflation_radius, cost_scaling_factor)
        self._call("neo_mpc_update_scan_layer_from_ranges", stream, C.byref(b))

    def get_scan_layer(self, first=0, count=None):
        """Layers [first, first + count) as the last `update_scan_layer` left them: uint8 [count, size_y, size_x] with
        values in {255, 0, 254}, and their origins, float64 [count, 2].  Synchronous; waits for the update in flight."""
        return self._pool_cells(self._lib.neo_mpc_get_scan_layer, first, count)

    def reset_scan_layer(self):
        """The next `update_scan_layer` starts from a layer of `unknown_value`."""
        _lib.check(self._lib.neo_mpc_reset_scan_layer(self._handle))

    # -- the fleet's shared obstacle layer on the world map (in front of the roll) ---------
    @staticmethod
    def _fleet_clear(clear, count, on_host):
        """`clear` = None, or a mapping with `padding` (m) and either `polygons` [count, points, 2] or `footprint` ([points, 2]
        or [count, points, 2]) with `poses` [count, 3] or `problems` -> (neo_mpc_fleet_clear or None, what must stay alive)."""
        if clear is None:
            return None, None
        assert set(clear) <= {"padding", "polygons", "footprint", "poses", "problems"}, sorted(clear)
        c = abi.NeoMpcFleetClear()
        c.padding = float(clear.get("padding", 0.0))
        c.count, keep = BatchSolver._outlines(c, on_host, clear.get("polygons"), clear.get("footprint"), clear.get("poses"),
                                              clear.get("problems"), count=int(count))
        return c, keep

    def update_world_scan_layer(self, inscribed_radius, inflation_radius, cost_scaling_factor, points=None, sensor_origins=None,
                                point_counts=None, flags=None, clear=None, count=None, obstacle_max_range=2.5,
                                obstacle_min_range=0.0, raytrace_max_range=3.0, raytrace_min_range=0.0, unknown_value=255,
                                on_device=None):
        """Updates the fleet's shared obstacle layer on the world map from one observation per robot and composes the map
        the next `roll_costmap_pool` cuts its windows from (K12; the contract: neo_mpc_fleet_clear in include/neo_mpc.h):
        world scan -> roll -> stamp -> gate -> carrots -> solve.  Points, flags, ranges and `on_device` as
        `update_scan_layer`; the number of robots is that of `points`, else of `clear`'s arrays, else `count` (default 1),
        and is not tied to the pool's.  `clear` = a mapping with `padding` (metres) and either `polygons` or `footprint`
        with `poses` or `problems`, as `stamp_fleet` takes them: the robots' own outlines are set free in the layer."""
        if points is not None:
            count = points.shape[0]
        elif clear is not None:
            count = next(clear[k].shape[0] for k in ("polygons", "poses", "problems") if clear.get(k) is not None)
        elif count is None:
            count = 1
        b, stream, keep = self._scan_batch(count, inscribed_radius, inflation_radius, cost_scaling_factor, points,
                                           sensor_origins, point_counts, flags, obstacle_max_range, obstacle_min_range,
                                           raytrace_max_range, raytrace_min_range, unknown_value, on_device)
        c, keep_c = self._fleet_clear(clear, count, stream is None)
        self._call("neo_mpc_update_world_scan_layer", stream, C.byref(b), C.byref(c) if c is not None else None)

    def update_world_scan_layer_from_ranges(self, inscribed_radius, inflation_radius, cost_scaling_factor, ranges, poses,
                                            scanners, flags=None, clear=None, points_out=None, origins_out=None,
                                            obstacle_max_range=2.5, obstacle_min_range=0.0, raytrace_max_range=3.0,
                                            raytrace_min_range=0.0, unknown_value=255):
        """Projects the ranges as `project_laser` does and updates the fleet's shared layer on the world map from all
        scanners of all robots (K11 and K12).  Arguments as `update_scan_layer_from_ranges`; `clear` as
        `update_world_scan_layer`."""
        b, keep, stream = self._laser_update(ranges, poses, scanners, points_out, origins_out, flags, unknown_value,
                                             obstacle_max_range, obstacle_min_range, raytrace_max_range, raytrace_min_range,
                                             inscribed_radius, inflation_radius, cost_scaling_factor)
        c, keep_c = self._fleet_clear(clear, b.count, stream is None)
        self._call("neo_mpc_update_world_scan_layer_from_ranges", stream, C.byref(b), C.byref(c) if c is not None else None)

    def get_world_scan_layer(self):
        """(layer, live), uint8 [size_y, size_x] each on the world map's geometry: the fleet's shared layer, values in
        {255, 0, 254}, and the world map with the layer merged in and inflated, as the last `update_world_scan_layer` left
        them.  Synchronous; waits for the update in flight."""
        return self._world_cells(self._lib.neo_mpc_get_world_scan_layer, np.uint8, np.uint8)

    def _world_cells(self, getter, *dtypes):
        """Cells of the world's shape read back through `getter`, one array per dtype: asks `getter` without arrays first, so
        that what it refuses is refused before anything is made, then the world map for its size -> the arrays."""
        _lib.check(getter(self._handle, *[None] * len(dtypes)))
        sx, sy = C.c_uint32(), C.c_uint32()
        _lib.check(self._lib.neo_mpc_get_world_map(self._handle, None, C.byref(sx), C.byref(sy), None, None, None))
        cells = tuple(np.zeros((sy.value, sx.value), dtype=dtype) for dtype in dtypes)
        _lib.check(getter(self._handle, *[C.c_void_p(a.ctypes.data) for a in cells]))
        return cells

    def reset_world_scan_layer(self):
        """The next `update_world_scan_layer` starts from a layer of `unknown_value`; until then the roll reads the world
        map."""
        _lib.check(self._lib.neo_mpc_reset_world_scan_layer(self._handle))

    def set_world_scan_denoise(self, minimal_group_size, connectivity=8):
        """The speckle filter of the fleet's shared layer (K13; the contract: step 3b of neo_mpc_fleet_clear's text in
        include/neo_mpc.h): from the next `update_world_scan_layer` on, a mark whose group of occupied cells -- marks and
        the world map's own 254 cells, connected over 4 or 8 neighbours -- has fewer than `minimal_group_size` members
        reaches `live` as a free cell; the layer keeps it.  0 or 1 switches the filter off; at most `abi.MAX_DENOISE_GROUP`.
        Handle configuration: it survives `reset_world_scan_layer` and `set_world_map`."""
        _lib.check(self._lib.neo_mpc_set_world_scan_denoise(self._handle, int(minimal_group_size), int(connectivity)))

    def get_world_scan_denoised(self):
        """uint8 [size_y, size_x] on the world map's geometry: the layer as the composition of the last
        `update_world_scan_layer` read it -- the layer itself when the filter was off.  Synchronous; waits for the update in
        flight."""
        return self._world_cells(self._lib.neo_mpc_get_world_scan_denoised, np.uint8)[0]

    def set_world_scan_decay(self, max_age):
        """The decay of the fleet's shared layer (K14; the contract: step 2b of neo_mpc_fleet_clear's text in
        include/neo_mpc.h): from the next `update_world_scan_layer` on, a mark that no scan update -- an update with
        abi.SCAN_MARK in its flags -- has made again for `max_age` scan updates becomes `unknown_value` in the layer itself.
        0 switches it off.  Handle configuration: it survives `reset_world_scan_layer` and `set_world_map`."""
        _lib.check(self._lib.neo_mpc_set_world_scan_decay(self._handle, int(max_age)))

    def get_world_scan_ages(self):
        """uint32 [size_y, size_x] on the world map's geometry: under a mark of the layer the number of scan updates since it
        was last made (0: by the last one), `abi.NO_AGE` elsewhere, as the last `update_world_scan_layer` left them.  Refused
        when that update ran without decay.  Synchronous; waits for the update in flight."""
        return self._world_cells(self._lib.neo_mpc_get_world_scan_ages, np.uint32)[0]

    HOST_PATHS = {"auto": 0, "staged": 1, "zerocopy": 2, "zerocopy_out": 3}

    def set_host_path(self, mode):
        """How `solve` moves a batch whose arrays are all page-locked: "auto" (= "zerocopy": K1 works on the
        caller's arrays in place over PCIe), "staged" (DMA copies in and out), "zerocopy_out" (DMA in, results
        written in place)."""
        _lib.check(self._lib.neo_mpc_set_host_path(self._handle, self.HOST_PATHS[mode]))

    def kernel_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(self._lib.neo_mpc_kernel_info(self._handle, C.byref(a), C.byref(b), C.byref(c)))
        return dict(lds_bytes=a.value, reach_cells=b.value, tile_in_lds=bool(c.value))

    # -- host batches ----------------------------------------------------------------
    def _host_batch(self, problems, states, warm, solution, want_path, footprints, commands=None):
        n = self.control_steps
        problems = np.ascontiguousarray(problems, dtype=abi.PROBLEM_DTYPE)
        count = problems.shape[0]
        assert states.dtype == abi.STATE_DTYPE and states.shape == (count,) and states.flags.c_contiguous
        assert warm.dtype == np.float64 and warm.shape == (count, 3 * n) and warm.flags.c_contiguous
        if commands is None:
            commands = np.zeros(count, dtype=abi.COMMAND_DTYPE)
        assert commands.dtype == abi.COMMAND_DTYPE and commands.shape == (count,) and commands.flags.c_contiguous
        path = np.zeros((count, n, 3)) if want_path else None
        if footprints is not None:
            footprints = np.ascontiguousarray(footprints, dtype=np.float64)
            assert footprints.shape[0] == count and footprints.shape[2] == 2
        b = abi.batch_struct(problems, states, warm, commands, solution, path, footprints)
        self._keep = (problems, footprints)
        return b, commands, path

    def solve(self, problems, states, warm, want_path=False, footprints=None, out=None):
        """`optimizer()` (py:349-403) for a batch of host records.  `states` / `warm` are
        updated in place.  Returns (commands, solution[, path]).  `out` = (commands, solution) arrays to fill
        instead of fresh ones -- page-locked ones (with page-locked inputs) make every transfer of the call a DMA."""
        count = len(problems)
        if out is not None and not want_path and footprints is None:
            # a caller that owns its arrays (a fleet server's request arena) passes the same ones every tick: the
            # marshalled batch of the previous call is reused as long as every array is the same object
            # (address and shape are part of the key: an array resized or re-allocated in place keeps its id())
            key = tuple((id(a), a.ctypes.data, a.shape) for a in (problems, states, warm, out[0], out[1]))
            if self._last_call is not None and self._last_call[0] == key:
                _lib.check(self._lib.neo_mpc_solve_batch(self._handle, self._last_call[1]))
                return out
        commands, solution = out if out is not None else (None, np.zeros((count, 3 * self.control_steps)))
        assert solution.dtype == np.float64 and solution.shape == (count, 3 * self.control_steps) and solution.flags.c_contiguous
        b, commands, path = self._host_batch(problems, states, warm, solution, want_path, footprints, commands)
        if out is not None and not want_path and footprints is None and self._keep[0] is problems:
            self._last_call = (key, C.byref(b), b, (problems, states, warm, out))   # (keeps the arrays and the struct alive)
        _lib.check(self._lib.neo_mpc_solve_batch(self._handle, C.byref(b)))
        return (commands, solution, path) if want_path else (commands, solution)

    def solve_begin(self, problems, states, warm, out):
        """First half of `solve` for page-locked arrays (`client->async_send_request(request)`, cpp:248): enqueues the
        batch -- it is worked on in place -- and returns a ticket for `solve_wait`.  `out` = (commands, solution).  The
        arrays must stay untouched (and alive) until the wait; up to four batches may be in flight."""
        assert problems.dtype == abi.PROBLEM_DTYPE and problems.flags.c_contiguous
        b, _, _ = self._host_batch(problems, states, warm, out[1], False, None, out[0])
        ticket = C.c_uint32(0)
        _lib.check(self._lib.neo_mpc_solve_batch_begin(self._handle, C.byref(b), C.byref(ticket)))
        self._in_flight[ticket.value] = (b, problems, states, warm, out)
        return ticket.value

    def solve_wait(self, ticket):
        """Second half (`result.get()`, cpp:250): blocks until the batch of `ticket` is done; its results are then in the
        arrays handed to `solve_begin`, which are returned."""
        try:
            _lib.check(self._lib.neo_mpc_solve_batch_wait(self._handle, C.c_uint32(ticket)))
        except Exception:
            self._in_flight.pop(ticket, None)   # (the library has given the slot up either way: no stale entry)
            raise
        return self._in_flight.pop(ticket)[4]

    def postprocess(self, problems, states, warm, solution, success=None, want_path=False, footprints=None):
        """Everything of `optimizer()` after the solve (py:365-403) with `solution` = x.x."""
        solution = np.ascontiguousarray(solution, dtype=np.float64)
        b, commands, path = self._host_batch(problems, states, warm, solution, want_path, footprints)
        sp = None
        if success is not None:
            success = np.ascontiguousarray(success, dtype=np.int32)
            sp = C.c_void_p(success.ctypes.data)
        _lib.check(self._lib.neo_mpc_postprocess_batch(self._handle, C.byref(b), sp))
        return (commands, path) if want_path else commands

    def objective(self, problems, u):
        """`objective()` (py:204-269) on the device for u[count, 3*control_steps]."""
        problems = np.ascontiguousarray(problems, dtype=abi.PROBLEM_DTYPE)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.zeros(len(problems))
        _lib.check(self._lib.neo_mpc_objective_batch(
            self._handle, C.c_void_p(problems.ctypes.data), C.c_void_p(u.ctypes.data),
            C.c_void_p(out.ctypes.data), len(problems)))
        return out

    def gradient(self, problems, u):
        """Test hook: the total gradient the solve kernel works with at `u` (projected like x0):
        analytic adjoint gradient + gradient of the control norm, from inside the kernel variant
        the current parameters select."""
        problems = np.ascontiguousarray(problems, dtype=abi.PROBLEM_DTYPE)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.zeros_like(u)
        _lib.check(self._lib.neo_mpc_gradient_batch(
            self._handle, C.c_void_p(problems.ctypes.data), C.c_void_p(u.ctypes.data),
            C.c_void_p(out.ctypes.data), len(problems)))
        return out

    def direction(self, problems, u, iteration):
        """Test hook: the search direction of lanes 32-63 in solver iteration `iteration` (0-based) of a
        solve started from `u`; rows of instances that stopped earlier stay NaN."""
        problems = np.ascontiguousarray(problems, dtype=abi.PROBLEM_DTYPE)
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.full_like(u, np.nan)
        _lib.check(self._lib.neo_mpc_direction_batch(
            self._handle, C.c_void_p(problems.ctypes.data), C.c_void_p(u.ctypes.data),
            C.c_void_p(out.ctypes.data), len(problems), int(iteration)))
        return out

    # -- carrot selection (the step before the solver) ------------------------------------
    def select_carrots(self, plan_poses, plan_offsets, robot_poses, slow_down, footprint_costs=None,
                       problems=None, lookahead_dist_min=0.5, lookahead_dist_max=0.5,
                       lookahead_dist_close_to_goal=0.5, max_transform_dist=1e9):
        """Plan pruning + look-ahead point + slow_down_ update for a ragged batch of plans
        (NeoMpcPlanner.cpp:83-104, 157-189, 221-232).  `slow_down` (int32) is updated in place;
        when `problems` is given the carrot pose is written into the requests."""
        plan_poses = np.ascontiguousarray(plan_poses, dtype=np.float64).reshape(-1, 3)
        plan_offsets = np.ascontiguousarray(plan_offsets, dtype=np.uint32)
        robot_poses = np.ascontiguousarray(robot_poses, dtype=np.float64).reshape(-1, 3)
        count = robot_poses.shape[0]
        assert plan_offsets.shape == (count + 1,) and slow_down.dtype == np.int32 and slow_down.shape == (count,)
        carrots = np.zeros(count, dtype=abi.CARROT_DTYPE)
        lp = abi.NeoMpcLookaheadParams(lookahead_dist_min, lookahead_dist_max, lookahead_dist_close_to_goal,
                                       max_transform_dist)
        if footprint_costs is not None:
            footprint_costs = np.ascontiguousarray(footprint_costs, dtype=np.float64)
        if problems is not None:
            assert problems.dtype == abi.PROBLEM_DTYPE and problems.flags.c_contiguous
        b = self._plan_batch(True, count, plan_poses, plan_offsets, robot_poses, slow_down, carrots, footprint_costs, problems)
        _lib.check(self._lib.neo_mpc_select_carrots(self._handle, C.byref(lp), C.byref(b)))
        return carrots

    def _plan_batch(self, on_host, count, plan_poses, plan_offsets, robot_poses, slow_down, carrots, footprint_costs, problems):
        """neo_mpc_plan_batch over NumPy arrays (`on_host`) or CUDA tensors."""
        b = abi.NeoMpcPlanBatch()
        b.count = count
        (b.plan_poses, b.plan_offsets, b.robot_poses, b.footprint_costs, b.slow_down, b.carrots, b.problems) = self._addresses(
            on_host, plan_poses, plan_offsets, robot_poses, footprint_costs, slow_down, carrots, problems)
        return b

    def select_carrots_device(self, lp, plan_poses, plan_offsets, robot_poses, slow_down, carrots,
                              footprint_costs=None, problems=None, stream=None):
        """Device-resident variant: torch CUDA tensors; enqueues K4 on `stream`."""
        b = self._plan_batch(False, robot_poses.shape[0], plan_poses, plan_offsets, robot_poses, slow_down, carrots,
                             footprint_costs, problems)
        self._call("neo_mpc_select_carrots", self._stream(False, robot_poses) if stream is None else stream, C.byref(lp),
                   C.byref(b))

    # -- plan check (the fleet's plans against the live world map) -------------------------
    def _plan_check_batch(self, on_host, plan_poses, plan_offsets, results, robot_poses, footprint, max_cost, unknown_blocks,
                          outside_value, max_poses):
        """neo_mpc_plan_check_batch over NumPy arrays (`on_host`) or CUDA tensors."""
        b = abi.NeoMpcPlanCheckBatch()
        b.count = plan_offsets.shape[0] - 1
        b.footprint_points = footprint.shape[0] if footprint is not None else 0
        b.max_cost, b.unknown_blocks, b.outside_value, b.max_poses = int(max_cost), int(unknown_blocks), int(outside_value), int(max_poses)
        b.plan_poses, b.plan_offsets, b.results, b.robot_poses, b.footprint = self._addresses(
            on_host, plan_poses, plan_offsets, results, robot_poses, footprint)
        return b

    def check_plans(self, plan_poses, plan_offsets, robot_poses=None, footprint=None, max_cost=253, unknown_blocks=False,
                    outside_value=255, max_poses=0):
        """Which plans of a ragged batch (`select_carrots`' arrays, poses in the world map's frame) the world map the
        next roll would read blocks (K15; the contract: include/neo_mpc.h, neo_mpc_plan_check_batch).  With `robot_poses`
        [count, 3] the check starts at each plan's closest pose, else at pose 0; `footprint` [points, 2] (base frame,
        shared) selects footprint mode, None point mode.  Returns the records (abi.PLAN_CHECK_DTYPE [count])."""
        plan_poses = np.ascontiguousarray(plan_poses, dtype=np.float64).reshape(-1, 3)
        plan_offsets = np.ascontiguousarray(plan_offsets, dtype=np.uint32)
        count = plan_offsets.shape[0] - 1
        results = np.zeros(count, dtype=abi.PLAN_CHECK_DTYPE)
        if footprint is not None:
            footprint = np.ascontiguousarray(footprint, dtype=np.float64)
            assert footprint.ndim == 2 and footprint.shape[1] == 2
        if robot_poses is not None:
            robot_poses = np.ascontiguousarray(robot_poses, dtype=np.float64).reshape(-1, 3)
            assert robot_poses.shape[0] == count
        b = self._plan_check_batch(True, plan_poses, plan_offsets, results, robot_poses, footprint, max_cost, unknown_blocks,
                                   outside_value, max_poses)
        _lib.check(self._lib.neo_mpc_check_plans(self._handle, C.byref(b)))
        return results

    def check_plans_device(self, plan_poses, plan_offsets, results, robot_poses=None, footprint=None, max_cost=253,
                           unknown_blocks=False, outside_value=255, max_poses=0, stream=None):
        """Device-resident variant: contiguous torch CUDA tensors (float64; `plan_offsets` [count + 1] as int32 or uint32
        bits; `results` the records as bytes, 24 a robot); enqueues K15 on `stream` (default: torch's current) and
        returns without waiting.  Capturable in a HIP graph behind one call of the same shape."""
        b = self._plan_check_batch(False, plan_poses, plan_offsets, results, robot_poses, footprint, max_cost, unknown_blocks,
                                   outside_value, max_poses)
        self._call("neo_mpc_check_plans", self._stream(False, results) if stream is None else stream, C.byref(b))

    # -- grid planner (detours for the plans the live world map blocks) ---------------------
    def _replan_batch(self, on_host, starts, goals, checks, path_cells, path_poses, results, window, max_cost, unknown_cost,
                      neutral_cost):
        """neo_mpc_replan_batch over NumPy arrays (`on_host`) or CUDA tensors; the stride is `path_cells`' second dimension."""
        b = abi.NeoMpcReplanBatch()
        count = b.count = starts.shape[0]
        b.window, b.max_cost, b.unknown_cost, b.neutral_cost = int(window), int(max_cost), int(unknown_cost), int(neutral_cost)
        stride = b.max_path_cells = path_cells.shape[1]
        records = (count,) if on_host else None       # (a tensor holds records as bytes, flat or [count, 24])
        _, b.starts = self._array(starts, on_host, np.float64, (count, 2), coerce=False)
        _, b.goals = self._array(goals, on_host, np.float64, (count, 2), coerce=False)
        _, b.path_cells = self._array(path_cells, on_host, np.int32, (count, stride, 2), coerce=False)
        _, b.results = self._array(results, on_host, abi.REPLAN_DTYPE, records, coerce=False)
        if checks is not None:
            _, b.checks = self._array(checks, on_host, abi.PLAN_CHECK_DTYPE, records, coerce=False)
        if path_poses is not None:
            _, b.path_poses = self._array(path_poses, on_host, np.float64, (count, stride, 3), coerce=False)
        return b

    def replan_plans(self, starts, goals, window, checks=None, max_cost=253, unknown_cost=0, neutral_cost=50,
                     max_path_cells=None, want_poses=False):
        """A path from `starts[i]` to `goals[i]` ([count, 2], the world map's frame) for every robot, searched inside a window
        of `window` x `window` cells of the world map the next roll would read (K16; the contract: include/neo_mpc.h,
        neo_mpc_replan_batch).  `checks`: `check_plans`' records as a mask -- only robots with status 1 are searched.
        `max_path_cells` (default window * window: every path fits) is the stride of the outputs.  Returns (records
        abi.REPLAN_DTYPE [count], path_cells int32 [count, max_path_cells, 2][, path_poses float64 [count, max_path_cells, 3]
        with `want_poses`]); entries beyond a path stay 0."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 2)
        goals = np.ascontiguousarray(goals, dtype=np.float64).reshape(-1, 2)
        count = starts.shape[0]
        stride = int(window) * int(window) if max_path_cells is None else int(max_path_cells)
        results = np.zeros(count, dtype=abi.REPLAN_DTYPE)
        path_cells = np.zeros((count, stride, 2), dtype=np.int32)
        path_poses = np.zeros((count, stride, 3), dtype=np.float64) if want_poses else None
        if checks is not None:
            checks = np.ascontiguousarray(checks, dtype=abi.PLAN_CHECK_DTYPE)
        b = self._replan_batch(True, starts, goals, checks, path_cells, path_poses, results, window, max_cost, unknown_cost,
                               neutral_cost)
        self._call("neo_mpc_replan_plans", None, C.byref(b))
        return (results, path_cells, path_poses) if want_poses else (results, path_cells)

    def replan_plans_device(self, starts, goals, window, path_cells, results, checks=None, path_poses=None, max_cost=253,
                            unknown_cost=0, neutral_cost=50, stream=None):
        """Device-resident variant: contiguous torch CUDA tensors (`starts`, `goals` float64 [count, 2]; `path_cells` int32
        [count, max_path_cells, 2]; `path_poses` float64 [count, max_path_cells, 3] or None; `results` and `checks` the
        records as bytes, 24 a robot -- `checks` may be what `check_plans_device` wrote on the same stream); enqueues K16 on
        `stream` (default: torch's current) and returns without waiting.  Capturable in a HIP graph."""
        b = self._replan_batch(False, starts, goals, checks, path_cells, path_poses, results, window, max_cost, unknown_cost,
                               neutral_cost)
        self._call("neo_mpc_replan_plans", self._stream(False, results) if stream is None else stream, C.byref(b))

    # -- footprint gate (the step before the carrot) --------------------------------------
    def footprint_gate(self, footprint, poses=None, problems=None, map_indices=None, want_polygons=False):
        """`footprintCostAtPose` (NeoMpcPlanner.cpp:218-219; nav2's FootprintCollisionChecker on raw cell values) for a
        batch of host arrays.  `footprint`: the base-frame polygon, [points, 2] shared by every robot or
        [count, points, 2] one per robot.  `poses` [count, 3] (x, y, yaw); without them `problems` supplies cur_xy and
        the yaw of cur_q.  `map_indices` (int32) picks the map of a pool; without it problems["map_index"], else map 0.
        When `problems` is given its footprint_cost is set in place (1.0 where the cost is >= 254, else 0.0).
        Returns the costs on nav2's 0..255 scale (float64 [count]) -- what `select_carrots(footprint_costs=...)`
        takes -- and with `want_polygons` also the oriented polygons [count, points, 2] (`solve(footprints=...)`)."""
        footprint = np.ascontiguousarray(footprint, dtype=np.float64)
        assert footprint.ndim in (2, 3) and footprint.shape[-1] == 2
        if poses is not None:
            poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
            count = poses.shape[0]
        else:
            assert problems is not None, "poses or problems"
            count = problems.shape[0]
        if problems is not None:
            assert problems.dtype == abi.PROBLEM_DTYPE and problems.shape == (count,) and problems.flags.c_contiguous
        if map_indices is not None:
            map_indices = np.ascontiguousarray(map_indices, dtype=np.int32)
            assert map_indices.shape == (count,)
        assert footprint.ndim == 2 or footprint.shape[0] == count
        costs = np.zeros(count, dtype=np.float64)
        polygons = np.zeros((count, footprint.shape[-2], 2), dtype=np.float64) if want_polygons else None
        b = self._footprint_batch(True, footprint, costs, poses, problems, map_indices, polygons)
        _lib.check(self._lib.neo_mpc_footprint_gate(self._handle, C.byref(b)))
        return (costs, polygons) if want_polygons else costs

    def _footprint_batch(self, on_host, footprint, footprint_costs, poses, problems, map_indices, footprints_out):
        """neo_mpc_footprint_batch over NumPy arrays (`on_host`) or CUDA tensors."""
        b = abi.NeoMpcFootprintBatch()
        b.count = footprint_costs.shape[0]
        b.footprint_points = footprint.shape[-2]
        b.per_robot_footprints = 1 if len(footprint.shape) == 3 else 0
        b.footprint, b.poses, b.map_indices, b.problems, b.footprint_costs, b.footprints_out = self._addresses(
            on_host, footprint, poses, map_indices, problems, footprint_costs, footprints_out)
        return b

    def footprint_gate_device(self, footprint, footprint_costs, poses=None, problems=None, map_indices=None,
                              footprints_out=None, stream=None):
        """Device-resident variant: contiguous torch CUDA tensors (float64; `map_indices` int32; `problems` the request
        records as bytes); enqueues K6 on `stream` (default: torch's current) and returns without waiting.
        `footprint_costs` [count] and the optional `footprints_out` [count, points, 2] are written; `footprint` is
        [points, 2] or [count, points, 2]."""
        b = self._footprint_batch(False, footprint, footprint_costs, poses, problems, map_indices, footprints_out)
        self._call("neo_mpc_footprint_gate", self._stream(False, footprint_costs) if stream is None else stream, C.byref(b))

    # -- device-resident batches (torch tensors as plain device memory) ----------------
    def balance_dispatch(self, commands, stream=None):
        """Dispatch order of the following device solves of the same count from the iteration counts in `commands` (a CUDA
        uint8 tensor of command records, e.g. the previous tick's; None: back to launch order) --
        neo_mpc_balance_dispatch_device.  Enqueued on `stream` (default: torch's current).  Changes no result."""
        if commands is None:
            _lib.check(self._lib.neo_mpc_balance_dispatch_device(self._handle, None, 0, None))
            return
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(commands.device).cuda_stream
        _lib.check(self._lib.neo_mpc_balance_dispatch_device(self._handle, C.c_void_p(commands.data_ptr()), commands.shape[0],
                                                             C.c_void_p(stream)))

    def dispatch_order(self):
        """Test hook (neo_mpc_get_dispatch_order): what the last `balance_dispatch` left in the handle -> (order, load), or
        None when no order is armed.  `order` uint32 [count]: workgroup w of the next device solve of that count solves
        instance order[w].  `load` float32 [count]: the averages the order is sorted by -- None for a count that gets launch
        order (not a multiple of 1024, or beyond 4096), which has none.  Synchronous; waits for the device."""
        count = C.c_size_t()
        _lib.check(self._lib.neo_mpc_get_dispatch_order(self._handle, None, None, C.byref(count)))
        if count.value == 0:
            return None
        order = np.zeros(count.value, dtype=np.uint32)
        load = np.zeros(count.value, dtype=np.float32) if count.value % 1024 == 0 and count.value <= 4096 else None
        _lib.check(self._lib.neo_mpc_get_dispatch_order(self._handle, *self._addresses(True, order, load), C.byref(count)))
        assert count.value == len(order)
        return order, load

    def solve_device(self, problems, states, warm, commands, solution=None, path=None, footprints=None,
                     stream=None, velocities=None, events=None):
        """All arguments are CUDA uint8/float64 torch tensors holding the C records
        (`DeviceBatch` builds them).  Enqueues K1 on `stream` (default: torch's current).
        `events` = (start, stop) torch.cuda.Event pair, already created (recorded once): stamped by
        the kernel dispatch itself (`neo_mpc_solve_batch_device_timed`)."""
        import torch
        count = problems.shape[0]
        b = abi.NeoMpcBatch()
        b.count = count
        b.problems = problems.data_ptr()
        b.states = states.data_ptr()
        b.warm_start = warm.data_ptr()
        b.commands = commands.data_ptr()
        b.solution = solution.data_ptr() if solution is not None else None
        b.predicted_path = path.data_ptr() if path is not None else None
        if footprints is not None:
            b.footprints = footprints.data_ptr()
            b.footprint_points = footprints.shape[1]
        if velocities is not None:
            b.velocities = velocities.data_ptr()
        if stream is None:
            stream = torch.cuda.current_stream(problems.device).cuda_stream
        if events is None:
            _lib.check(self._lib.neo_mpc_solve_batch_device(self._handle, C.byref(b), C.c_void_p(stream)))
        else:
            _lib.check(self._lib.neo_mpc_solve_batch_device_timed(
                self._handle, C.byref(b), C.c_void_p(stream), C.c_void_p(events[0].cuda_event),
                C.c_void_p(events[1].cuda_event)))


class DeviceBatch:
    """A batch resident in HBM: the C records as torch CUDA byte/float64 tensors."""

    def __init__(self, problems, states, warm, device, want_solution=True):
        import torch
        self.count = len(problems)
        dev = torch.device(device)
        self.problems = torch.from_numpy(np.ascontiguousarray(problems).view(np.uint8).reshape(self.count, -1)).to(dev)
        self.states = torch.from_numpy(np.ascontiguousarray(states).view(np.uint8).reshape(self.count, -1)).to(dev)
        self.warm = torch.from_numpy(np.ascontiguousarray(warm)).to(dev)
        self.commands = torch.zeros((self.count, abi.COMMAND_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        self.solution = torch.zeros_like(self.warm) if want_solution else None
        self.vel = torch.zeros((self.count, 3), dtype=torch.float64, device=dev)   # packed (vx, vy, w)

    def fresh_state(self):
        """Another (states, warm, commands) set for the same problems (shares `problems`)."""
        import torch
        other = object.__new__(DeviceBatch)
        other.count = self.count
        other.problems = self.problems
        other.states = self.states.clone()
        other.warm = self.warm.clone()
        other.commands = torch.zeros_like(self.commands)
        other.solution = None
        other.vel = torch.zeros_like(self.vel)
        return other

    def commands_host(self):
        return self.commands.cpu().numpy().view(abi.COMMAND_DTYPE).reshape(self.count)

    def velocities(self):
        """(count, 3) float64 view of the (vx, vy, omega) outputs on the device."""
        import torch
        return self.commands.view(torch.float64).view(self.count, 6)[:, :3]

    def states_host(self):
        return self.states.cpu().numpy().view(abi.STATE_DTYPE).reshape(self.count)
