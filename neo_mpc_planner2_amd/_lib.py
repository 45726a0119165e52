"""ctypes binding of the C-ABI library `libneo_mpc.so` (include/neo_mpc.h).

The library is built in-tree by `__graft_entry__.build()` /
`make -C neo_mpc_planner2_amd/csrc`.  There is no Python or CPU fallback: when the
shared object is missing, `load()` raises.
"""
import ctypes as C
import os

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
#: NEO_MPC_LIB selects another build of the same library (development A/B runs inside one gpurun
#: call: box-to-box variance is ~5 %, so two builds are only comparable on the same box)
LIB_PATH = os.environ.get("NEO_MPC_LIB") or os.path.join(HERE, "libneo_mpc.so")

_P = C.POINTER
_H = _V = C.c_void_p     # the handle; any other address: an array, a stream, an event
_U32, _F64, _SIZE = C.c_uint32, C.c_double, C.c_size_t
_COSTMAP = [_H, _V, _U32, _U32, _F64, _F64, _F64]
_CELLS = [_H, _U32, _U32, _V, _V]


def _pair(name, *args):
    """The prototypes of a step's host entry point and of its `_device` twin, which takes a stream behind the same arguments."""
    return {name: (C.c_int, [_H, *args]), name + "_device": (C.c_int, [_H, *args, _V])}


#: every symbol include/neo_mpc.h declares -> (restype, argtypes), or None where this package declares no prototype
PROTOTYPES = {
    "neo_mpc_abi_version": (C.c_int, None),
    "neo_mpc_behaviour_version": (C.c_int, None),
    "neo_mpc_effective_method": (C.c_int, [_H]),
    "neo_mpc_balance_dispatch_device": (C.c_int, [_H, _V, _SIZE, _V]),
    "neo_mpc_get_dispatch_order": (C.c_int, [_H, _V, _V, _P(_SIZE)]),
    "neo_mpc_last_error": (C.c_char_p, None),
    "neo_mpc_last_error_code": None,
    "neo_mpc_default_params": (C.c_int, [_P(abi.NeoMpcParams)]),
    "neo_mpc_create": (C.c_void_p, [_P(abi.NeoMpcParams), C.c_int]),
    "neo_mpc_destroy": (None, [_H]),
    "neo_mpc_set_params": (C.c_int, [_H, _P(abi.NeoMpcParams)]),
    "neo_mpc_get_params": (C.c_int, [_H, _P(abi.NeoMpcParams)]),
    "neo_mpc_set_costmap": (C.c_int, _COSTMAP),
    "neo_mpc_set_costmap_device": (C.c_int, _COSTMAP + [_V]),
    "neo_mpc_set_costmap_pool": (C.c_int, [_H, _V, _U32, _U32, _U32, _F64, _V]),
    "neo_mpc_set_costmap_pool_device": (C.c_int, [_H, _V, _U32, _U32, _U32, _F64, _V, _V]),
    **_pair("neo_mpc_solve_batch", _P(abi.NeoMpcBatch)),
    "neo_mpc_solve_batch_device_timed": (C.c_int, [_H, _P(abi.NeoMpcBatch), _V, _V, _V]),
    "neo_mpc_solve_batch_begin": (C.c_int, [_H, _P(abi.NeoMpcBatch), _P(_U32)]),
    "neo_mpc_solve_batch_wait": (C.c_int, [_H, _U32]),
    "neo_mpc_postprocess_batch": (C.c_int, [_H, _P(abi.NeoMpcBatch), _V]),
    "neo_mpc_objective_batch": (C.c_int, [_H, _V, _V, _V, _SIZE]),
    "neo_mpc_gradient_batch": (C.c_int, [_H, _V, _V, _V, _SIZE]),
    "neo_mpc_direction_batch": (C.c_int, [_H, _V, _V, _V, _SIZE, C.c_int]),
    "neo_mpc_kernel_info": (C.c_int, [_H, _P(_U32), _P(_U32), _P(_U32)]),
    "neo_mpc_pin_host_memory": (C.c_int, [_V, _SIZE]),
    "neo_mpc_unpin_host_memory": (C.c_int, [_V]),
    "neo_mpc_set_host_path": (C.c_int, [_H, C.c_int]),
    **_pair("neo_mpc_select_carrots", _P(abi.NeoMpcLookaheadParams), _P(abi.NeoMpcPlanBatch)),
    **_pair("neo_mpc_footprint_gate", _P(abi.NeoMpcFootprintBatch)),
    "neo_mpc_set_world_map": (C.c_int, _COSTMAP),
    "neo_mpc_set_world_map_device": (C.c_int, _COSTMAP + [_V]),
    **_pair("neo_mpc_roll_costmap_pool", _P(abi.NeoMpcWindowBatch)),
    "neo_mpc_get_costmap_pool": (C.c_int, _CELLS),
    **_pair("neo_mpc_stamp_fleet", _P(abi.NeoMpcStampBatch)),
    "neo_mpc_inflation_costs": (C.c_int, [_F64, _F64, _F64, _F64, _V, _SIZE, _P(_U32)]),
    **_pair("neo_mpc_inflate_world_map", _F64, _F64, _F64),
    "neo_mpc_get_world_map": (C.c_int, [_H, _V, _P(_U32), _P(_U32), _P(_F64), _P(_F64), _P(_F64)]),
    **_pair("neo_mpc_update_scan_layer", _P(abi.NeoMpcScanBatch)),
    "neo_mpc_get_scan_layer": (C.c_int, _CELLS),
    "neo_mpc_reset_scan_layer": (C.c_int, [_H]),
    "neo_mpc_laser_beam_table": (C.c_int, [_P(abi.NeoMpcScanner), _U32, _V]),
    **_pair("neo_mpc_project_laser", _P(abi.NeoMpcLaserBatch)),
    **_pair("neo_mpc_update_scan_layer_from_ranges", _P(abi.NeoMpcLaserBatch)),
    **_pair("neo_mpc_update_world_scan_layer", _P(abi.NeoMpcScanBatch), _P(abi.NeoMpcFleetClear)),
    **_pair("neo_mpc_update_world_scan_layer_from_ranges", _P(abi.NeoMpcLaserBatch), _P(abi.NeoMpcFleetClear)),
    "neo_mpc_get_world_scan_layer": (C.c_int, [_H, _V, _V]),
    "neo_mpc_reset_world_scan_layer": (C.c_int, [_H]),
    "neo_mpc_set_world_scan_denoise": (C.c_int, [_H, _U32, _U32]),
    "neo_mpc_get_world_scan_denoised": (C.c_int, [_H, _V]),
    "neo_mpc_set_world_scan_decay": (C.c_int, [_H, _U32]),
    "neo_mpc_get_world_scan_ages": (C.c_int, [_H, _V]),
    **_pair("neo_mpc_check_plans", _P(abi.NeoMpcPlanCheckBatch)),
    **_pair("neo_mpc_replan_plans", _P(abi.NeoMpcReplanBatch)),
    "neo_mpc_rccl_available": None, "neo_mpc_comm_init_all": None, "neo_mpc_comm_destroy": None,
    "neo_mpc_group_start": None, "neo_mpc_group_end": None,
    "neo_mpc_allgather_velocities": None, "neo_mpc_broadcast_costmap": None,
}
EXPORTS = tuple(PROTOTYPES)

_lib = None


class NeoMpcError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("neo_mpc error %d: %s" % (code, message))
        self.code = code


def load():
    """Load libneo_mpc.so and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C neo_mpc_planner2_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
    # PyTorch wheels bundle their own HIP runtime; if torch is going to be used in this process
    # (device memory / streams / torch.distributed plumbing) it must initialise that runtime
    # BEFORE another copy is mapped, otherwise torch reports "No HIP GPUs are available".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    # development A/B against an older build of the same library (NEO_MPC_LIB, tools/ab_many.sh): the record layouts have not
    # changed since ABI 1, so only the entry points a tool actually calls have to exist.  Otherwise a missing symbol is an
    # AttributeError here: the .so is older than include/neo_mpc.h
    older = bool(os.environ.get("NEO_MPC_LIB"))
    for name, prototype in PROTOTYPES.items():
        if older and not hasattr(lib, name):
            continue
        entry = getattr(lib, name)
        if prototype is not None:
            entry.restype = prototype[0]
            if prototype[1] is not None:
                entry.argtypes = prototype[1]
    version = lib.neo_mpc_abi_version()
    if older and version not in (1, abi.ABI_VERSION):
        raise ImportError("%s: ABI version %d" % (LIB_PATH, version))
    if not older and version != abi.ABI_VERSION:
        raise ImportError("libneo_mpc.so ABI version %d, this package binds %d" % (version, abi.ABI_VERSION))
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise NeoMpcError(code, (load().neo_mpc_last_error() or b"").decode())
