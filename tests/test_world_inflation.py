"""The world inflation (K9), the part that needs no GPU: nav2's inflation layer applied to the world map the rolling windows
are cut from -- set -> inflate -> roll.

nav2's layers cannot be built here, so the contract is the text in include/neo_mpc.h (neo_mpc_inflate_world_map) and its
executable form the transcription in tests/world_inflation_reference.py.  The contract is integers apart from the cost
table, so every comparison is exact equality of uint8 cells: no tolerance, no dropped case.  The maps and parameter sets of
`cases()` are what tests/test_world_inflation_gpu.py holds the library to."""
import ctypes as C
import functools
import re

import numpy as np

from neo_mpc_planner2_amd import _lib
from tests import world_inflation_reference as ref
from tests.c_probe import HEADER, kernel_resources, run_c_probe

ENTRY_POINTS = ("neo_mpc_inflate_world_map", "neo_mpc_inflate_world_map_device", "neo_mpc_get_world_map")
SIZES = ((13, 11), (70, 67), (130, 75))                 # size_x, size_y: below one tile, just over one, 3 x 2 tiles
DENSITIES = (0.002, 0.03)                               # seeds
UNKNOWN = 0.05
#: world resolution; inscribed_radius, inflation_radius, cost_scaling_factor -> R = 18, 12, 0 (nothing changes), 64 (larger
#: than every map)
PARAMETER_SETS = ((0.05, (0.45, 0.9, 3.0)), (0.025, (0.2, 0.3, 5.0)), (0.05, (0.3, 0.0, 1.0)), (0.05, (0.0, 3.2, 0.5)))
REACHES = (18, 12, 0, 64)


def random_map(rng, size_x, size_y, density):
    """Mostly free space, a fifth of the cells with some cost below 253, `density` seeds, 5 % unknown cells."""
    cells = np.where(rng.random((size_y, size_x)) < 0.2, rng.integers(1, 253, size=(size_y, size_x)), 0).astype(np.uint8)
    cells[rng.random((size_y, size_x)) < 0.01] = 253          # inscribed cells that are no seeds
    cells[rng.random((size_y, size_x)) < UNKNOWN] = 255
    cells[rng.random((size_y, size_x)) < density] = 254
    return cells


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, cells, resolution, (inscribed_radius, inflation_radius, cost_scaling_factor), inflated cells)]: the 24
    cases of test 2, the inflated cells by the fast transcription.  Made once, read-only."""
    rng = np.random.default_rng(97)
    out = []
    for size_x, size_y in SIZES:
        for density in DENSITIES:
            cells = random_map(rng, size_x, size_y, density)
            cells.setflags(write=False)
            for (res, params), reach in zip(PARAMETER_SETS, REACHES):
                table, got_reach = ref.table_for(res, *params)
                assert got_reach == reach
                want = ref.inflate(cells, table, reach)
                want.setflags(write=False)
                out.append(("%dx%d-%g-R%d" % (size_x, size_y, density, reach), cells, res, params, want))
    return tuple(out)


# ------------------------------------------------------------------------------------------ 1: the hand-worked map
HAND_IN = [[0, 0, 0, 0, 0, 0, 0, 0, 254], [0, 0, 0, 100, 0, 0, 0, 0, 0], [0, 0, 253, 0, 0, 0, 0, 0, 0], [0, 0, 0, 254, 0, 200, 0, 0, 0],
           [0, 0, 0, 255, 0, 0, 0, 0, 0], [0, 0, 0, 255, 0, 0, 0, 0, 0], [255, 0, 0, 0, 0, 0, 0, 0, 0]]
HAND_OUT = [[0, 0, 0, 0, 0, 0, 92, 253, 254], [0, 0, 0, 100, 0, 0, 0, 166, 253], [0, 0, 253, 253, 166, 0, 0, 0, 92],
            [0, 92, 253, 254, 253, 200, 0, 0, 0], [0, 0, 166, 253, 166, 0, 0, 0, 0], [0, 0, 0, 255, 0, 0, 0, 0, 0],
            [255, 0, 0, 0, 0, 0, 0, 0, 0]]


def test_transcription_on_a_hand_worked_map():
    """A corner seed; an unknown cell taking 253 and one refusing 92; the maximum keeping 100 and 200; a 253 that is no seed."""
    table, reach = ref.table_for(0.5, 0.5, 1.0, 2.0)
    assert reach == 2 and table.tolist() == [254, 253, 166, 121, 92]
    cells = np.array(HAND_IN, dtype=np.uint8)
    assert cells.shape == (7, 9)
    for form in (ref.inflate_by_definition, ref.inflate):
        out = form(cells, table, reach)
        assert out.tolist() == HAND_OUT, form.__name__
        assert form(out, table, reach).tolist() == HAND_OUT, form.__name__        # idempotent
    assert ref.inflate_world(cells, 0.5, 0.5, 1.0, 2.0).tolist() == HAND_OUT


# ------------------------------------------------------------------------------------------ 2: the two forms
def test_the_fast_transcription_equals_the_definition():
    changed = 0
    assert len(cases()) == 24
    for name, cells, res, params, fast in cases():
        table, reach = ref.table_for(res, *params)
        assert np.array_equal(fast, ref.inflate_by_definition(cells, table, reach)), name
        assert np.array_equal(fast == 254, cells == 254), name                     # the seed set is unchanged
        assert np.array_equal(ref.inflate(fast, table, reach), fast), name         # the second application is the identity
        assert np.array_equal(ref.inflate_by_definition(fast, table, reach), fast), name
        if reach == 0:
            assert np.array_equal(fast, cells), name
        changed += int((fast != cells).any())
    print("%d of %d cases change a cell" % (changed, len(cases())))
    assert changed >= 12


# ------------------------------------------------------------------------------------------ 3: the entry points
def test_entry_points_are_declared_and_exported(tmp_path):
    got = run_c_probe(tmp_path, '#include <stdio.h>\n#include "neo_mpc.h"\n'
                      'int main(void) {\n'
                      '  int (*host)(neo_mpc_handle*, double, double, double) = neo_mpc_inflate_world_map;\n'
                      '  int (*device)(neo_mpc_handle*, double, double, double, void*) = neo_mpc_inflate_world_map_device;\n'
                      '  int (*get)(neo_mpc_handle*, uint8_t*, uint32_t*, uint32_t*, double*, double*, double*) = neo_mpc_get_world_map;\n'
                      '  void* volatile f[3] = {(void*)host, (void*)device, (void*)get};\n'
                      '  printf("abi %d\\nbehaviour %d\\ncells %d\\n", NEO_MPC_ABI_VERSION, NEO_MPC_BEHAVIOUR_VERSION, NEO_MPC_MAX_INFLATION_CELLS);\n'
                      '  printf("null %d %d %d\\n", host(0, 0.45, 0.9, 3.0), device(0, 0.45, 0.9, 3.0, 0), get(0, 0, 0, 0, 0, 0, 0));\n'
                      '  return f[0] == 0 || f[1] == 0 || f[2] == 0;\n}\n', werror=("incompatible-pointer-types",))
    assert got["abi"] == "2" and got["behaviour"] == "6" and got["cells"] == "64"
    assert got["null"] == "-1 -1 -1"                                                # a null handle: NEO_MPC_ERR_INVALID_ARGUMENT
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert "#define NEO_MPC_ABI_VERSION 2" in text and "#define NEO_MPC_BEHAVIOUR_VERSION 6" in text


# ------------------------------------------------------------------------------------------ 4: refusals without a device
def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    assert lib.neo_mpc_inflate_world_map(None, 0.45, 0.9, 3.0) == -1 and lib.neo_mpc_last_error_code() == -1
    assert lib.neo_mpc_inflate_world_map_device(None, 0.45, 0.9, 3.0, None) == -1
    size = C.c_uint32(7)
    assert lib.neo_mpc_get_world_map(None, None, C.byref(size), None, None, None, None) == -1 and size.value == 7


# ------------------------------------------------------------------------------------------ the kernel's resources
def test_the_inflation_kernel_is_scratch_free(tmp_path):
    """k_inflate_world spills nothing: the compiler's own resource remarks for a translation unit that holds this kernel
    alone, with the flags of the Makefile; no GPU needed.  Held to the figures DESIGN.md states: 8 waves per SIMD and 8736
    bytes of LDS (masks 4608, table 4112, flags 16)."""
    rows = kernel_resources(tmp_path, '#include "world_inflation.h"\n'
                            'void launch(const neo_mpc::InflateArgs& a) {\n'
                            '  hipLaunchKernelGGL(neo_mpc::k_inflate_world, dim3(1, 1), dim3(256), 0, nullptr, a);\n}\n')
    hit = [v for k, v in rows.items() if "k_inflate_world" in k]
    assert len(hit) == 1, list(rows)
    print("k_inflate_world:", hit[0])
    assert hit[0]["ScratchSize"] == 0 and hit[0]["VGPRs Spill"] == 0 and hit[0]["SGPRs Spill"] == 0
    assert hit[0]["LDS Size"] <= 8736 and hit[0]["Occupancy"] >= 8
