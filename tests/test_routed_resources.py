"""Registers, scratch and occupancy of every K1 variant the dispatch tables (csrc/neo_mpc_kernels.hip launch_solve,
csrc/neo_mpc_riccati.hip launch_solve_riccati) can pick at four waves per SIMD, from the compiler's own resource remarks: the
two compile lines of `make resource-usage`, the Makefile's flags, no GPU.  The routed stage-wise iteration keeps its operands
in registers where it can, and every such change is one spilled register away from scratch traffic in each iteration of
each instance -- or from a lost wave per SIMD.  tests/test_abi.py::test_baseline_kernels_are_scratch_free holds the two
BASELINE kernels; this holds the rest of the four-wave rows.

The rule: occupancy 4 (or more), no spilled vector register, no scratch for the tame kernels; the two general stage-wise
kernels (k_solve_routed<4, false, 0>, k_solve<4, 0, 2, false, 0>) at most 12 bytes.

The dense-direction kernels of neo_mpc_kernels.hip that carry scratch since before this rule was written -- launch_solve's
comment says why the general control_steps-3 one is still launched at four waves; the run-time-sized two are four-wave only
under a tuning override -- are held to what they had then: none of them may gain scratch."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests.c_probe import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#: template arguments behind the wave count (as the mangled names spell them) -> bytes of scratch allowed
TAME_ROUTED = {"k_solve_routedILi4ELb1ELi1024E": 0, "k_solve_routedILi4ELb1ELi0E": 0}
GENERAL_STAGEWISE = {"k_solve_routedILi4ELb0ELi0E": 12, "7k_solveILi4ELi0ELi2ELb0ELi0E": 12}
TAME_STAGEWISE = {"7k_solveILi4ELi0ELi2ELb1ELi0E": 0}
TAME_DENSE_AND_LBFGS = {"7k_solveILi4ELi3ELi1ELb1ELi1024E": 0, "7k_solveILi4ELi3ELi1ELb1ELi0E": 0, "7k_solveILi4ELi3ELi0ELb0ELi0E": 0,
                        "7k_solveILi4ELi0ELi0ELb1ELi0E": 0, "7k_solveILi4ELi0ELi0ELb0ELi0E": 0}
#: (scratch they carried when this test was written; a vector spill is what that scratch is)
DENSE_WITH_SCRATCH = {"7k_solveILi4ELi3ELi1ELb0ELi0E": 68, "7k_solveILi4ELi0ELi1ELb1ELi0E": 108, "7k_solveILi4ELi0ELi1ELb0ELi0E": 268}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    mk = open(os.path.join(ROOT, "neo_mpc_planner2_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^RICCATI_FLAGS := (.*)$", mk, re.M).group(1).split()
    lines = re.findall(r"^\t\$\(HIPCC\).*-Rpass-analysis=kernel-resource-usage -x hip -c (\S+) -o /dev/null$", mk, re.M)
    assert lines == ["neo_mpc_kernels.hip", "neo_mpc_riccati.hip"], lines
    with ThreadPoolExecutor(2) as pool:    # (the two units side by side: one compile's time)
        jobs = [pool.submit(kernel_resources, tmp_path_factory.mktemp(unit.split(".")[0]), '#include "%s"\n' % unit,
                            flags if "riccati" in unit else ()) for unit in lines]
        return {"kernels": jobs[0].result(), "riccati": jobs[1].result()}


def _one(rows, key):
    hit = [v for k, v in rows.items() if key in k]
    assert len(hit) == 1, (key, sorted(rows))
    return hit[0]


@pytest.mark.parametrize("unit, table", [("riccati", TAME_ROUTED), ("riccati", TAME_STAGEWISE), ("riccati", GENERAL_STAGEWISE),
                                         ("kernels", TAME_DENSE_AND_LBFGS)],
                         ids=["routed-tame", "stagewise-tame", "stagewise-general", "dense-and-lbfgs"])
def test_four_wave_kernels_keep_their_waves_and_stay_out_of_scratch(remarks, unit, table):
    for key, scratch in table.items():
        r = _one(remarks[unit], key)
        print(key, {f: r.get(f) for f in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy")})
        assert r["Occupancy"] >= 4, (key, r)
        assert r["ScratchSize"] <= scratch, (key, r)
        if scratch == 0:
            assert r["VGPRs Spill"] == 0 and r["VGPRs"] <= 128, (key, r)


def test_dense_kernels_with_scratch_gain_none(remarks):
    for key, scratch in DENSE_WITH_SCRATCH.items():
        r = _one(remarks["kernels"], key)
        print(key, {f: r.get(f) for f in ("VGPRs", "VGPRs Spill", "ScratchSize", "Occupancy")})
        assert r["Occupancy"] >= 4 and r["ScratchSize"] <= scratch, (key, r)


def test_every_four_wave_variant_is_listed(remarks):
    """A four-wave instantiation the tables above do not name would go unchecked."""
    named = {**TAME_ROUTED, **GENERAL_STAGEWISE, **TAME_STAGEWISE, **TAME_DENSE_AND_LBFGS, **DENSE_WITH_SCRATCH}
    for unit in ("kernels", "riccati"):
        for fn in remarks[unit]:
            if re.search(r"k_solve(_routed)?ILi4E", fn):
                assert any(key in fn for key in named), fn
