"""The compile-time table of the 64 candidate step multipliers (csrc/lane_scale_table.h) against a NumPy restatement of the
rule lane_scale (csrc/feasible_set.h) computes on the device.  No GPU: the header is plain C++, a stand-alone host program
prints its entries as hex words, and a float64 multiply is IEEE on both sides -- the comparison is exact."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neo_mpc_planner2_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "lane_scale_table.h"
template <bool kLongShots> static void dump(const char* name) {
  static constexpr neo_mpc::LaneScaleTable t = neo_mpc::make_lane_scale_table<kLongShots>();
  for (int l = 0; l < 64; ++l) {
    uint64_t w;
    std::memcpy(&w, &t.v[l], 8);
    std::printf("%s %d %016llx\n", name, l, (unsigned long long)w);
  }
}
int main() {
  dump<true>("long");
  dump<false>("plain");
  return 0;
}
"""


def qn_steps():
    """NEO_QN_STEPS as the header spells it: the decimal literals, parsed by Python as the compiler parses them (both round
    a decimal literal to the nearest float64)."""
    text = open(os.path.join(CSRC, "lane_scale_table.h")).read()
    body = re.search(r"#define NEO_QN_STEPS(.*?)\n\n", text, re.S).group(1).replace("\\", " ")
    steps = [float(x) for x in body.replace(",", " ").split()]
    assert len(steps) == 32
    return np.array(steps, dtype=np.float64)


def expected(long_shots):
    """lanes 0-31: 2^(-12 + lane // 2), times the sqrt(2) literal on odd lanes; lanes 32-63: the step lengths; with long
    shots lanes 61-63 are 8, 16, 32."""
    lanes = np.arange(32)
    prox = np.ldexp(np.float64(1.0), -12 + lanes // 2)
    prox = np.where(lanes % 2 == 1, prox * np.float64(1.4142135623730951), prox)
    t = np.concatenate([prox, qn_steps()])
    if long_shots:
        t[61:64] = [8.0, 16.0, 32.0]
    return t


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_scale_table")
    (d / "table.cpp").write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(d / "table.cpp"), "-o", str(d / "table")])
    got = {"long": np.zeros(64, dtype=np.uint64), "plain": np.zeros(64, dtype=np.uint64)}
    for line in subprocess.check_output([str(d / "table")]).decode().splitlines():
        name, lane, word = line.split()
        got[name][int(lane)] = int(word, 16)
    return got


@pytest.mark.parametrize("name,long_shots", [("long", True), ("plain", False)])
def test_table_is_the_rule_bit_for_bit(tables, name, long_shots):
    want = expected(long_shots).view(np.uint64)
    bad = np.flatnonzero(tables[name] != want)
    assert bad.size == 0, [(int(l), hex(int(tables[name][l])), hex(int(want[l]))) for l in bad]


def test_the_tables_differ_in_the_long_shots_only(tables):
    assert np.flatnonzero(tables["long"] != tables["plain"]).tolist() == [61, 62, 63]
    assert tables["long"][61:64].view(np.float64).tolist() == [8.0, 16.0, 32.0]
