"""The grid planner (K16) without a GPU: the plain-Python transcription of its contract (tests/grid_planner_reference.py, the
executable form of neo_mpc_replan_batch in include/neo_mpc.h) against records, cell lists and poses written out by hand
(tests/grid_planner_cases.py) and against the properties the contract states -- G satisfies its Bellman equation at every
reached cell, a path's step costs sum to its record's cost; the record layout and the entry points against the header; the
compiler's resource remarks for the kernel.  Every comparison is an exact equality."""
import numpy as np

from neo_mpc_planner2_amd import abi
from tests import grid_planner_cases as cases
from tests import grid_planner_reference as ref
from tests.c_probe import check_entry_points, check_layout, kernel_resources, probe_header


def test_the_yaw_table_is_the_multiples_of_a_quarter_pi():
    for k in range(8):
        assert ref.YAW[k] == (k if k <= 4 else k - 8) * np.pi / 4 == (k if k <= 4 else k - 8) * ref.YAW[1], k


def test_transcription_on_hand_worked_maps():
    for case in cases.HAND_CASES:
        name, cells, starts, goals, kw, want, path, poses = cases.hand_inputs(case)
        stride = kw.get("max_path_cells", kw["window"] ** 2)
        got, got_cells, got_poses = ref.replan_plans(cells, 1.0, 0.0, 0.0, starts, goals, **kw)
        assert got.tolist() == want.tolist(), name
        assert got_cells.shape == (1, stride, 2) and got_poses.shape == (1, stride, 3), name
        assert got_cells[0, :len(path)].tolist() == [list(c) for c in path], name
        assert got_poses[0, :len(path)].tolist() == [list(p) for p in poses], name
        assert not got_cells[0, len(path):].any() and not got_poses[0, len(path):].any(), name       # nothing beyond the path
        assert len(path) == (min(int(want["length"][0]), stride) if want["status"][0] in (0, 5) else 0), name


def test_poses_on_a_map_with_a_resolution_and_an_origin():
    """The straight run on 5 cm cells from (-1.3, 2.7): each coordinate one rounded multiply and one rounded add."""
    name, cells, starts, goals, kw, want, path, _ = cases.hand_inputs(cases.HAND_CASES[0])
    res, ox, oy = 0.05, -1.3, 2.7
    got, got_cells, got_poses = ref.replan_plans(cells, res, ox, oy, starts * res + (ox, oy), goals * res + (ox, oy), **kw)
    assert got.tolist() == want.tolist() and got_cells[0, :6].tolist() == [list(c) for c in path]
    assert got_poses[0, :6].tolist() == [[-1.3 + (mx + 0.5) * 0.05, 2.7 + (my + 0.5) * 0.05, 0.0] for mx, my in path]


def test_checks_are_a_mask():
    """A robot whose check is not 1 is not asked: status 4, nothing written, whatever its start and goal."""
    name, cells, starts, goals, kw, want, path, _ = cases.hand_inputs(cases.HAND_CASES[0])
    checks = np.zeros(4, dtype=abi.PLAN_CHECK_DTYPE)
    checks["status"] = (1, 0, 2, 1)
    fill_cells = np.full((4, 64, 2), -7, dtype=np.int32)
    fill_poses = np.full((4, 64, 3), -7.0)
    got, got_cells, got_poses = ref.replan_plans(cells, 1.0, 0.0, 0.0, np.repeat(starts, 4, 0), np.repeat(goals, 4, 0),
                                                 checks=checks, path_cells=fill_cells, path_poses=fill_poses, **kw)
    assert got.tolist() == [want[0].tolist(), ref.record(4), ref.record(4), want[0].tolist()]
    for i in (0, 3):
        assert got_cells[i, :6].tolist() == [list(c) for c in path] and (got_cells[i, 6:] == -7).all()
        assert (got_poses[i, :6, 2] == 0.0).all() and (got_poses[i, 6:] == -7.0).all()
    assert (got_cells[1:3] == -7).all() and (got_poses[1:3] == -7.0).all()


def test_the_potential_satisfies_its_bellman_equation_and_paths_sum_to_their_cost():
    """Random maps, lethal and unknown cells among them, unknown both a wall and a cost: at every cell with a G other than the
    goal, G is the minimum over the allowed moves of step + G(target); G(goal) is 0; no cell without a G has a move to one
    with a G (unless no move may leave it); along every path the step costs sum to the record's cost."""
    found = 0
    for seed, unknown_cost in ((1, 0), (2, 20), (3, 0)):
        cells = cases.random_map(40, 33, seed)
        starts, goals = cases.random_pairs(cells, 1.0, 0.0, 0.0, 24, 16, seed + 100)
        for start, goal in zip(starts, goals):
            r, path, q = ref.replan_one(cells, 1.0, 0.0, 0.0, start, goal, 16, 253, unknown_cost, 50, 256)
            if r[0] in (1, 2, 3) or len(path) == 1:
                continue
            G = q.potential()
            assert G[q.g] == 0
            for y in range(q.y0, min(q.y0 + 16, 33)):
                for x in range(q.x0, min(q.x0 + 16, 40)):
                    a = (x, y)
                    if a == q.g or not q.leaves(a):
                        assert a == q.g or a not in G
                        continue
                    reach = [q.step(a, k) + G[(x + ref.MOVES[k][0], y + ref.MOVES[k][1])] for k in range(8)
                             if q.allowed(a, k) and (x + ref.MOVES[k][0], y + ref.MOVES[k][1]) in G
                             and q.traversable((x + ref.MOVES[k][0], y + ref.MOVES[k][1]))]
                    assert (G[a] == min(reach)) if reach else (a not in G), (seed, a)
            assert r[0] == 0 and path[0] == q.s and path[-1] == q.g and r[1] == len(path) and r[2] == G[q.s]
            total = 0
            for a, b in zip(path[:-1], path[1:]):
                k = ref.MOVES.index((b[0] - a[0], b[1] - a[1]))
                assert q.allowed(a, k)
                total += q.step(a, k)
            assert total == r[2] < 2 ** 32
            found += 1
    assert found >= 30, found


def test_at_least_half_of_every_random_fleet_finds_a_path():
    """The condition the GPU tests put on their inputs (fixed seeds, no robot dropped); found, no path and a goal that is not
    traversable all occur among them."""
    seen = set()
    for name in cases.FLEETS:
        got = cases.random_fleet(name)[-1][0]
        print(name, np.bincount(got["status"], minlength=6).tolist())
        assert 2 * (got["status"] == 0).sum() >= len(got), name
        seen |= set(got["status"].tolist())
    assert {0, 1, 2} <= seen, seen          # (3, 4 and 5 are among the hand-worked cases)


def test_the_serpentine_is_the_longest_search():
    cells, start, goal, kw = cases.serpentine()
    got, got_cells, _ = ref.replan_plans(cells, 1.0, 0.0, 0.0, start, goal, **kw)
    assert got.tolist() == [ref.record(0, 7627, 3813000, 0, 6)]
    assert got_cells[0, 0].tolist() == [10, 8] and got_cells[0, 7626].tolist() == [10, 132]


def test_replan_layout_and_entry_points(tmp_path):
    entry_points = ("neo_mpc_replan_plans", "neo_mpc_replan_plans_device")
    got = probe_header(tmp_path, ["neo_mpc_replan_batch", "neo_mpc_replan"], entry_points=entry_points)
    check_layout(got, "neo_mpc_replan_batch", 80, struct=abi.NeoMpcReplanBatch)
    check_layout(got, "neo_mpc_replan", 24, struct=abi.NeoMpcReplan, dtype=abi.REPLAN_DTYPE)
    assert abi.REPLAN_DTYPE.names == ("status", "length", "cost", "window_x0", "window_y0", "reserved")
    check_entry_points(entry_points)


def test_the_planner_kernel_is_scratch_free_and_fits_the_lds(tmp_path):
    """k_replan for windows of up to 32, 64 and 128 cells: no scratch, and static LDS a single workgroup may hold on gfx950
    (160 KiB a CU).  The compiler's own resource remarks, with the flags of the Makefile; no GPU needed."""
    rows = kernel_resources(tmp_path, '#include "grid_planner.h"\n'
                            'template <int W> void launch(const neo_mpc::ReplanArgs& a) {\n'
                            '  hipLaunchKernelGGL(neo_mpc::k_replan<W>, dim3(1), dim3(256), 0, nullptr, a);\n}\n'
                            'template void launch<32>(const neo_mpc::ReplanArgs&);\n'
                            'template void launch<64>(const neo_mpc::ReplanArgs&);\n'
                            'template void launch<128>(const neo_mpc::ReplanArgs&);\n')
    mine = {name: row for name, row in rows.items() if "k_replan" in name}
    assert len(mine) == 3, sorted(rows)
    for name, row in mine.items():
        print(name, row)
        assert row["ScratchSize"] == 0 and row["VGPRs Spill"] == 0 and row["SGPRs Spill"] == 0, (name, row)
        assert 0 < row["LDS Size"] <= 163840, (name, row)
    # the window picks the kernel and with it how many searches share a CU: 8 KiB, 32 KiB and the whole budget
    assert all(got <= most for got, most in zip(sorted(r["LDS Size"] for r in mine.values()), (8192, 32768, 163840)))
