// neo_mpc_riccati.hip -- the stage-wise (Riccati) variants of K1, k_solve<*, 0, 2, *>, and the routed control_steps-3
// kernel k_solve_routed (k1_solve.h), with their rows of the dispatch table.  Part of libneo_mpc.so.
//
// A unit of their own for flags of their own (Makefile, RICCATI_FLAGS).  -fno-slp-vectorize: the SLP vectoriser packs the
// sweep's float32 arithmetic into v_pk_* instructions and pays for it with three hundred register moves that assemble the
// operand pairs (859 vector instructions in the sweep against 757 without it) -- measured +7 % solves/s at control_steps 8
// and +9 % at 32 without; the dense-Newton kernels are 0.5 % faster WITH it.  The routed kernel is built without it too:
// with it its stage-wise branch spills 22 vector registers.  -mllvm -disable-machine-licm: the Makefile says what for.
#include "k1_solve.h"

namespace neo_mpc {

void launch_solve_riccati(const SolveArgs& a, const LaunchTuning& tuning, void* stream, void* ev_start, void* ev_stop) {
  if (a.count == 0) return;
  const K1Launch launch(a, tuning, stream, ev_start, ev_stop);   // (k1_solve.h: what both tables know before they pick a row)
  const bool disc = launch.disc, small_tile = launch.small_tile;
  const size_t lds = launch.lds;
  if (a.p.routed) {   // control_steps 3, AUTO: direction by neighbourhood (k_solve_routed; the dense layout, 4 waves/SIMD like the dense kernels)
    const int w = solve_variant(tuning, 4);
    if (disc && w == 4 && small_tile) launch(k_solve_routed<4, true, 1024>, 0);   // (the static variant takes no dynamic LDS)
    else if (disc) launch(NEO_K1_BY_WAVES(w, k_solve_routed, true), lds);
    else launch(NEO_K1_BY_WAVES(w, k_solve_routed, false), lds);
  } else {  // any control_steps: Newton direction by the Riccati sweep (riccati.h)
    // the 128-VGPR build (4 waves/SIMD) wherever LDS lets a CU hold more than 12 workgroups -- 13 need <= 12.3 KB
    // each -- else the 168-VGPR build (measured: control_steps 8, 16 workgroups/CU: +17 %; control_steps 32 at
    // 11.3 KB = 14 workgroups/CU: +9 %; with 12 workgroups/CU the 4-wave build's spills make it 4 % slower; the general
    // variant's 10 spilled VGPRs at 4 waves/SIMD cost nothing measurable: "turn" parameter set, 65 536 instances, same
    // box: 34.9 M solves/s against 30.6 M at 3 waves/SIMD, tools/ab_general.py)
    const int w = solve_variant(tuning, lds <= 12600 ? 4 : 3);
    if (disc) launch(NEO_K1_BY_WAVES(w, k_solve, 0, 2, true), lds);
    else launch(NEO_K1_BY_WAVES(w, k_solve, 0, 2), lds);
  }
}

}  // namespace neo_mpc
