// k1_timing.h -- the clock stamps of K1's study builds (`make timing`, `make segments`); empty macros in the product build.
// Included by k1_solve.h only: the macros expand inside solve_search and the kernels and name their locals.
#pragma once

// Study build (make timing -> libneo_mpc_timing.so): shader-clock stamps at the phase boundaries of
// solver iteration 2 in entries 0-5 of `solution` (tools/phase_timing.py); wall-clock start and end of
// the wave and its HW_ID in entries 6-8 (tools/wave_timeline.py; control_steps >= 3).
#ifdef NEO_MPC_PHASE_TIMING
// (-DNEO_MPC_SEGMENT_TIMING on top: wall-clock stamps at the first and behind the last solver iteration replace
// the phase clocks of entries 4-5 -- set-up, iterations and K2 of every wave, tools/wave_timeline.py)
#ifdef NEO_MPC_SEGMENT_TIMING
#define NEO_SEGMENT_DECL unsigned long long seg_t0 = 0, seg_t1 = 0, seg_scan = 0, seg_scan_at = 0
#define NEO_SEGMENT(k) seg_t##k = wall_clock64()
#define NEO_SEGMENT_SCAN_BEGIN() seg_scan_at = wall_clock64(); seg_scan = seg_scan_at
#define NEO_SEGMENT_SCAN_END() seg_scan = wall_clock64() - seg_scan
#define NEO_SEGMENT_DUMP()                                                                                   \
  {                                                                                                          \
    SolveArgs ad;                                                                                            \
    fresh_args<V>(ad);                                                                                       \
    const int nvd = 3 * ad.p.n;                                                                              \
    if (ad.solution && lane_again() == 0 && nvd >= 9) {                                                      \
      ad.solution[(size_t)b * nvd + 4] = (double)seg_t0; ad.solution[(size_t)b * nvd + 5] = (double)seg_t1;  \
      ad.solution[(size_t)b * nvd + 3] = (double)seg_scan; ad.solution[(size_t)b * nvd + 2] = (double)seg_scan_at; \
    }                                                                                                        \
  }
#else
#define NEO_SEGMENT_DECL
#define NEO_SEGMENT(k)
#define NEO_SEGMENT_SCAN_BEGIN()
#define NEO_SEGMENT_SCAN_END()
#define NEO_SEGMENT_DUMP()
#endif
#define NEO_WAVE_START const unsigned long long wave_t0 = wall_clock64()
#define NEO_WAVE_END_ARGS(args)                                                                     \
  if ((args).solution && lane == 0 && (args).p.n >= 3) {                                            \
    const int nvw = 3 * (args).p.n;                                                                \
    unsigned int hw_id, xcc_id;                                                                    \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));                            \
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));                          \
    (args).solution[(size_t)b * nvw + 6] = (double)wave_t0;                                        \
    (args).solution[(size_t)b * nvw + 7] = (double)wall_clock64();                                 \
    (args).solution[(size_t)b * nvw + 8] = (double)hw_id + 4294967296.0 * (double)(xcc_id & 15u);  \
  }
#define NEO_PHASE_DECL long long phase_clock[8]
#define NEO_PHASE(k) phase_clock[k] = clock64()
#define NEO_PHASE_DUMP()                                                                            \
  if (it == 2 && a.solution && lane == 0)                                                          \
    for (int k = 0; k < 6; ++k) a.solution[(size_t)b * nv + k] = (double)(phase_clock[k + 1] - phase_clock[k])
#else
#define NEO_WAVE_START
#define NEO_WAVE_END_ARGS(args)
#define NEO_SEGMENT_DECL
#define NEO_SEGMENT(k)
#define NEO_SEGMENT_SCAN_BEGIN()
#define NEO_SEGMENT_SCAN_END()
#define NEO_SEGMENT_DUMP()
#define NEO_PHASE_DECL
#define NEO_PHASE(k)
#define NEO_PHASE_DUMP()
#endif
