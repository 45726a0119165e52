// What a wave alone on its SIMD pays for where a constant comes from, gfx950 (study; one 64-lane workgroup per SIMD):
//   a dependent chain of twelve three-address v_fma_f64 whose addends are
//     (a) literals rebuilt by two s_mov_b32 in front of every fma (what -disable-machine-licm leaves in the solver loop),
//     (b) held in scalar register pairs filled before the clock starts,
//     (c) fetched by one s_load_dwordx16 + one s_load_dwordx4 in front of every twelve;
//   and one LDS read + wait + the same chain
//     (d) alone,  (e) with a second, lane-indexed ds_read_b64 issued next to it (one wait for both),
//     (f) with a lane-indexed global_load_dwordx2 from a warm 256-byte table and its s_waitcnt vmcnt(0).
//   hipcc --offload-arch=gfx950 -O2 -w -o /tmp/mb_constant_sources tools/mb_constant_sources.hip && /tmp/mb_constant_sources
// Prints shader clocks (clock64) per body of twelve fmas: minimum and median over the waves.
// (results: profiles/r20_constant_sources.txt)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdio.h>
#include <vector>

__device__ double g_table[32];   // the scalar loads' and the vector load's source (filled by the host)

// twelve steps r = z * r + c_k; the literals are those of fast_math.h's sincos kernels (ten) and two more
#define LIT_FMA(lo, hi) "s_mov_b32 s40, " #lo "\n s_mov_b32 s41, " #hi "\n v_fma_f64 %0, %1, %0, s[40:41]\n"
#define TWELVE_LITERAL                                                                                                     \
  LIT_FMA(0x57b1fe7d, 0x3ec71de3) LIT_FMA(0x8a2b9ceb, 0xbe927e4f) LIT_FMA(0x19c161d5, 0xbf2a01a0) LIT_FMA(0x19cb1590, 0x3efa01a0) \
  LIT_FMA(0x1110f8a6, 0x3f811111) LIT_FMA(0x16c15177, 0xbf56c16c) LIT_FMA(0x55555549, 0xbfc55555) LIT_FMA(0x5555554c, 0x3fa55555) \
  LIT_FMA(0x5acfd57c, 0xbe5ae5e6) LIT_FMA(0xbdb4b1c4, 0x3e21ee9e) LIT_FMA(0x00000000, 0x3fe00000) LIT_FMA(0x00000000, 0x3ff00000)
#define HELD_FMA(k) "v_fma_f64 %0, %1, %0, %" #k "\n"
#define TWELVE_HELD HELD_FMA(2) HELD_FMA(3) HELD_FMA(4) HELD_FMA(5) HELD_FMA(6) HELD_FMA(7) HELD_FMA(8) HELD_FMA(9) HELD_FMA(10) HELD_FMA(11) HELD_FMA(12) HELD_FMA(13)
#define FETCHED_FMA(lo, hi) "v_fma_f64 %0, %1, %0, s[" #lo ":" #hi "]\n"
#define TWELVE_FETCHED                                                                                            \
  FETCHED_FMA(40, 41) FETCHED_FMA(42, 43) FETCHED_FMA(44, 45) FETCHED_FMA(46, 47) FETCHED_FMA(48, 49) FETCHED_FMA(50, 51) \
  FETCHED_FMA(52, 53) FETCHED_FMA(54, 55) FETCHED_FMA(56, 57) FETCHED_FMA(58, 59) FETCHED_FMA(40, 41) FETCHED_FMA(42, 43)
#define FETCHED_CLOBBERS "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59"

constexpr int kBodies = 4;   // bodies per pass of the timed loop

template <int MODE>
__global__ __launch_bounds__(64) void k(long long* clocks, double* sink, int passes) {
  __shared__ double lds[128];
  const int lane = threadIdx.x;
  lds[lane] = 1.0 + lane;
  lds[64 + lane] = 0.25;
  __syncthreads();
  double r = 0.5 + lane * 1e-3, z = 0.25;
  double c[12];
  for (int i = 0; i < 12; ++i) c[i] = g_table[i];
  const double* tab = g_table;
  asm volatile("" : "+s"(tab));
  const unsigned lds_u = (unsigned)(size_t)(&lds[64]), lds_l = (unsigned)(size_t)(&lds[lane]);
  const double* vaddr = g_table + (lane & 31);
  double warm = *vaddr;   // (the table is in the cache before the clock starts)
  asm volatile("" : "+v"(warm));
  long long t0 = clock64();
  for (int p = 0; p < passes; ++p) {
#pragma unroll
    for (int b = 0; b < kBodies; ++b) {
      if (MODE == 0) {
        asm volatile(TWELVE_LITERAL : "+v"(r) : "v"(z) : "s40", "s41");
      } else if (MODE == 1) {
        asm volatile(TWELVE_HELD : "+v"(r) : "v"(z), "s"(c[0]), "s"(c[1]), "s"(c[2]), "s"(c[3]), "s"(c[4]), "s"(c[5]), "s"(c[6]), "s"(c[7]),
                     "s"(c[8]), "s"(c[9]), "s"(c[10]), "s"(c[11]));
      } else if (MODE == 2) {
        asm volatile("s_load_dwordx16 s[40:55], %2, 0x0\n s_load_dwordx4 s[56:59], %2, 0x40\n s_waitcnt lgkmcnt(0)\n" TWELVE_FETCHED
                     : "+v"(r) : "v"(z), "s"(tab) : FETCHED_CLOBBERS, "memory");
      } else if (MODE == 3) {
        double x;
        asm volatile("ds_read_b64 %2, %3\n s_waitcnt lgkmcnt(0)\n v_mul_f64 %0, %0, %2\n" TWELVE_LITERAL
                     : "+v"(r), "+v"(z), "=&v"(x) : "v"(lds_u) : "s40", "s41", "memory");
      } else if (MODE == 4) {
        double x, y;
        asm volatile("ds_read_b64 %2, %4\n ds_read_b64 %3, %5\n s_waitcnt lgkmcnt(0)\n v_mul_f64 %0, %0, %2\n v_mul_f64 %0, %0, %3\n" TWELVE_LITERAL
                     : "+v"(r), "+v"(z), "=&v"(x), "=&v"(y) : "v"(lds_u), "v"(lds_l) : "s40", "s41", "memory");
      } else if (MODE == 5) {
        double x, y;
        asm volatile("ds_read_b64 %2, %4\n global_load_dwordx2 %3, %5, off\n s_waitcnt vmcnt(0) lgkmcnt(0)\n v_mul_f64 %0, %0, %2\n v_mul_f64 %0, %0, %3\n" TWELVE_LITERAL
                     : "+v"(r), "+v"(z), "=&v"(x), "=&v"(y) : "v"(lds_u), "v"(vaddr) : "s40", "s41", "memory");
      }
    }
  }
  long long t1 = clock64();
  if (lane == 0) clocks[blockIdx.x] = t1 - t0;
  sink[blockIdx.x * 64 + lane] = r + z + warm;
}

template <int MODE>
double run(const char* name, long long* d_clocks, double* d_sink, int blocks) {
  const int passes = 2000;
  std::vector<long long> h(blocks);
  k<MODE><<<blocks, 64>>>(d_clocks, d_sink, 50);
  hipDeviceSynchronize();
  k<MODE><<<blocks, 64>>>(d_clocks, d_sink, passes);
  if (hipDeviceSynchronize() != hipSuccess) { printf("%s: launch failed\n", name); exit(2); }
  hipMemcpy(h.data(), d_clocks, blocks * sizeof(long long), hipMemcpyDeviceToHost);
  std::sort(h.begin(), h.end());
  const double per = 1.0 / ((double)passes * kBodies);
  printf("%-58s min %8.2f  median %8.2f  max %8.2f clocks per body\n", name, h[0] * per, h[blocks / 2] * per, h[blocks - 1] * per);
  return h[blocks / 2] * per;
}

int main() {
  hipDeviceProp_t prop;
  hipGetDeviceProperties(&prop, 0);
  const int blocks = prop.multiProcessorCount * 4;   // one wave per SIMD
  double table[32];
  for (int i = 0; i < 32; ++i) table[i] = 1.0 / (1.0 + i);
  hipMemcpyToSymbol(HIP_SYMBOL(g_table), table, sizeof(table));
  long long* d_clocks;
  double* d_sink;
  hipMalloc(&d_clocks, blocks * sizeof(long long));
  hipMalloc(&d_sink, blocks * 64 * sizeof(double));
  printf("%s, %d one-wave workgroups (one per SIMD); a body is twelve dependent v_fma_f64\n", prop.name, blocks);
  for (int rep = 0; rep < 3; ++rep) {
    printf("-- repeat %d\n", rep);
    const double a = run<0>("(a) two literal s_mov_b32 in front of each fma", d_clocks, d_sink, blocks);
    const double b = run<1>("(b) addends held in scalar pairs", d_clocks, d_sink, blocks);
    const double c = run<2>("(c) s_load_dwordx16 + s_load_dwordx4 + wait per body", d_clocks, d_sink, blocks);
    const double d = run<3>("(d) ds_read_b64 + wait + mul + (a)", d_clocks, d_sink, blocks);
    const double e = run<4>("(e) (d) + a lane-indexed ds_read_b64 under the same wait", d_clocks, d_sink, blocks);
    const double f = run<5>("(f) (d) + a lane-indexed global_load_dwordx2, vmcnt(0)", d_clocks, d_sink, blocks);
    printf("   per fma: (a) %.2f  (b) %.2f  (c) %.2f;  the second operand costs: from LDS %+.1f, from vector memory %+.1f clocks\n",
           a / 12, b / 12, c / 12, e - d, f - d);
  }
  hipFree(d_clocks);
  hipFree(d_sink);
  return 0;
}
