// Microbenchmark: the ISSUE cost of the control bookkeeping in the two-CU unroll's step loop -- SALU, s_nop, s_waitcnt
// with nothing outstanding, taken s_branch, and a whole divergent region (s_and_saveexec_b64 + s_cbranch_execz (not
// taken) + one VALU + s_or_b64 exec) -- on ONE wave per SIMD, as the shipped kernel runs, next to v_cndmask_b32 (what a
// guard becomes as a select).  The companion of valu_issue_cost.hip: both time 64 instructions per trip with s_memtime.
// Build: hipcc -O3 --offload-arch=gfx950 scripts/microbench/salu_branch_issue_cost.hip -o build/salu_branch_issue_cost
#include <hip/hip_runtime.h>
#include <cstdio>

template <int KIND>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k(float* out, long long* cyc, int iters) {
  float r[16];
  for (int i = 0; i < 16; ++i) r[i] = 0.001f * (threadIdx.x + i);
  unsigned su[8];
  for (int i = 0; i < 8; ++i) su[i] = __builtin_amdgcn_readfirstlane(threadIdx.x + i);
  const unsigned long long half_mask = 0x00000000ffffffffull;     // a divergent region that half the lanes enter
  const long long t0 = __builtin_amdgcn_s_memtime();
#pragma nounroll
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int rnd = 0; rnd < 4; ++rnd) {
      if (KIND == 0) {             // 16 independent SALU adds
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("s_add_u32 %0, %0, 1" : "+s"(su[i & 7]) : : "scc");
      } else if (KIND == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("s_nop 0");
      } else if (KIND == 2) {
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)");
      } else if (KIND == 3) {      // taken branches to the next instruction
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("s_branch 1f\n1:");
      } else if (KIND == 4) {      // 4 divergent regions of 4 instructions each = 16 instructions
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned long long saved;
          asm volatile("s_and_saveexec_b64 %0, %2\n\ts_cbranch_execz 1f\n\tv_add_f32 %1, %1, %1\n1:\n\ts_or_b64 exec, exec, %0"
                       : "=&s"(saved), "+v"(r[i]) : "s"(half_mask) : "scc");
        }
      } else if (KIND == 5) {      // 16 independent selects (the guard as a v_cndmask_b32)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          asm volatile("v_cndmask_b32 %0, %0, %1, %2" : "+v"(r[i]) : "v"(r[(i + 1) & 15]), "s"(half_mask));
      } else {                     // 6: VALU and SALU alternating (per pair /2): does the SALU issue under the VALU?
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(r[i]) : "v"(r[i + 1]));
          asm volatile("s_add_u32 %0, %0, 1" : "+s"(su[i & 7]) : : "scc");
        }
      }
    }
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0;
  for (int i = 0; i < 16; ++i) s += r[i];
  for (int i = 0; i < 8; ++i) s += (float)su[i];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

template <int KIND>
void run(const char* name, float* out, long long* cyc, int per_trip) {
  const int iters = 2000;
  hipLaunchKernelGGL(k<KIND>, dim3(256), dim3(256), 0, 0, out, cyc, iters);
  hipLaunchKernelGGL(k<KIND>, dim3(256), dim3(256), 0, 0, out, cyc, iters);
  (void)hipDeviceSynchronize();
  long long cy; (void)hipMemcpy(&cy, cyc, 8, hipMemcpyDeviceToHost);
  printf("%-52s %6.2f cycles per %s\n", name, (double)cy / iters / per_trip, per_trip == 16 ? "region" : "instruction");
}

int main() {
  float* out; long long* cyc;
  (void)hipMalloc(&out, 256 * 256 * 4); (void)hipMalloc(&cyc, 8);
  run<0>("s_add_u32", out, cyc, 64);
  run<1>("s_nop 0", out, cyc, 64);
  run<2>("s_waitcnt (nothing outstanding)", out, cyc, 64);
  run<3>("s_branch (taken, to the next instruction)", out, cyc, 64);
  run<4>("saveexec + cbranch_execz + 1 VALU + s_or_b64 exec", out, cyc, 16);
  run<5>("v_cndmask_b32", out, cyc, 64);
  run<6>("v_fma_f32 + s_add_u32 alternating (per pair /2)", out, cyc, 64);
  return 0;
}
