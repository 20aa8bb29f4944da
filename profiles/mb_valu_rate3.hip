// micro-benchmark: issue rate of the byte-packed estimator's VALU ops on gfx950 (v_dot4_u32_u8, v_and_or_b32,
// v_bcnt_u32_b32, v_sad_u8; v_add_u32, v_mad_i32_i24 and v_pk_mad_i16 as the yardsticks) at 4 and 8 waves per SIMD
// build: hipcc --offload-arch=gfx950 -O3 -o mb_valu_rate3 mb_valu_rate3.hip        output: profiles/mb_valu_rate3.txt
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
template <int KIND>
__global__ void __launch_bounds__(256) k(uint32_t *out, int iters, uint32_t seed)
{
    uint32_t a0 = threadIdx.x + seed, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, a6 = a0 * 17, a7 = a0 * 19;
    uint32_t s = seed | 1;
    for (int i = 0; i < iters; ++i) {
#define OP8(INS) asm volatile(INS : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(s));
        if (KIND == 0) { OP8("v_add_u32 %0, %0, %8\n v_add_u32 %1, %1, %8\n v_add_u32 %2, %2, %8\n v_add_u32 %3, %3, %8\n v_add_u32 %4, %4, %8\n v_add_u32 %5, %5, %8\n v_add_u32 %6, %6, %8\n v_add_u32 %7, %7, %8") }
        if (KIND == 1) { OP8("v_dot4_u32_u8 %0, %8, %8, %0\n v_dot4_u32_u8 %1, %8, %8, %1\n v_dot4_u32_u8 %2, %8, %8, %2\n v_dot4_u32_u8 %3, %8, %8, %3\n v_dot4_u32_u8 %4, %8, %8, %4\n v_dot4_u32_u8 %5, %8, %8, %5\n v_dot4_u32_u8 %6, %8, %8, %6\n v_dot4_u32_u8 %7, %8, %8, %7") }
        if (KIND == 2) { OP8("v_and_or_b32 %0, %0, %8, %8\n v_and_or_b32 %1, %1, %8, %8\n v_and_or_b32 %2, %2, %8, %8\n v_and_or_b32 %3, %3, %8, %8\n v_and_or_b32 %4, %4, %8, %8\n v_and_or_b32 %5, %5, %8, %8\n v_and_or_b32 %6, %6, %8, %8\n v_and_or_b32 %7, %7, %8, %8") }
        if (KIND == 3) { OP8("v_bcnt_u32_b32 %0, %8, %0\n v_bcnt_u32_b32 %1, %8, %1\n v_bcnt_u32_b32 %2, %8, %2\n v_bcnt_u32_b32 %3, %8, %3\n v_bcnt_u32_b32 %4, %8, %4\n v_bcnt_u32_b32 %5, %8, %5\n v_bcnt_u32_b32 %6, %8, %6\n v_bcnt_u32_b32 %7, %8, %7") }
        if (KIND == 4) { OP8("v_sad_u8 %0, %8, %8, %0\n v_sad_u8 %1, %8, %8, %1\n v_sad_u8 %2, %8, %8, %2\n v_sad_u8 %3, %8, %8, %3\n v_sad_u8 %4, %8, %8, %4\n v_sad_u8 %5, %8, %8, %5\n v_sad_u8 %6, %8, %8, %6\n v_sad_u8 %7, %8, %8, %7") }
        if (KIND == 5) { OP8("v_mad_i32_i24 %0, %0, %8, %8\n v_mad_i32_i24 %1, %1, %8, %8\n v_mad_i32_i24 %2, %2, %8, %8\n v_mad_i32_i24 %3, %3, %8, %8\n v_mad_i32_i24 %4, %4, %8, %8\n v_mad_i32_i24 %5, %5, %8, %8\n v_mad_i32_i24 %6, %6, %8, %8\n v_mad_i32_i24 %7, %7, %8, %8") }
        if (KIND == 6) { OP8("v_pk_mad_i16 %0, %0, %8, %8\n v_pk_mad_i16 %1, %1, %8, %8\n v_pk_mad_i16 %2, %2, %8, %8\n v_pk_mad_i16 %3, %3, %8, %8\n v_pk_mad_i16 %4, %4, %8, %8\n v_pk_mad_i16 %5, %5, %8, %8\n v_pk_mad_i16 %6, %6, %8, %8\n v_pk_mad_i16 %7, %7, %8, %8") }
        if (KIND == 7) { OP8("v_perm_b32 %0, %0, %8, %8\n v_perm_b32 %1, %1, %8, %8\n v_perm_b32 %2, %2, %8, %8\n v_perm_b32 %3, %3, %8, %8\n v_perm_b32 %4, %4, %8, %8\n v_perm_b32 %5, %5, %8, %8\n v_perm_b32 %6, %6, %8, %8\n v_perm_b32 %7, %7, %8, %8") }
    }
    out[blockIdx.x * 256 + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}
template <int KIND> void run(const char *name, uint32_t *d, int wavesPerSimd)
{
    // 256 CUs x 4 SIMDs; block = 256 threads = 4 waves (one per SIMD); blocks per CU = wavesPerSimd
    const int blocks = 256 * wavesPerSimd, iters = 20000;
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, d, 100, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<KIND>, dim3(blocks), dim3(256), 0, 0, d, iters, 1u);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    const double instrPerSimd = (double)iters * 8 * wavesPerSimd;          // wave-instructions per SIMD
    printf("%-16s waves/SIMD %d: %.3f ms -> %.2f cycles per wave-instruction per SIMD (at 2.4 GHz)\n", name, wavesPerSimd, ms,
           ms * 1e-3 * 2.4e9 / instrPerSimd);
}
int main()
{
    uint32_t *d; hipMalloc(&d, 256 * 8 * 256 * 4);
    for (int w : {4, 8}) {
        run<0>("v_add_u32", d, w); run<1>("v_dot4_u32_u8", d, w); run<2>("v_and_or_b32", d, w); run<3>("v_bcnt_u32_b32", d, w);
        run<4>("v_sad_u8", d, w); run<5>("v_mad_i32_i24", d, w); run<6>("v_pk_mad_i16", d, w); run<7>("v_perm_b32", d, w);
    }
    return 0;
}
