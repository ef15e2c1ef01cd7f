// Issue rate of v_mad_i64_i32 against v_mad_u64_u32 on gfx950, one and two waves per SIMD: the balanced-digit form of the
// digit-pair decrypt kernel (csrc/mont_padic.hpp: kara_pass_bal) turns every multiply-add into the signed one.
// Method of tools/ubench_issue.hip: ONE workgroup per CU (large dynamic LDS allocation), 16 independent accumulator chains,
// the scalar carry-out rotating over four SGPR pairs (back-to-back asm blocks that clobber the same pair get an s_nop from
// the hazard recogniser, which compiled code does not).  A third variant alternates the two instructions, as the kernel does.
// Findings on MI355X: profiles/r15/ubench_mad_signed.jsonl, DESIGN section 2.
// Build: hipcc --offload-arch=gfx950 -O3 tools/ubench_mad_signed.hip -o tools/ubench_mad_signed
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1);} } while (0)

enum V { MAD_U = 0, MAD_I, MAD_UI, NUMV };
static const char* kNames[] = {"v_mad_u64_u32, 16 chains", "v_mad_i64_i32, 16 chains", "alternating u64_u32 / i64_i32, 16 chains"};

#define MAD(op, pair, lo, hi) asm volatile(op " %0, " pair ", %1, %2, %0" : "+v"(acc[k_]) : "v"(a), "v"(b) : lo, hi)

template <int VAR, int THREADS>
__global__ void __launch_bounds__(THREADS) k(uint32_t* out, int iters, uint32_t sa, uint32_t sb) {
    extern __shared__ uint32_t lds[];
    constexpr int NACC = 16;
    uint64_t acc[NACC];
    // operands with the sign bit set in half of the lanes: the signed form sees both signs
    uint32_t a = sa * (threadIdx.x * 2 + 1) + 12345u + (threadIdx.x << 31), b = sb + threadIdx.x * 7u + (threadIdx.x << 30);
#pragma unroll
    for (int k_ = 0; k_ < NACC; ++k_) acc[k_] = ((uint64_t)(a + k_) << 20) | (b ^ k_);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int k_ = 0; k_ < NACC; ++k_) {
                const bool sgn = VAR == MAD_I || (VAR == MAD_UI && ((k_ + r) & 1));
                if (sgn) {
                    if ((k_ & 3) == 0) MAD("v_mad_i64_i32", "s[20:21]", "s20", "s21");
                    if ((k_ & 3) == 1) MAD("v_mad_i64_i32", "s[22:23]", "s22", "s23");
                    if ((k_ & 3) == 2) MAD("v_mad_i64_i32", "s[24:25]", "s24", "s25");
                    if ((k_ & 3) == 3) MAD("v_mad_i64_i32", "s[26:27]", "s26", "s27");
                } else {
                    if ((k_ & 3) == 0) MAD("v_mad_u64_u32", "s[20:21]", "s20", "s21");
                    if ((k_ & 3) == 1) MAD("v_mad_u64_u32", "s[22:23]", "s22", "s23");
                    if ((k_ & 3) == 2) MAD("v_mad_u64_u32", "s[24:25]", "s24", "s25");
                    if ((k_ & 3) == 3) MAD("v_mad_u64_u32", "s[26:27]", "s26", "s27");
                }
            }
        }
    }
    uint64_t s = 0;
#pragma unroll
    for (int k_ = 0; k_ < NACC; ++k_) s ^= acc[k_];
    if (s == 0x123456789abcdefull) { out[0] = (uint32_t)s; lds[threadIdx.x] = 1; }
}

template <int VAR, int THREADS>
static void run(int blocks, int lds_bytes, int iters, uint32_t* d_out) {
    auto kern = k<VAR, THREADS>;
    CK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {                     // the first launch warms up; the best of the other three counts
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(THREADS), lds_bytes, 0, d_out, iters, 3u, 5u);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) best = ms;
    }
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    // cycles per wave-instruction per SIMD: a SIMD hosts THREADS/256 waves of the CU's one block
    const double waves_per_simd = THREADS / 256.0;
    const double cyc = best * 1e-3 * 2.4e9 / ((double)iters * 64 * waves_per_simd);
    printf("{\"variant\": \"%s\", \"waves_per_simd\": %.0f, \"blocks\": %d, \"ms\": %.3f, \"cycles_per_instr_per_simd_at_2.4GHz\": %.3f}\n",
           kNames[VAR], waves_per_simd, blocks, best, cyc);
    fflush(stdout);
}

int main(int argc, char** argv) {
    int iters = argc > 1 ? atoi(argv[1]) : 20000;
    hipDeviceProp_t p; CK(hipGetDeviceProperties(&p, 0));
    int ncu = p.multiProcessorCount;
    uint32_t* d_out; CK(hipMalloc(&d_out, 4096));
    const int BIG = 100 * 1024;
    for (int pass = 0; pass < 2; ++pass) {                  // twice, interleaved: order effects show as a difference between passes
        run<MAD_U, 256>(ncu, BIG, iters, d_out);
        run<MAD_I, 256>(ncu, BIG, iters, d_out);
        run<MAD_UI, 256>(ncu, BIG, iters, d_out);
        run<MAD_U, 512>(ncu, BIG, iters, d_out);
        run<MAD_I, 512>(ncu, BIG, iters, d_out);
        run<MAD_UI, 512>(ncu, BIG, iters, d_out);
    }
    CK(hipFree(d_out));
    return 0;
}
