// The one way a kernel with dynamic LDS is launched: raise the kernel's dynamic-LDS limit to what this launch asks for, launch.
#pragma once
#include <cxxabi.h>
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

namespace pai {

// PAI_DEBUG_OCC=1: print the resident workgroups per CU the runtime computes for a kernel (dev probe)
inline void report_occupancy(const void* fn, hipStream_t s, int block_threads, int bytes) {
    static const bool on = [] { const char* e = std::getenv("PAI_DEBUG_OCC"); return e && e[0] == '1'; }();
    if (!on) return;
    int nb = -1;
    hipFuncAttributes fa;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block_threads, (size_t)bytes);
    (void)hipFuncGetAttributes(&fa, fn);
    const char* sym = hipKernelNameRefByPtr(fn, s);
    char* name = sym ? abi::__cxa_demangle(sym, nullptr, nullptr, nullptr) : nullptr;     // k_modmul<pai::Geo<36, 4, ...>>(...)
    fprintf(stderr, "PAI_OCC %s: blocks/CU=%d lds=%d B regs=%d scratch=%zu B\n", name ? name : (sym ? sym : "?"), nb, bytes, fa.numRegs,
            (size_t)fa.localSizeBytes);
    std::free(name);
}

// The attribute belongs to the kernel ON THE CURRENT DEVICE and one process serves several devices (pai_scatter): it is
// set on every launch, never cached.
template <class... P, class... A>
inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const A&... args) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    report_occupancy((const void*)kernel, s, (int)block.x, lds_bytes);
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
}

}  // namespace pai
