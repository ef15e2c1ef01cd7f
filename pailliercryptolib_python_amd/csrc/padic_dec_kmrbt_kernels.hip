// The 36-limb digit-pair decrypt kernel in mode PADIC_LDS_KMRBT (kernels_padic.hpp: PADIC_LDS_KMRBS with the right operand of a
// product staged in LDS ahead of the step's squarings), the default for primes of 677..1024 bits.  Own translation unit, as
// padic_dec_kmrbs_kernels.hip, which keeps the kernel that loads the operand into registers at the head of the product
// (PAI_DISABLE=padic_stage).  -DPAI_KMRBT_PARTS / -DPAI_KMRBT_REREAD / -DPAI_KMRBT_MUL_SCHED_EVERY / -DPAI_KMRBT_SQR_SCHED_EVERY /
// -DPAI_KMRBT_LAZY_DIFFS build the measured variants (profiles/r20/README.md, profiles/r25/README.md).
#include "geo_ops.hpp"
#include "kernels_padic.hpp"
#include "launch.hpp"

namespace pai {

void launch_dec_a_padic_kmrbt(hipStream_t s, int gridx, const DecPadicParams& P, const uint32_t* ct, uint32_t* u_out, int n, uint32_t* table) {
    constexpr int NL = 36;
    constexpr int bytes = 3 * NL * BLOCK_THREADS * 4 + 2 * NL * 4;       // as launch_padic<36, 12, PADIC_LDS_KM>
    launch(k_dec_a_padic<NL, 12, MODEXP_WINDOW, PADIC_LDS_KMRBT>, dim3(gridx, 2), dim3(BLOCK_THREADS), bytes, s, P, ct, u_out, n,
           reinterpret_cast<uint4*>(table));
}

}  // namespace pai
