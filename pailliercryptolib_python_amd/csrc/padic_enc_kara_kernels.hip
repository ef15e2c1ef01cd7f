// The Karatsuba-column mode of k_encrypt_padic (kernels_padic_enc.hpp: KARA) for 72 limbs, DJN encryption on a g-factored
// table.  Own translation unit: the four inlined half-width steps are the longest straight-line code of the library.
#include "padic_enc_launch.hpp"

namespace pai {

void launch_encrypt_padic_kara72(hipStream_t s, int grid, const EncPadicParams& P, const uint32_t* m, const uint32_t* r,
                                 const uint32_t* ct_in, uint32_t* ct_out, int n, int mode) {
    launch(k_encrypt_padic<72, 12, false, true, true>, dim3(grid), dim3(BLOCK_THREADS), EncLaunch<72, 12>::BYTES2, s, P, m, r, ct_in,
           ct_out, n, mode);
}

}  // namespace pai
