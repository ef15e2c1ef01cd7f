// Instantiations of the one-digit fold modulo n behind pai_opening_fold (kernels_open_fold.hpp): 72 limbs (n of 1400..2048 bits,
// 8-row blocks) and 36 limbs (n of 700..1024 bits, 12-row blocks), the row blocks of the digit-pair kernels' ct x pt.
// Own translation unit (see padic_dec_kernels.hip).
#include "kernels_open_fold.hpp"

namespace pai {

template <int NL, int U>
static void open_fold_go(hipStream_t s, int grid, const OpenFoldParams& P, const uint32_t* r, const uint32_t* m, const uint32_t* e,
                         uint32_t* out_b, uint32_t* out_m, int nlanes) {
    constexpr int BYTES = 2 * NL * BLOCK_THREADS * 4 + 3 * NL * 4;      // two digits per lane + n, R^2 mod n, R mod n
    launch(k_open_fold<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES, s, P, r, m, e, out_b, out_m, nlanes);
}

bool launch_open_fold(int nl, hipStream_t s, int grid, const OpenFoldParams& P, const uint32_t* r, const uint32_t* m, const uint32_t* e,
                      uint32_t* out_b, uint32_t* out_m, int nlanes) {
    if (nl == 72) open_fold_go<72, 8>(s, grid, P, r, m, e, out_b, out_m, nlanes);
    else if (nl == 36) open_fold_go<36, 12>(s, grid, P, r, m, e, out_b, out_m, nlanes);
    else return false;
    return true;
}

size_t open_fold_table_bytes(int nl, int chunk, int wbits, size_t blocks) {
    return (size_t)chunk * (((size_t)1 << wbits) - 1) * (size_t)nl * 4 * blocks * BLOCK_THREADS;
}

}  // namespace pai
