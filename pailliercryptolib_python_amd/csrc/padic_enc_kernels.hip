// Instantiations of the base-n digit-pair kernels (kernels_padic_enc.hpp): fixed-base table construction, raw / DJN
// encryption, apply_obfuscator, ciphertext * plaintext and the standard scheme's r^n.  72 limbs here (n of 1400..2048
// bits), 36 limbs in padic_enc36_kernels.hip (n of 700..1024 bits).  Own translation units (see padic_dec_kernels.hip).
#include "padic_enc_launch.hpp"

namespace pai {

using L72 = EncLaunch<72, 8>;     // rows per block of the 72-limb products: 8
// k_encrypt_padic runs 12-row blocks: with the fused product rule (two accumulator windows, 320+ registers, parked in
// AGPRs between row blocks) fewer, larger blocks mean fewer window round trips — 67.2 vs 69.8 ms per 2^20; ct x pt
// prefers 8 rows (4.87 vs 5.07 ms per 65536) and r^n does not care (144-150 ms per 65536 either way)
using L72E = EncLaunch<72, 12>;

int padic_enc_nl_for_n_bits(int bits) {
    if (bits >= 700 && RB * 36 >= bits + 20) return 36;
    if (bits >= 1400 && RB * 72 >= bits + 20) return 72;
    return 0;
}
const PadicEncOps* padic_enc_ops(int nl) {
    static const PadicEncOps o72 = enc_ops<L72, L72E>();
    return nl == 72 ? &o72 : (nl == 36 ? padic_enc_ops_36() : nullptr);
}
bool padic_enc_gform_supported() { return PAI_ENC_GFORM_OK; }
size_t ctmul_padic_table_words(int nl, int wbits, size_t blocks) { return ((size_t)1 << wbits) * 2 * nl * blocks * BLOCK_THREADS; }

}  // namespace pai
