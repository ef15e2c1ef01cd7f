// Launchers of the base-n digit-pair kernels (kernels_padic_enc.hpp) for one limb count; instantiated once per
// translation unit (padic_enc_kernels.hip: 72 limbs, padic_enc36_kernels.hip: 36 limbs) to keep the compile times parallel.
#pragma once
#include "geo_ops.hpp"
#include "kernels_padic_enc.hpp"
#include "kernels_threshold.hpp"
#include "launch.hpp"

namespace pai {

// padic_enc_kara_kernels.hip
void launch_encrypt_padic_kara72(hipStream_t s, int grid, const EncPadicParams& P, const uint32_t* m, const uint32_t* r,
                                 const uint32_t* ct_in, uint32_t* ct_out, int n, int mode);

template <int NL, int U>
struct EncLaunch {
    static constexpr int BYTES2 = 2 * NL * BLOCK_THREADS * 4 + 2 * NL * 4;      // digit pair per lane + modulus copies
    static void fb_table(hipStream_t s, const MontCtx* nctx, const uint32_t* nm1, const uint32_t* hs_dig, const uint32_t* one_dig,
                         uint32_t* table, int J, int wb, const FbBases& fb) {
        constexpr int bytes = 3 * NL * 64 * 4 + 2 * NL * 4;
        launch(k_fb_table_padic<NL, U>, dim3((J + 63) / 64), dim3(64), bytes, s, nctx, nm1, hs_dig, one_dig,
               reinterpret_cast<uint4*>(table), J, wb, fb.bases_plain, fb.base_words, fb.kdig, fb.nd);
    }
    static void fb_expand(hipStream_t s, int grid, const MontCtx* nctx, const uint32_t* nm1, const uint32_t* S, uint32_t* T, int J,
                          int h, uint32_t* mscratch) {
        launch(k_fb_expand_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, nctx, nm1,
               reinterpret_cast<const uint4*>(S), reinterpret_cast<uint4*>(T), J, h, reinterpret_cast<uint4*>(mscratch));
    }
    static void encrypt(hipStream_t s, int grid, const EncPadicParams& P, const uint32_t* m, const uint32_t* r, const uint32_t* ct_in,
                        uint32_t* ct_out, int n, int mode) {
        // one instantiation per (apply_obfuscator?, g-factored table?): the table format is fixed when the table is built
        auto go = [&](auto kernel) {
            launch(kernel, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, m, r, ct_in, ct_out, n, mode);
        };
        const bool gf = PAI_ENC_GFORM_OK && P.fb_gform != 0;
        if constexpr (NL == 72) {
            if (gf && mode == 1 && P.enc_kara != 0) {
                launch_encrypt_padic_kara72(s, grid, P, m, r, ct_in, ct_out, n, mode);
                return;
            }
        }
        if (mode == 2) {
            if (gf) go(k_encrypt_padic<NL, U, true, PAI_ENC_GFORM_OK>);
            else go(k_encrypt_padic<NL, U, true, false>);
        } else {
            if (gf) go(k_encrypt_padic<NL, U, false, PAI_ENC_GFORM_OK>);
            else go(k_encrypt_padic<NL, U, false, false>);
        }
    }
    // g-factoring passes over a finished table (kernels_padic_enc.hpp: k_fb_g_prefix / k_fb_g_finish)
    static void g_prefix(hipStream_t s, int grid, const MontCtx* nctx, const uint32_t* table, size_t count, int K, uint32_t* pref,
                         uint32_t* tot, int tw, uint32_t* mscratch) {
        launch(k_fb_g_prefix<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, nctx, reinterpret_cast<const uint4*>(table),
               count, K, reinterpret_cast<uint4*>(pref), tot, tw, reinterpret_cast<uint4*>(mscratch));
    }
    static void g_finish(hipStream_t s, int grid, const MontCtx* nctx, uint32_t* table, size_t count, int K, const uint32_t* pref,
                         const uint32_t* inv, int tw, uint32_t* mscratch) {
        launch(k_fb_g_finish<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, nctx, reinterpret_cast<uint4*>(table), count,
               K, reinterpret_cast<const uint4*>(pref), inv, tw, reinterpret_cast<uint4*>(mscratch));
    }
    static void ctmul(hipStream_t s, int grid, const CtMulPadicParams& P, const uint32_t* ct, const uint32_t* e, uint32_t* out, int n) {
        launch(k_ctmul_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, ct, e, out, n);
    }
    static void mexp_table(hipStream_t s, int grid, const MexpPadicParams& P, const uint32_t* ct, const uint32_t* ct_inv, int nlanes) {
        launch(k_mexp_table_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, ct, ct_inv, nlanes);
    }
    static void mexp(hipStream_t s, int grid, const MexpPadicParams& P, const uint32_t* e, const uint8_t* sign, uint32_t* out, int nlanes) {
        launch(k_mexp_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, e, sign, out, nlanes);
    }
    static void smexp(hipStream_t s, int grid, const MexpPadicParams& P, const SmexpArgs& S, const uint32_t* e, const uint8_t* sign,
                      uint32_t* out, int nlanes) {
        launch(k_smexp_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, S, e, sign, out, nlanes);
    }
    static void ct_pack(hipStream_t s, int grid, const MexpPadicParams& P, int nrows, int slots, int slot_bits, uint32_t* out, int nlanes) {
        launch(k_ct_pack_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, nrows, slots, slot_bits, out, nlanes);
    }
    static void pow(hipStream_t s, int grid, const PowPadicParams& P, const uint32_t* base, uint32_t* out, int n) {
        launch(k_pow_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, base, out, n);
    }
    static void tcomb(hipStream_t s, int grid, const TcombPadicParams& P, uint32_t* out_pos, uint32_t* out_neg, int n) {
        launch(k_tcomb_padic<NL, U>, dim3(grid), dim3(BLOCK_THREADS), BYTES2, s, P, out_pos, out_neg, n);
    }
};

// the table of one limb count: k_encrypt_padic and the g-factoring passes from LE, everything else from L (their row
// blocks may differ: padic_enc_kernels.hip)
template <class L, class LE>
PadicEncOps enc_ops() {
    PadicEncOps t{};
    t.fb_table = &L::fb_table;
    t.fb_expand = &L::fb_expand;
    t.encrypt = &LE::encrypt;
    t.g_prefix = &LE::g_prefix;
    t.g_finish = &LE::g_finish;
    t.ctmul = &L::ctmul;
    t.pow = &L::pow;
    t.mexp_table = &L::mexp_table;
    t.mexp = &L::mexp;
    t.smexp = &L::smexp;
    t.ct_pack = &L::ct_pack;
    t.tcomb = &L::tcomb;
    return t;
}

}  // namespace pai
