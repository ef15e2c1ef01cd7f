// Instantiates every kernel for one geometry and fills its GeoOps table.
#pragma once
#include "geo_ops.hpp"
#include "kernels_modexp.hpp"
#include "launch.hpp"

namespace pai {

template <class G>
struct GeoInst {
    // the tile-I/O kernels (k_modmul, k_pow2, k_add_aligned, k_addn, k_segprod) keep the modulus slice in registers
    using GM = Geo<G::NLL, G::T, G::U, false>;
    using GM1 = Geo<G::NLL, G::T, G::U, false, true>;
    static constexpr int TILE_BYTES = GM::LDS_BYTES + GM::STAGE_BYTES;
    // wide-group geometries with a minus-one context (c) and the true modulus' context (fin) run a kernel on GM1, everything
    // else on the kernel's usual geometry without fin: go(geometry, fin)
    template <class Usual, class F>
    static void with_m1(const MontCtx* fin, F go) {
        if constexpr (G::T >= 16) {
            if (fin != nullptr) {
                go(GM1{}, fin);
                return;
            }
        }
        go(Usual{}, (const MontCtx*)nullptr);
    }
    // (measured and dropped, profiles/r04/ctadd_ab_*.jsonl: the same products on per-wave LDS regions with 18 limbs x 8 lanes at
    // three or four waves per SIMD: 2.14-2.35 ms per 2^20 against 1.98 ms here)
    static void modmul(hipStream_t s, int grid, const MontCtx* c, const uint32_t* a, const uint32_t* b, uint32_t* out,
                       int n, int w32, int b_bcast, int mode, const MontCtx* fin) {
        constexpr int bytes = TILE_BYTES + GM::NL * 4;     // + the R^2 copy
        with_m1<GM>(fin, [&](auto g, const MontCtx* f) {
            launch(k_modmul<decltype(g)>, dim3(grid), dim3(BLOCK_THREADS), bytes, s, c, a, b, out, n, w32, b_bcast, mode, f);
        });
    }
    static void modexp_fixed(hipStream_t s, int grid, const MontCtx* c, const uint32_t* base, int base_w32,
                             const uint32_t* expo, int ewords, int ebits, uint32_t* out, int out_w32, int n,
                             uint32_t* table, int keep_mont) {
        launch(k_modexp_fixed<G, MODEXP_WINDOW>, dim3(grid), dim3(BLOCK_THREADS), G::LDS_BYTES, s, c, base, base_w32, expo, ewords,
               ebits, out, out_w32, n, table, keep_mont);
    }
    static void modexp_var(hipStream_t s, int grid, const MontCtx* c, const uint32_t* base, int base_w32, int base_shift,
                           const uint32_t* expo, int ew, int ebits_max, int exp_bcast, uint32_t* out, int out_w32,
                           int n, int keep_mont, int out_raw) {
        launch(k_modexp_var<G>, dim3(grid), dim3(BLOCK_THREADS), G::LDS_BYTES, s, c, base, base_w32, base_shift, expo, ew, ebits_max,
               exp_bcast, out, out_w32, n, keep_mont, out_raw);
    }
    static void encrypt(hipStream_t s, int grid, EncParams P, const uint32_t* m, const uint32_t* r,
                        const uint32_t* ct_in, uint32_t* ct_out, int n, int mode) {
        const dim3 g(grid), b(BLOCK_THREADS);
        if constexpr (G::T >= 16 && G::T <= 64) {
            if (mode == 7)         // table conversion to a minus-one context's Montgomery form: m = table in, ct_out = table out, r = the constant
                return launch(k_fb_to_m1<GM1>, g, b, GM1::LDS_BYTES, s, P.nsq, m, ct_out, n, r);
            if ((mode == 3 || mode == 0) && P.fin != nullptr)       // ct + plaintext / raw encryption of small batches on a minus-one context
                return launch(k_encrypt<GM1>, g, b, GM1::LDS_BYTES, s, P, m, r, ct_in, ct_out, n, mode);
            if (mode >= 5 && P.fin != nullptr)       // the shared chain on a minus-one context
                return launch(k_encrypt_tree<GM1>, g, b, GM1::LDS_BYTES, s, P, m, r, ct_in, ct_out, n, mode - 4);
            if (mode >= 5)         // modes 5 / 6: modes 1 / 2 with the fixed-base chain shared by the four waves (grid counts 64 / T integers)
                return launch(k_encrypt_tree<G>, g, b, G::LDS_BYTES, s, P, m, r, ct_in, ct_out, n, mode - 4);
        }
        launch(k_encrypt<G>, g, b, G::LDS_BYTES, s, P, m, r, ct_in, ct_out, n, mode);
    }
    static void pair_finish(hipStream_t s, int grid, EncParams P, const uint32_t* wv, int wv_words, const uint32_t* ct_in,
                            uint32_t* ct_out, int n, int mul_ct) {
        launch(k_pair_finish<G>, dim3(grid), dim3(BLOCK_THREADS), G::LDS_BYTES, s, P, wv, wv_words, ct_in, ct_out, n, mul_ct);
    }
    static void fb_expand(hipStream_t s, int grid, const MontCtx* c, const uint32_t* S, uint32_t* T, int J, int h) {
        launch(k_fb_expand<G>, dim3(grid), dim3(BLOCK_THREADS), G::LDS_BYTES, s, c, S, T, J, h);
    }
    static void dec_a(hipStream_t s, int gridx, DecAParams P, const uint32_t* ct, uint32_t* u_out, int n,
                      uint32_t* table) {
        // the wide-group (latency) geometries run stage A on minus-one contexts (mont_dev.hpp: Rows::block_m1)
        using GD = Geo<G::NLL, G::T, G::U, G::NMLDS, (G::T >= 16)>;
        if constexpr (GD::M1) {
            if (P.rl) {         // gridx counts workgroups of EPB / 2 integers here
                constexpr int bytes = ((RL_RING + 1) * GD::LDS_WORDS + 16) * 4;
                return launch(k_dec_a_rl<GD>, dim3(gridx, 2), dim3(BLOCK_THREADS), bytes, s, P, ct, u_out, n);
            }
        }
        launch(k_dec_a<GD, MODEXP_WINDOW>, dim3(gridx, 2), dim3(BLOCK_THREADS), GD::LDS_BYTES, s, P, ct, u_out, n, table);
    }
    static void dec_b(hipStream_t s, int grid, DecBParams P, const uint32_t* u_in, uint32_t* m_out, int n) {
        launch(k_dec_b<G>, dim3(grid), dim3(BLOCK_THREADS), 2 * G::LDS_WORDS * 4, s, P, u_in, m_out, n);
    }
    static void modexp_var_win(hipStream_t s, int grid, const MontCtx* c, const uint32_t* base, int base_w32, const uint32_t* expo,
                               int ew, int ebits_max, int exp_bcast, uint32_t* out, int out_w32, int n, uint32_t* table, int wbits,
                               const MontCtx* fin) {
        // 8-lane geometries: modulus slice from LDS (3072 / 4096-bit ct * pt 20.8 -> 20.5 / 32.7 -> 31.8 ms per 65536)
        using GV = Geo<G::NLL, G::T, G::U, (G::T >= 8 && G::NLL % 4 == 0)>;
        with_m1<GV>(fin, [&](auto g, const MontCtx* f) {
            using GK = decltype(g);
            if constexpr (GK::M1) {
                if (wbits == 0) {    // right to left on wave pairs, no table (grid counts workgroups of EPB / 2 integers)
                    constexpr int bytes = ((RL_RING + 1) * GK::LDS_WORDS + 16) * 4;
                    return launch(k_modexp_rl<GK>, dim3(grid), dim3(BLOCK_THREADS), bytes, s, c, base, base_w32, expo, ew, ebits_max,
                                  exp_bcast, out, out_w32, n, f);
                }
            }
            launch(k_modexp_var_win<GK>, dim3(grid), dim3(BLOCK_THREADS), VarWinCfg<GK>::LDS_BYTES, s, c, base, base_w32, expo, ew,
                   ebits_max, exp_bcast, out, out_w32, n, table, wbits, f);
        });
    }
    static void sq_chain(hipStream_t s, const MontCtx* c, const MontCtx* fin, const uint32_t* base, int w32, uint32_t* out, int h,
                         int nsnap) {
        with_m1<G>(fin, [&](auto g, const MontCtx* f) {
            using GK = decltype(g);
            launch(k_sq_chain<GK>, dim3(1), dim3(BLOCK_THREADS), GK::LDS_BYTES, s, c, f, base, w32, out, h, nsnap);
        });
    }
    static void pow2(hipStream_t s, int grid, const MontCtx* c, uint32_t* ct, const int32_t* delta, int delta_bcast,
                     int n, int w32, const MontCtx* fin) {
        constexpr int bytes = TILE_BYTES + GM::NL * 4;     // + the R^2 copy
        with_m1<GM>(fin, [&](auto g, const MontCtx* f) {
            launch(k_pow2<decltype(g)>, dim3(grid), dim3(BLOCK_THREADS), bytes, s, c, ct, delta, delta_bcast, n, w32, f);
        });
    }
    static void add_aligned(hipStream_t s, int grid, const MontCtx* c, const uint32_t* a, const uint32_t* b, int b_bcast,
                            const int32_t* delta, uint32_t* out, int n, int w32, const uint32_t* entry, const MontCtx* fin) {
        constexpr int bytes = TILE_BYTES + GM::NL * 4;
        with_m1<GM>(fin, [&](auto g, const MontCtx* f) {
            launch(k_add_aligned<decltype(g)>, dim3(grid), dim3(BLOCK_THREADS), bytes, s, c, a, b, b_bcast, delta, out, n, w32, entry, f);
        });
    }
    static void addn(hipStream_t s, int grid, const MontCtx* c, AddnArgs A, uint32_t* out, int n, int w32, const uint32_t* rpow) {
        constexpr int bytes = TILE_BYTES + GM::NL * 4;     // + the domain-entry constant
        launch(k_addn<GM>, dim3(grid), dim3(BLOCK_THREADS), bytes, s, c, A, out, n, w32, rpow);
    }
    static void segprod(hipStream_t s, int grid, const MontCtx* c, SegArgs A, int w32, const uint32_t* rpow) {
        launch(k_segprod<GM>, dim3(grid), dim3(BLOCK_THREADS), TILE_BYTES, s, c, A, w32, rpow);
    }
    static void segscan(hipStream_t s, int grid, const MontCtx* c, ScanArgs A, int w32, const uint32_t* rpow) {
        launch(k_segscan<GM>, dim3(grid), dim3(BLOCK_THREADS), TILE_BYTES, s, c, A, w32, rpow);
    }
    static void mexp_table(hipStream_t s, int grid, const MontCtx* c, const uint32_t* ct, const uint32_t* ct_inv, int w32,
                           uint32_t* table, int nentries, int nsigns, int wbits) {
        launch(k_mexp_table<G>, dim3(grid), dim3(BLOCK_THREADS), G::LDS_BYTES, s, c, ct, ct_inv, w32, table, nentries, nsigns, wbits);
    }
    static void mexp(hipStream_t s, int grid, const MontCtx* c, MexpParams P, const uint32_t* table, const uint32_t* e,
                     const uint8_t* sign, uint32_t* out, int nlanes) {
        launch(k_mexp<GM>, dim3(grid), dim3(BLOCK_THREADS), GM::LDS_BYTES, s, c, P, table, e, sign, out, nlanes);
    }
    static void smexp(hipStream_t s, int grid, const MontCtx* c, MexpParams P, SmexpArgs S, const uint32_t* table, const uint32_t* e,
                      const uint8_t* sign, uint32_t* out, int nlanes) {
        launch(k_smexp<GM>, dim3(grid), dim3(BLOCK_THREADS), GM::LDS_BYTES, s, c, P, S, table, e, sign, out, nlanes);
    }
    static void modmul_msb(hipStream_t s, int grid, const MsbCtx* c, const uint32_t* a, const uint32_t* b, uint32_t* out, int n, int w32) {
        if constexpr (G::T <= 8) {
            // (rows per block: the geometry's own — 9 / 12 / 18 on 36 x 4 spill inside the row loop, /tmp probe of round 6)
            launch(k_modmul_msb<GM>, dim3(grid), dim3(BLOCK_THREADS), MsbLds<GM>::WORDS * 4, s, c, a, b, out, n, w32);
        }
    }
    static void rrec_a(hipStream_t s, int gridx, RrecAParams P, const uint32_t* ct, uint32_t* r_out, int n, uint32_t* table) {
        launch(k_rrec_a<G, MODEXP_WINDOW>, dim3(gridx, 2), dim3(BLOCK_THREADS), G::LDS_BYTES, s, P, ct, r_out, n, table);
    }
    static void rrec_b(hipStream_t s, int grid, RrecBParams P, const uint32_t* r_in, uint32_t* r_out, int n) {
        launch(k_rrec_b<G>, dim3(grid), dim3(BLOCK_THREADS), 2 * G::LDS_WORDS * 4, s, P, r_in, r_out, n);
    }
    static size_t table_words(size_t blocks) { return (size_t)(1u << MODEXP_WINDOW) * G::NL * blocks * G::EPB; }

    static const GeoOps* ops() {
        static const GeoOps o = [] {
            GeoOps t{};
            t.nll = G::NLL, t.t = G::T, t.u = G::U, t.nl = G::NL, t.epb = G::EPB;
            t.lds_bytes = G::LDS_BYTES;
            t.lds_bytes_b = 2 * G::LDS_WORDS * 4;
            t.modmul = &modmul;
            t.modexp_fixed = &modexp_fixed;
            t.modexp_var = &modexp_var;
            t.modexp_var_win = &modexp_var_win;
            t.encrypt = &encrypt;
            t.fb_expand = &fb_expand;
            t.dec_a = &dec_a;
            t.dec_b = &dec_b;
            t.pow2 = &pow2;
            t.sq_chain = &sq_chain;
            t.add_aligned = &add_aligned;
            t.addn = &addn;
            t.table_words = &table_words;
            t.pair_finish = &pair_finish;
            t.mexp_table = &mexp_table;
            t.mexp = &mexp;
            t.modmul_msb = G::T <= 8 ? &modmul_msb : nullptr;
            t.segprod = &segprod;
            t.segscan = &segscan;
            t.smexp = &smexp;
            t.rrec_a = &rrec_a;
            t.rrec_b = &rrec_b;
            return t;
        }();
        return &o;
    }
};

}  // namespace pai
