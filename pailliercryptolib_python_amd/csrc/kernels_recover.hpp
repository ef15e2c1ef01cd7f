// Randomness recovery (pai_recover_r): the r of a ciphertext's opening c = (1 + m n) r^n mod n^2, computed by the holder of p and q.
//
//   k_rrec_a   per (element, prime s in {p, q}): r_s = (c mod s)^(d_s) mod s, d_s = n^-1 mod (s - 1)
//   k_rrec_b   r = r_p + p ((r_q - r_p) p^-1 mod q)                       (the Garner tail of k_dec_b, no L function, no h)
//
// Modulo s the factor 1 + m n is 1 and r -> r^n is a bijection of the units (gcd(n, s - 1) = 1), undone by the exponent d_s.
// Both kernels run on the lane-group geometry of the primes THEMSELVES (sk->pr[w]: half the limbs of decryption's s^2), with the
// row engine, the [entry][limb][slot] window tables and the wave-uniform exponent windows of k_modexp_fixed.
#pragma once
#include "kernels_paillier.hpp"

namespace pai {

struct RrecAParams {
    const MontCtx* pr[2];        // moduli p, q
    const uint32_t* kdig[2];     // [nd][NL] limbs of R^(i+2) mod s: digit i of a row times this is (digit R^i) R mod s, no division
    const uint32_t* expo[2];     // d_s = n^-1 mod (s - 1), packed u32 words
    int ewords[2], ebits[2];
    int nd;                      // base-R digits of a ciphertext row (R = 2^(29 NL))
    int ct_words, r_words;       // r_words = words of a residue modulo the wider prime
};

// Stage A.  blockIdx.y selects the prime.  The row enters Montgomery form modulo s as sum_i MM(digit_i, R^(i+2)): every term is
// below 2 s (digit_i < R, the constant < s), the running sum is brought back below 2 s by two conditional subtractions per term.
// A row that s divides gives 0 all the way (d_s >= 1): r_s = 0, no special case.  The result leaves canonical: the lift needs r_p
// as an integer and r_q - r_p as a residue, so a Montgomery-form exit would cost the lift the product it saves here.
template <class G, int W>
__global__ void __launch_bounds__(BLOCK_THREADS, PAI_LG_WAVES(G))
k_rrec_a(RrecAParams P, const uint32_t* __restrict__ ct, uint32_t* __restrict__ r_out /*[2][n][r_words]*/, int n,
         uint32_t* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int which = blockIdx.y;
    const MontCtx* ctx = P.pr[which];
    const uint32_t* expo = P.expo[which];
    const uint32_t* kdig = P.kdig[which];
    const int ewords = P.ewords[which], ebits = P.ebits[which];
    const int t = G::gl();
    typename G::NM nm;
    load_modulus<G>(nm, ctx, lds);
    const uint32_t n0inv = ctx->n0inv;
    const size_t nslots = (size_t)gridDim.x * gridDim.y * G::EPB;
    const size_t slot = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * G::EPB + G::elem();
    auto tbl = [&](int entry, int j) -> uint32_t& {
        return table[((size_t)entry * G::NL + (G::NLL * t + j)) * nslots + slot];
    };
    const int nwin = (ebits + W - 1) / W;
    const int tiles = (n + G::EPB - 1) / G::EPB;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ei = tile * G::EPB + G::elem();
        const bool live = ei < n;
        const int es = live ? ei : n - 1;
        const uint32_t* row = ct + (size_t)es * P.ct_words;
        uint32_t x[G::NLL];
        {
            uint32_t bR[G::NLL];
            {   // (c mod s) R
                uint32_t c[G::NLL];
                load_elem_off<G>(bR, row, P.ct_words, 0);
                load_const_slice<G>(c, kdig);
                mm_times<G>(bR, c, lds, nm, n0inv);
#pragma unroll 1
                for (int i = 1; i < P.nd; ++i) {
                    uint32_t d[G::NLL];
                    load_elem_off<G>(d, row, P.ct_words, G::NL * i);
                    load_const_slice<G>(c, kdig + (size_t)i * G::NL);
                    mm_times<G>(d, c, lds, nm, n0inv);
                    add_limbs<G>(bR, d);
                    cond_sub<G::NLL, G::T>(bR, nm);                 // < 4 s -> < 2 s
                    cond_sub<G::NLL, G::T>(bR, nm);
                }
            }
#pragma unroll
            for (int j = 0; j < G::NLL; ++j) { x[j] = bR[j]; tbl(1, j) = bR[j]; }
#pragma unroll 1
            for (int k = 2; k < (1 << W); ++k) {
                mm_times<G>(x, bR, lds, nm, n0inv);
#pragma unroll
                for (int j = 0; j < G::NLL; ++j) tbl(k, j) = x[j];
            }
        }
        {
            const uint32_t wv = exp_bits(expo, ewords, (nwin - 1) * W, W);
            if (wv == 0) load_const_slice<G>(x, ctx->one);
            else {
#pragma unroll
                for (int j = 0; j < G::NLL; ++j) x[j] = tbl((int)wv, j);
            }
        }
#pragma unroll 1
        for (int wi = nwin - 2; wi >= 0; --wi) {
            const uint32_t wv = exp_bits(expo, ewords, wi * W, W);
#pragma unroll 1
            for (int s = 0; s < W; ++s) mm_square<G>(x, lds, nm, n0inv);
            if (wv != 0) {
                uint32_t y[G::NLL];
#pragma unroll
                for (int j = 0; j < G::NLL; ++j) y[j] = tbl((int)wv, j);
                mm_times<G>(x, y, lds, nm, n0inv);
            }
        }
        {
            uint32_t one[G::NLL];
            set_plain_one<G>(one);
            mm_times<G>(x, one, lds, nm, n0inv);
            cond_sub<G::NLL, G::T>(x, nm);
        }
        if (live) store_elem<G>(x, r_out + ((size_t)which * n + ei) * P.r_words, P.r_words, lds);
    }
}

struct RrecBParams {
    const MontCtx* pr[2];        // moduli p, q
    const uint32_t* pinvqR;      // (p^-1 mod q) R mod q
    int r_words, out_words;      // words of a stage-A residue, of a result row (n_words)
};

// Stage B: t = (r_q - r_p + q) p^-1 mod q, r = r_p + p t < p q — in words, what k_dec_b does after its L functions.
template <class G>
__global__ void __launch_bounds__(BLOCK_THREADS, PAI_LG_WAVES(G))
k_rrec_b(RrecBParams P, const uint32_t* __restrict__ r_in /*[2][n][r_words]*/, uint32_t* __restrict__ r_out, int n) {
    static_assert(!G::NMLDS, "stage B keeps the (small) prime moduli in registers");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];       // 2 operand buffers
    uint32_t* ldsA = lds;
    uint32_t* ldsB = lds + G::LDS_WORDS;
    const int t = G::gl(), e = G::elem();
    const int tiles = (n + G::EPB - 1) / G::EPB;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ei = tile * G::EPB + e;
        const bool live = ei < n;
        const int es = live ? ei : n - 1;
        uint32_t rp[G::NLL], d[G::NLL];
        NmRegs<G::NLL> nq;
        load_const_slice<G>(nq.v, P.pr[1]->n);
        load_elem<G>(rp, r_in + (size_t)es * P.r_words, P.r_words);
        {
            uint32_t rq[G::NLL];
            load_elem<G>(rq, r_in + ((size_t)n + es) * P.r_words, P.r_words);
            int64_t sd[G::NLL];
#pragma unroll
            for (int j = 0; j < G::NLL; ++j) sd[j] = (int64_t)rq[j] - (int64_t)rp[j] + (int64_t)nq.v[j];
            Rows<G::NLL, G::U, G::T>::finish_signed(sd, d);
        }
        uint32_t c[G::NLL];
        load_const_slice<G>(c, P.pinvqR);
        mm_times<G>(d, c, ldsA, nq, P.pr[1]->n0inv);
        cond_sub<G::NLL, G::T>(d, nq);
        stage_b<G>(d, ldsA);
        uint32_t pl[G::NLL], hi[G::NLL];
        load_const_slice<G>(pl, P.pr[0]->n);
        mul_plain<G::NLL, G::U, G::T>(hi, rp, pl, ldsA + e, G::EPB, ldsB + e, G::EPB);
        wave_lds_fence();
        // r = lo (LDS B, NL limbs) + hi (registers) 2^(29 NL) as packed words
#pragma unroll
        for (int j = 0; j < G::NLL; ++j) ldsA[(G::NLL * t + j) * G::EPB + e] = hi[j];
        wave_lds_fence();
        if (live) {
            uint32_t* row = r_out + (size_t)ei * P.out_words;
            auto limb = [&](int J) -> uint64_t {
                if (J < G::NL) return ldsB[J * G::EPB + e];
                if (J < 2 * G::NL) return ldsA[(J - G::NL) * G::EPB + e];
                return 0;
            };
            for (int k = t; k < P.out_words; k += G::T) {
                const int j0 = (32 * k) / RB;
                const int s0 = 32 * k - RB * j0;
                uint64_t v = limb(j0) >> s0;
                v |= limb(j0 + 1) << (RB - s0);
                v |= limb(j0 + 2) << (2 * RB - s0);
                row[k] = (uint32_t)v;
            }
        }
        wave_lds_fence();
    }
}

}  // namespace pai
