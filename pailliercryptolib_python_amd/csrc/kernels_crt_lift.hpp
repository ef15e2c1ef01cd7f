// Garner lift of the owner-side CRT encryption (dispatch_encrypt_crt.hpp): from the residues c_p = x mod p^2 and
// c_q = x mod q^2 (canonical, packed words) to x mod n^2,
//   h = (c_q - c_p) (p^-2 mod q^2) mod q^2,   x = c_p + p^2 h   (< p^2 + p^2 (q^2 - 1) = n^2: canonical as it stands).
// The job of k_dec_b (kernels_paillier.hpp) one size up: the lane-group geometry of q^2, one Montgomery product modulo q^2
// against the constant (p^-2 mod q^2) R, then the plain product p^2 h seeded with c_p.  The handle keeps p < q, so
// c_p < p^2 < q^2 and c_q - c_p + q^2 lies in (0, 2 q^2): a lazy operand of the product as it is.
#pragma once
#include "kernels_common.hpp"

namespace pai {

struct CrtLiftParams {
    const MontCtx* q2;           // modulus q^2 on the lift's geometry (R = 2^(29 NL))
    const uint32_t* p2;          // p^2, radix 29, NLMAX-padded
    const uint32_t* pinv2R;      // (p^-2 mod q^2) R mod q^2, radix 29, NLMAX-padded
    int in_words;                // packed words of a residue row (covers q^2)
    int ct_words;
};

template <class G>
__global__ void __launch_bounds__(BLOCK_THREADS, 1)
k_crt_lift(CrtLiftParams P, const uint32_t* __restrict__ c_in /*[2][n][in_words]*/, uint32_t* __restrict__ ct_out, int n) {
    static_assert(!G::NMLDS && !G::M1, "the lift keeps q^2 in registers on a conventional context");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];       // 2 operand buffers
    uint32_t* ldsA = lds;
    uint32_t* ldsB = lds + G::LDS_WORDS;
    const int t = G::gl(), e = G::elem();
    NmRegs<G::NLL> nq;
    load_const_slice<G>(nq.v, P.q2->n);
    const uint32_t n0inv = P.q2->n0inv;
    const int tiles = (n + G::EPB - 1) / G::EPB;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ei = tile * G::EPB + e;
        const bool live = ei < n;
        const int es = live ? ei : n - 1;
        uint32_t cp[G::NLL], d[G::NLL];
        load_elem<G>(cp, c_in + (size_t)es * P.in_words, P.in_words);
        load_elem<G>(d, c_in + ((size_t)n + es) * P.in_words, P.in_words);
        {   // d = c_q - c_p + q^2
            int64_t sd[G::NLL];
#pragma unroll
            for (int j = 0; j < G::NLL; ++j) sd[j] = (int64_t)d[j] - (int64_t)cp[j] + (int64_t)nq.v[j];
            Rows<G::NLL, G::U, G::T>::finish_signed(sd, d);
        }
        uint32_t c[G::NLL];
        load_const_slice<G>(c, P.pinv2R);
        mm_times<G>(d, c, ldsA, nq, n0inv);                          // h (lazy)
        cond_sub<G::NLL, G::T>(d, nq);
        stage_b<G>(d, ldsA);
        // x = c_p + p^2 h: low NL limbs to LDS B, high NL limbs in registers
        uint32_t hi[G::NLL];
        load_const_slice<G>(c, P.p2);
        mul_plain<G::NLL, G::U, G::T>(hi, cp, c, ldsA + e, G::EPB, ldsB + e, G::EPB);
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < G::NLL; ++j) ldsA[(G::NLL * t + j) * G::EPB + e] = hi[j];
        wave_lds_fence();
        if (live) {
            uint32_t* row = ct_out + (size_t)ei * P.ct_words;
            auto limb = [&](int J) -> uint64_t {
                if (J < G::NL) return ldsB[J * G::EPB + e];
                if (J < 2 * G::NL) return ldsA[(J - G::NL) * G::EPB + e];
                return 0;
            };
            for (int k = t; k < P.ct_words; k += G::T) {
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
