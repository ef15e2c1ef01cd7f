// Threshold decryption, the combine: from t partial decryptions c_j = c^(2 Delta s_j) mod n^2 and the integer
// Lagrange coefficients mu_j of the share set,
//     x = prod_j c_j^(2 mu_j) = P+ (P-)^-1 mod n^2,     m = ((x - 1) / n) theta mod n,     theta = (4 Delta^2)^-1 mod n.
//   k_tcomb_padic<NL, U>  P+ and P- on base-n digit pairs, one element per lane (keys the digit engine serves)
//   k_tfinish<WMAX>       x -> m with the test x = 1 (mod n), word-serial on 32-bit words, any key size
#pragma once
#include "kernels_padic_enc.hpp"

namespace pai {

constexpr int TCOMB_MAX_PARTS = 16;
constexpr int TCOMB_MU_WORDS = 4;

// ---- P+ = prod_(mu_j > 0) c_j^|2 mu_j|,  P- = prod_(mu_j < 0) c_j^|2 mu_j|  mod n^2 ---------------------------------------------------
// Modelled on k_ctmul_padic: the accumulator pair (A, B) in LDS, a global per-slot table — here the t partials in Montgomery
// digit form where k_ctmul_padic keeps powers.  The exponents are kernel arguments, so the whole control flow is wave-uniform: a
// plain binary chain, most significant bit first, one squaring per bit and one table product per set bit of a member's exponent;
// the chain starts from the table entry of its first set bit.  A side without members is not run.
struct TcombPadicParams {
    const MontCtx* nctx;         // modulus n (NL limbs)
    const uint32_t* nm1;         // n - 1 limbs
    const uint32_t* nsq;         // n^2 limbs (2 NL, radix 29)
    const uint32_t* kdig;        // [nd][2][NL] digit pairs of R^(i+2) mod n^2
    uint4* mscratch;             // [2 NC][nslots]
    uint4* table;                // [t][2][NC][nslots]: the partials in Montgomery digit form
    int nd, ct_words, t;
    unsigned neg_mask;           // bit j: member j is on the negative side
    const uint32_t* parts[TCOMB_MAX_PARTS];
    uint32_t mu[TCOMB_MAX_PARTS][TCOMB_MU_WORDS];     // |2 mu_j|, little-endian words, non-zero
};

template <int NL, int U>
__global__ void __launch_bounds__(BLOCK_THREADS, 1)
k_tcomb_padic(TcombPadicParams P, uint32_t* __restrict__ out_pos, uint32_t* __restrict__ out_neg, int n) {
    using E = Padic<NL, U, false>;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* ldsn = lds + (BLOCK_THREADS / 64) * 2 * E::DIGIT_WORDS;
    for (int i = threadIdx.x; i < NL; i += BLOCK_THREADS) { ldsn[i] = P.nctx->n[i]; ldsn[NL + i] = P.nm1[i]; }
    __syncthreads();
    uint32_t sn[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) sn[j] = __builtin_amdgcn_readfirstlane(ldsn[j]);
    const uint32_t* nm = sn;
    const uint32_t* nm_lds = ldsn;
    const uint32_t* nm1 = ldsn + NL;
    const uint32_t n0inv = P.nctx->n0inv;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4* A = reinterpret_cast<uint4*>(lds + wave * 2 * E::DIGIT_WORDS) + lane;
    uint4* B = A + E::NC * 64;
    const size_t nslots = (size_t)gridDim.x * BLOCK_THREADS;
    const size_t slot = (size_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
    const typename E::MBuf M{P.mscratch + slot, nslots};
    auto tbl = [&](int ent, int d, int c) -> uint4& { return P.table[(((size_t)ent * 2 + d) * E::NC + c) * nslots + slot]; };
    auto from_table = [&](int ent, int d) {
        return [&, ent, d](int blk, uint32_t (&xv)[U]) {
#pragma unroll
            for (int c = 0; c < E::UC; ++c) {
                const uint4 t = tbl(ent, d, E::UC * blk + c);
                xv[4 * c] = t.x; xv[4 * c + 1] = t.y; xv[4 * c + 2] = t.z; xv[4 * c + 3] = t.w;
            }
        };
    };
    auto mu_bit = [&](int j, int bit) -> bool { return (P.mu[j][bit >> 5] >> (bit & 31)) & 1u; };
    const int T = P.t;
    const int tiles = (n + BLOCK_THREADS - 1) / BLOCK_THREADS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ei = tile * BLOCK_THREADS + threadIdx.x;
        const bool live = ei < n;
        const int es = live ? ei : n - 1;
#pragma unroll 1
        for (int j = 0; j < T; ++j) {
            padic_to_digit_form<E>(A, B, M, P.parts[j] + (size_t)es * P.ct_words, P.ct_words, P.kdig, P.nd, nm, nm1, n0inv);
#pragma unroll 1
            for (int c = 0; c < E::NC; ++c) { tbl(j, 0, c) = E::ld(A, c); tbl(j, 1, c) = E::ld(B, c); }
            wave_lds_fence();
        }
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            const unsigned members = (side ? P.neg_mask : ~P.neg_mask) & ((1u << T) - 1u);
            if (!members) continue;
            int top = 0;                                                  // highest set bit over the side's exponents
            for (int j = 0; j < T; ++j)
                if ((members >> j) & 1u)
                    for (int b = 32 * TCOMB_MU_WORDS - 1; b > top; --b)
                        if (mu_bit(j, b)) { top = b; break; }
            bool started = false;
#pragma unroll 1
            for (int bit = top; bit >= 0; --bit) {
                if (started) E::sqr_fused(A, B, nm, nm1, n0inv);
#pragma unroll 1
                for (int j = 0; j < T; ++j) {
                    if (!((members >> j) & 1u) || !mu_bit(j, bit)) continue;
                    if (!started) {
                        wave_lds_fence();
#pragma unroll 1
                        for (int c = 0; c < E::NC; ++c) { E::st(A, c, tbl(j, 0, c)); E::st(B, c, tbl(j, 1, c)); }
                        wave_lds_fence();
                        started = true;
                    } else {
                        E::mul_fused(A, B, from_table(j, 0), from_table(j, 1), nm, nm1, n0inv);
                    }
                }
            }
            // leave Montgomery form (times the plain pair (1, 0)), then w + v n as one integer, canonical (as k_ctmul_padic)
            uint32_t w[NL], v[NL];
            {
                auto one = [&](int blk, uint32_t (&xv)[U]) {
#pragma unroll
                    for (int u = 0; u < U; ++u) xv[u] = 0;
                    if (blk == 0) xv[0] = 1;
                };
                auto zero = [&](int blk, uint32_t (&xv)[U]) {
#pragma unroll
                    for (int u = 0; u < U; ++u) xv[u] = 0;
                };
                E::mm1_mul(w, M, A, one, nm, n0inv);
                E::mm2_mul(v, M, A, B, zero, one, nm, nm1, n0inv);
            }
            wave_lds_fence();
            E::store_digit(B, v);
            wave_lds_fence();
            uint32_t hi[NL];
            E::mul_plain(hi, A, w, B, [&](int blk, uint32_t (&xv)[U]) { E::digits_uniform(nm_lds, blk, xv); });
            wave_lds_fence();
            E::store_digit(B, hi);
            wave_lds_fence();
            cond_sub_2nl<E>(A, B, P.nsq);
            cond_sub_2nl<E>(A, B, P.nsq);
            if (live) {
                uint32_t* orow = (side ? out_neg : out_pos) + (size_t)ei * P.ct_words;
#pragma unroll 1
                for (int k = 0; k < P.ct_words; ++k) {
                    const int j0 = (32 * k) / RB, s0 = 32 * k - RB * j0;
                    uint64_t t = (uint64_t)lds_limb<E>(A, B, j0) >> s0;
                    t |= (uint64_t)lds_limb<E>(A, B, j0 + 1) << (RB - s0);
                    t |= (uint64_t)lds_limb<E>(A, B, j0 + 2) << (2 * RB - s0);
                    orow[k] = (uint32_t)t;
                }
            }
            wave_lds_fence();
        }
    }
}

// ---- m = ((x - 1) / n) theta mod n, with the test x = 1 (mod n) ------------------------------------------------------------------------
// One element per lane, word-serial.  x < n^2 in 2 W words.  Exact division digit by digit (Hensel): q_k = y_k n^-1 mod 2^32,
// y <- y - q_k n 2^(32 k) for k < W; n divides y = x - 1 with a quotient below 2^(32 W) exactly when y ends as 0 without a
// borrow out of the top — otherwise the row is flagged (bit 0 of *flag, rowflag[i] = 1).  Then one Montgomery product (CIOS) with
// thetaR = theta 2^(32 W) mod n and one conditional subtraction: the canonical residue.  A flagged row gets the product of its
// meaningless quotient: defined, never decoded.  About 2.5 W^2 multiply-adds per element.
template <int WMAX>
__global__ void __launch_bounds__(BLOCK_THREADS)
k_tfinish(const uint32_t* __restrict__ nw, const uint32_t* __restrict__ thetaR, int W, const uint32_t* __restrict__ x,
          uint32_t* __restrict__ m_out, int32_t* flag, int32_t* rowflag, int n) {
    const int i = blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t y[2 * WMAX + 2], u[WMAX];
    const uint32_t* xr = x + (size_t)i * 2 * W;
    uint32_t borrow = 1;
    for (int k = 0; k < 2 * W; ++k) {
        const uint32_t v = xr[k];
        y[k] = v - borrow;
        borrow &= (v == 0u) ? 1u : 0u;
    }
    bool bad = borrow != 0;                                   // x = 0
    const uint32_t n0 = nw[0];
    uint32_t inv = n0;                                        // n^-1 mod 2^32 (Newton: 3 correct bits double five times)
    for (int it = 0; it < 5; ++it) inv *= 2u - n0 * inv;
    for (int k = 0; k < W; ++k) {
        const uint32_t q = y[k] * inv;
        u[k] = q;
        uint64_t bw = 0;                                      // carry of q n plus the running borrow, at most 2^32
        for (int j = 0; j < W; ++j) {
            const uint64_t p = (uint64_t)q * nw[j] + bw;
            const uint32_t lo = (uint32_t)p, yv = y[k + j];
            y[k + j] = yv - lo;
            bw = (p >> 32) + (yv < lo ? 1u : 0u);
        }
        for (int j = k + W; j < 2 * W; ++j) {
            const uint32_t lo = (uint32_t)bw, yv = y[j];
            y[j] = yv - lo;
            bw = (bw >> 32) + (yv < lo ? 1u : 0u);
        }
        bad |= bw != 0;
    }
    for (int k = W; k < 2 * W; ++k) bad |= y[k] != 0;
    if (bad) {
        atomicOr(flag, 1);
        if (rowflag) rowflag[i] = 1;
    }
    // y <- u thetaR R^-1 mod n (CIOS), below 2 n in W + 1 words
    for (int k = 0; k < W + 2; ++k) y[k] = 0;
    const uint32_t nneg = 0u - inv;
    for (int k = 0; k < W; ++k) {
        const uint32_t b = u[k];
        uint64_t c = 0;
        for (int j = 0; j < W; ++j) {
            const uint64_t cur = (uint64_t)thetaR[j] * b + y[j] + c;
            y[j] = (uint32_t)cur;
            c = cur >> 32;
        }
        uint64_t cur = (uint64_t)y[W] + c;
        y[W] = (uint32_t)cur;
        y[W + 1] = (uint32_t)(cur >> 32);
        const uint32_t mm = y[0] * nneg;
        cur = (uint64_t)mm * n0 + y[0];
        c = cur >> 32;
        for (int j = 1; j < W; ++j) {
            cur = (uint64_t)mm * nw[j] + y[j] + c;
            y[j - 1] = (uint32_t)cur;
            c = cur >> 32;
        }
        cur = (uint64_t)y[W] + c;
        y[W - 1] = (uint32_t)cur;
        y[W] = y[W + 1] + (uint32_t)(cur >> 32);
    }
    uint32_t bw = 0;
    for (int j = 0; j < W; ++j) {
        const uint64_t d = (uint64_t)y[j] - nw[j] - bw;
        u[j] = (uint32_t)d;
        bw = (uint32_t)(d >> 63);
    }
    const bool ge = y[W] != 0 || bw == 0;
    uint32_t* orow = m_out + (size_t)i * W;
    for (int j = 0; j < W; ++j) orow[j] = ge ? u[j] : y[j];
}

}  // namespace pai
