// Batch verification of openings (pai_opening_fold): the one-digit fold modulo n.
//   k_open_fold   per chunk of <= P.chunk consecutive elements of one segment:
//                     B_chunk = prod_i r_i^(e_i) mod n       one Straus chain on the FIRST digit of Padic<NL, U> (mm1_mul / mm1_sqr)
//                     M_chunk = sum_i e_i m_i mod n          one product per element, lazy sum, one product by R^2 at the end
// Everything here is arithmetic modulo n (NL limbs), half the width of the digit-pair kernels of kernels_padic_enc.hpp: (r + k n)^n ==
// r^n (mod n^2), so the product of the r_i is only needed modulo n, and the full-width exponentiation by n happens once per segment.
// LDS: two digits per lane (A = the chain's accumulator, then the lazy sum; D = one operand), as k_smexp_padic's digit pair; the
// per-member power tables r_i^d R mod n, d = 1 .. 2^wbits - 1, live in handle scratch in [member][power][limb chunk][slot] order.
#pragma once
#include "geo_ops.hpp"
#include "kernels_padic_enc.hpp"
#include "launch.hpp"

namespace pai {

struct OpenFoldParams {
    const MontCtx* nctx;         // modulus n at NL limbs: n, R^2 mod n, R mod n, n0inv
    uint4* mscratch;             // [NC][nslots] quotient digits of the first-digit products
    uint4* table;                // [chunk][2^wbits - 1][NC][nslots]
    const int64_t* coff;         // [nlanes + 1] first element of every chunk (k_seg_chunk_expand)
    int n_words, ct_words;
    int chunk;                   // trip count of the member loops (wave-uniform)
    int e_words, ebits_max;
    int wbits;                   // window width of the B chain, 1 .. 4
};

// the plan rows of pai_opening_fold (both routes): segment starts off[s] = min(s L, N), s <= S, and the identity term list base[t] = t
static __global__ void __launch_bounds__(256)
k_open_plan(int64_t N, int64_t L, int S, int64_t* __restrict__ off, int32_t* __restrict__ base) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t s = i0; s <= S; s += stride) off[s] = s * L < N ? s * L : N;
    for (int64_t t = i0; t < N; t += stride) base[t] = (int32_t)t;
}
// out[i] = in[i] zero-extended from in_words to out_words (the composition route's r rows as residues modulo n^2)
static __global__ void __launch_bounds__(256)
k_open_widen(const uint32_t* __restrict__ in, int in_words, uint32_t* __restrict__ out, int out_words, size_t N) {
    const size_t total = N * (size_t)out_words;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / out_words;
        const int k = (int)(i - row * out_words);
        out[i] = k < in_words ? in[row * in_words + k] : 0u;
    }
}

// lane k: elements t in [coff[k], coff[k + 1]) of r [N][n_words], m [N][n_words], e [N][e_words];
// out_b [nlanes][ct_words] (canonical, zero-extended), out_m [nlanes][n_words] (canonical)
template <int NL, int U>
__global__ void __launch_bounds__(BLOCK_THREADS, 1)
k_open_fold(OpenFoldParams P, const uint32_t* __restrict__ r, const uint32_t* __restrict__ m, const uint32_t* __restrict__ e,
            uint32_t* __restrict__ out_b, uint32_t* __restrict__ out_m, int nlanes) {
    using E = Padic<NL, U, false>;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* ldsn = lds + (BLOCK_THREADS / 64) * 2 * E::DIGIT_WORDS;
    for (int i = threadIdx.x; i < NL; i += BLOCK_THREADS) {
        ldsn[i] = P.nctx->n[i];
        ldsn[NL + i] = P.nctx->r2[i];
        ldsn[2 * NL + i] = P.nctx->one[i];
    }
    __syncthreads();
    uint32_t sn[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) sn[j] = __builtin_amdgcn_readfirstlane(ldsn[j]);
    const uint32_t* nm = sn;
    const uint32_t* r2 = ldsn + NL;
    const uint32_t* one_m = ldsn + 2 * NL;
    const uint32_t n0inv = P.nctx->n0inv;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4* A = reinterpret_cast<uint4*>(lds + wave * 2 * E::DIGIT_WORDS) + lane;
    uint4* D = A + E::NC * 64;
    const size_t nslots = (size_t)gridDim.x * BLOCK_THREADS;
    const size_t slot = (size_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
    const typename E::MBuf M{P.mscratch + slot, nslots};
    const int W = P.wbits, NT = 1 << W, NP = NT - 1;
    const int nwin = (P.ebits_max + W - 1) / W;
    auto tbl = [&](int li, int d, int c) -> uint4& { return P.table[(((size_t)li * NP + (d - 1)) * E::NC + c) * nslots + slot]; };
    auto from_table = [&](int li, int d) {
        return [&, li, d](int blk, uint32_t (&xv)[U]) {
#pragma unroll
            for (int c = 0; c < E::UC; ++c) {
                const uint4 t = tbl(li, d, E::UC * blk + c);
                xv[4 * c] = t.x; xv[4 * c + 1] = t.y; xv[4 * c + 2] = t.z; xv[4 * c + 3] = t.w;
            }
        };
    };
    auto uniform = [&](const uint32_t* k) { return [=](int blk, uint32_t (&xv)[U]) { E::digits_uniform(k, blk, xv); }; };
    auto self = [&](const uint4* X) { return [=](int blk, uint32_t (&xv)[U]) { E::digits(X, blk, xv); }; };
    auto plain_one = [&](int blk, uint32_t (&xv)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = 0;
        if (blk == 0) xv[0] = 1;
    };
    auto put = [&](uint4* X, const uint32_t (&w)[NL]) {
        wave_lds_fence();
        E::store_digit(X, w);
        wave_lds_fence();
    };
    auto load_row = [&](uint4* X, const uint32_t* row, int words) {        // a packed row of `words` words as NL limbs
        wave_lds_fence();
#pragma unroll 1
        for (int c = 0; c < E::NC; ++c) {
            uint32_t t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = row_limb(row, words, 4 * c + k);
            E::st(X, c, make_uint4(t[0], t[1], t[2], t[3]));
        }
        wave_lds_fence();
    };
    // (X in LDS, zero in Y) -> packed row of `words` words
    auto store_row = [&](const uint4* X, const uint4* Y, uint32_t* orow, int words) {
#pragma unroll 1
        for (int k = 0; k < words; ++k) {
            const int j0 = (32 * k) / RB, s0 = 32 * k - RB * j0;
            uint64_t t = (uint64_t)lds_limb<E>(X, Y, j0) >> s0;
            t |= (uint64_t)lds_limb<E>(X, Y, j0 + 1) << (RB - s0);
            t |= (uint64_t)lds_limb<E>(X, Y, j0 + 2) << (2 * RB - s0);
            orow[k] = (uint32_t)t;
        }
    };
    const int tiles = (nlanes + BLOCK_THREADS - 1) / BLOCK_THREADS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int idx = tile * BLOCK_THREADS + threadIdx.x;
        const bool live = idx < nlanes;
        const long long t0 = live ? P.coff[idx] : 0, t1 = live ? P.coff[idx + 1] : 0;      // dead lanes: t0 == t1
        // ---- power tables: entry d of member li = r^d R mod n (lazy, < n (1 + 2^-18)); a lane without the member builds row 0's
        // (an empty chunk starts at N: no row of its own exists) and never multiplies by it
#pragma unroll 1
        for (int li = 0; li < P.chunk; ++li) {
            const long long t = t0 + li < t1 ? t0 + li : 0;
            load_row(A, r + (size_t)t * P.n_words, P.n_words);
            uint32_t w[NL];
            E::mm1_mul(w, M, A, uniform(r2), nm, n0inv);
#pragma unroll 1
            for (int d = 1;; ++d) {
#pragma unroll
                for (int c = 0; c < E::NC; ++c) tbl(li, d, c) = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
                if (d == NP) break;
                put(A, w);
                __threadfence();
                E::mm1_mul(w, M, A, from_table(li, 1), nm, n0inv);
            }
        }
        __threadfence();
        // ---- the B chain: acc = R mod n, per window W shared squarings and one table product per member
        wave_lds_fence();
#pragma unroll 1
        for (int c = 0; c < E::NC; ++c) E::st(A, c, make_uint4(one_m[4 * c], one_m[4 * c + 1], one_m[4 * c + 2], one_m[4 * c + 3]));
        wave_lds_fence();
        bool started = false;                         // wave-uniform: nothing but ones so far, squarings can be skipped
#pragma unroll 1
        for (int wi = nwin - 1; wi >= 0; --wi) {
            if (started) {
#pragma unroll 1
                for (int sq = 0; sq < W; ++sq) {
                    uint32_t w[NL];
                    if constexpr (NL <= 40) E::mm1_sqr(w, M, A, nm, n0inv);
                    else E::mm1_mul(w, M, A, self(A), nm, n0inv);
                    put(A, w);
                }
            }
            const int bit = wi * W, k = bit >> 5, sh = bit & 31;
#pragma unroll 1
            for (int li = 0; li < P.chunk; ++li) {
                const long long t = t0 + li;
                int d = 0;
                if (t < t1) {
                    const size_t eoff = (size_t)t * P.e_words;
                    uint64_t bits2 = k < P.e_words ? e[eoff + k] : 0u;
                    if (k + 1 < P.e_words) bits2 |= (uint64_t)e[eoff + k + 1] << 32;
                    d = (int)((uint32_t)(bits2 >> sh) & (uint32_t)(NT - 1));
                }
                if (__any(d != 0)) {
                    uint32_t w[NL];
                    E::mm1_mul(w, M, A, from_table(li, d ? d : 1), nm, n0inv);      // a lane with a zero window reads entry 1 and keeps its digit
                    wave_lds_fence();
                    if (d) E::store_digit(A, w);
                    wave_lds_fence();
                    started = true;
                }
            }
        }
        {   // leave Montgomery form, canonical, zero-extended to a ciphertext row
            uint32_t w[NL], z[NL];
            E::mm1_mul(w, M, A, plain_one, nm, n0inv);
            E::cond_sub(w, nm);
#pragma unroll
            for (int j = 0; j < NL; ++j) z[j] = 0;
            put(A, w);
            put(D, z);
            if (live) store_row(A, D, out_b + (size_t)idx * P.ct_words, P.ct_words);
        }
        // ---- the M sum: A = lazy sum of m_i e_i R^-1 mod n (< n (1 + (i + 1) 2^-18) after member i), D = the operand m_i
        {
            uint32_t z[NL];
#pragma unroll
            for (int j = 0; j < NL; ++j) z[j] = 0;
            put(A, z);
        }
#pragma unroll 1
        for (int li = 0; li < P.chunk; ++li) {
            const long long t = t0 + li;
            const bool has = t < t1;
            const long long ts = has ? t : 0;
            load_row(D, m + (size_t)ts * P.n_words, P.n_words);
            const uint32_t* erow = e + (size_t)ts * P.e_words;
            const int ew = P.e_words;
            uint32_t w[NL];
            E::mm1_mul(w, M, D, [&](int blk, uint32_t (&xv)[U]) {
#pragma unroll
                for (int u = 0; u < U; ++u) xv[u] = row_limb(erow, ew, U * blk + u);
            }, nm, n0inv);
            uint32_t acc[NL];
            E::load_digit(A, acc);
            uint32_t carry = 0;
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const uint32_t s = acc[j] + (has ? w[j] : 0u) + carry;
                acc[j] = s & RMASK;
                carry = s >> RB;
            }
            E::cond_sub(acc, nm);
            put(A, acc);
        }
        {
            uint32_t w[NL], z[NL];
            E::mm1_mul(w, M, A, uniform(r2), nm, n0inv);
            E::cond_sub(w, nm);
#pragma unroll
            for (int j = 0; j < NL; ++j) z[j] = 0;
            put(A, w);
            put(D, z);
            if (live) store_row(A, D, out_m + (size_t)idx * P.n_words, P.n_words);
        }
        wave_lds_fence();
    }
}

// launchers (open_fold_kernels.hip): false = no instantiation for this limb count
bool launch_open_fold(int nl, hipStream_t s, int grid, const OpenFoldParams& P, const uint32_t* r, const uint32_t* m, const uint32_t* e,
                      uint32_t* out_b, uint32_t* out_m, int nlanes);
size_t open_fold_table_bytes(int nl, int chunk, int wbits, size_t blocks);

}  // namespace pai
