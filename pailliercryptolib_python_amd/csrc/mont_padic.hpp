// Arithmetic modulo p^2 on base-p digit pairs — the engine behind CRT-decrypt stage A.
//
// An element x of Z/p^2 is kept in "Montgomery digit form": two integers (a, b), each of NL limbs of
// 29 bits (lazy: < 2p + eps, never canonicalised inside the exponentiation), with
//        a + b p  ==  x R   (mod p^2),        R = 2^(29 NL)  >>  p   (R/p >= 2^20).
// Product rule.  For (a, b) ~ x and (c, d) ~ y let
//        w  = (a c + m p) / R                     -- Montgomery product mod p, quotient digits m
//        v  = (a d + b c - m + R p + m' p) / R    -- second Montgomery reduction mod p, quotient m'
// then  w + v p == (a + b p)(c + d p) R^-1 (mod p^2), i.e. (w, v) ~ x y.   Proof: a c = R w - m p and
// R v = a d + b c - m + (R + m') p, hence (a + b p)(c + d p) == a c + (a d + b c) p == R w + R v p.
// The b d p^2 term vanishes and every reduction is modulo p (NL limbs) instead of p^2 (2 NL limbs):
// a multiplication costs 5 NL^2 limb products instead of 8 NL^2, a squaring (every limb pair of a^2
// once, 2 a b once) 3.5 NL^2 instead of ~6.7 NL^2.  There is no division anywhere: the input is
// brought into digit form by applying the rule to its base-R digits and host-precomputed digit
// pairs of R^(i+2) mod p^2, and at the end the second digit of x^(p-1) IS Paillier's L function.
//
// Layout: one element per lane; the digit pair lives in LDS (chunk-major, see mont_wide.hpp); the
// accumulator window (NL + U lazy 64-bit columns, U = 12), the quotient digits m and the first
// result digit w live in VGPRs; p and p - 1 are wave-uniform (scalar loads).
#pragma once
#include "mont_dev.hpp"


namespace pai {

// XLDS: digit-buffer accesses through LDS-qualified pointers instead of leaving it to address-space inference.  One
// kernel shape (wide digits with quotient digits in scratch) otherwise compiles digit accesses to flat_load /
// flat_store; measured per kernel: 72-limb decrypt 364 -> 324 ms with it, 36-limb decrypt 476 -> 490 and 72-limb
// encrypt 67 -> 70 ms — hence a per-kernel switch.
template <int NL, int U, bool XLDS = false>
struct Padic {
    static_assert(NL % 4 == 0 && U % 4 == 0 && NL % U == 0 && U <= 16, "geometry");
    static constexpr int NC = NL / 4;        // four-limb chunks per digit
    static constexpr int UC = U / 4;         // chunks per row block
    static constexpr int NB = NL / U;        // row blocks
    static constexpr int NW = NL + U;        // accumulator window
    static constexpr int DIGIT_WORDS = NL * 64;   // LDS words of one digit for one wave
    static constexpr int P1 = (24 / U) * U;       // rows between normalisations at 2^59 per row
    static constexpr int P2 = (16 / U) * U;       // ... at 1.5 * 2^59 per row (doubled or three products)

    typedef uint32_t v4u_ __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) v4u_ lds_v4u_;
    PAI_DEV static uint4 ld(const uint4* x, int c) {
        if constexpr (XLDS) {
            const v4u_ v = *((const lds_v4u_*)(x + c * 64));
            return make_uint4(v.x, v.y, v.z, v.w);
        } else {
            return x[c * 64];
        }
    }
    PAI_DEV static void st(uint4* x, int c, uint4 v) {
        if constexpr (XLDS) {
            v4u_ t;
            t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
            *((lds_v4u_*)(x + c * 64)) = t;
        } else {
            x[c * 64] = v;
        }
    }

    PAI_DEV static void zero(uint64_t (&acc)[NW]) {
#pragma unroll
        for (int j = 0; j < NW; ++j) acc[j] = 0;
    }
    PAI_DEV static void normalize(uint64_t (&acc)[NW]) {
#pragma unroll
        for (int j = NW - 1; j >= 1; --j) {
            const uint64_t keep = (j == NW - 1) ? acc[j] : (acc[j] & RMASK);
            acc[j] = keep + (acc[j - 1] >> RB);
        }
        acc[0] &= RMASK;
    }
    PAI_DEV static void slide(uint64_t (&acc)[NW]) {
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[j] = acc[j + U];
#pragma unroll
        for (int j = NL; j < NW; ++j) acc[j] = 0;
    }
    // U digits of an LDS operand for row block `blk`
    PAI_DEV static void digits(const uint4* x, int blk, uint32_t (&v)[U]) {
#pragma unroll
        for (int c = 0; c < UC; ++c) {
            const uint4 t = ld(x, UC * blk + c);
            v[4 * c] = t.x; v[4 * c + 1] = t.y; v[4 * c + 2] = t.z; v[4 * c + 3] = t.w;
        }
    }
    PAI_DEV static void digits_uniform(const uint32_t* __restrict__ k, int blk, uint32_t (&v)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = k[U * blk + u];
    }

    // One block of U rows:  acc += X * xv  (limbs of X below LO skipped, limbs >= HI taken twice)
    //                           (+ Y * yv)  + p * q ,  then the window slides by U columns.
    // q receives the block's quotient digits.  FEED: U limbs of a constant enter at the window top.
    // SYM (squaring, xv = limbs LO .. HI-1 of X itself): inside the diagonal class [LO, HI) the pair
    // (limb LO + d, row u) is taken once — skipped for d < u, single for d == u, doubled for d > u.
    template <bool HAS_X, int LO, int HI, bool HAS_Y, bool FEED, bool SYM = false>
    PAI_DEV static void block(uint64_t (&acc)[NW], const uint4* X, const uint32_t (&xv)[U], const uint4* Y,
                              const uint32_t (&yv)[U], const uint32_t* __restrict__ nm, uint32_t n0inv,
                              const uint32_t* __restrict__ feed, int blk, uint32_t (&q)[U]) {
        uint32_t xv2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv2[u] = xv[u] << 1;
        if constexpr (FEED) {
#pragma unroll
            for (int u = 0; u < U; ++u) acc[NL + u] += feed[U * blk + u];
        }
        // low U limbs of the operands (the quotient chain needs them)
        uint32_t x0[U], y0[U];
#pragma unroll
        for (int c = 0; c < UC; ++c) {
            if (HAS_X && LO < 4 * (c + 1)) {
                const uint4 t = ld(X, c);
                x0[4 * c] = t.x; x0[4 * c + 1] = t.y; x0[4 * c + 2] = t.z; x0[4 * c + 3] = t.w;
            } else {
                x0[4 * c] = x0[4 * c + 1] = x0[4 * c + 2] = x0[4 * c + 3] = 0;
            }
            if constexpr (HAS_Y) {
                const uint4 t = ld(Y, c);
                y0[4 * c] = t.x; y0[4 * c + 1] = t.y; y0[4 * c + 2] = t.z; y0[4 * c + 3] = t.w;
            } else {
                y0[4 * c] = y0[4 * c + 1] = y0[4 * c + 2] = y0[4 * c + 3] = 0;
            }
        }
        // multiplicity of the product (limb j of X) * (row u): 0, 1 or 2
        auto xmult = [](int j, int u) -> int {
            if (!HAS_X || j < LO) return 0;
            if (j >= HI) return 2;
            if (!SYM) return 1;
            return (j - LO < u) ? 0 : (j - LO == u ? 1 : 2);
        };
        auto xterm = [&](int j, int u) -> uint64_t {           // contribution of limb j (< U) of X in row u
            const int k = xmult(j, u);
            return k == 0 ? 0 : (uint64_t)x0[j] * (k == 2 ? xv2[u] : xv[u]);
        };
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j <= u; ++j) {
                if (xmult(j, u - j)) acc[u] += xterm(j, u - j);
                if constexpr (HAS_Y) acc[u] += (uint64_t)y0[j] * yv[u - j];
            }
#pragma unroll
            for (int j = 1; j <= u; ++j) acc[u] += (uint64_t)nm[j] * q[u - j];
            q[u] = ((uint32_t)acc[u] * n0inv) & RMASK;
            acc[u] += (uint64_t)nm[0] * q[u];
            acc[u + 1] += acc[u] >> RB;
        }
#pragma unroll
        for (int j = 1; j < U; ++j) {
#pragma unroll
            for (int u = U - j; u < U; ++u) {
                if (xmult(j, u)) acc[j + u] += xterm(j, u);
                if constexpr (HAS_Y) acc[j + u] += (uint64_t)y0[j] * yv[u];
                acc[j + u] += (uint64_t)nm[j] * q[u];
            }
        }
        // remaining chunks: a pure rank-(2U or 3U) update
        if constexpr (NL <= 48) {
#pragma unroll
            for (int c = UC; c < NC; ++c) {
                uint32_t xa[4] = {0, 0, 0, 0}, ya[4] = {0, 0, 0, 0};
                if constexpr (HAS_X) {
                    if (4 * c >= LO) { const uint4 t = ld(X, c); xa[0] = t.x; xa[1] = t.y; xa[2] = t.z; xa[3] = t.w; }
                }
                if constexpr (HAS_Y) { const uint4 t = ld(Y, c); ya[0] = t.x; ya[1] = t.y; ya[2] = t.z; ya[3] = t.w; }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int mult = xmult(4 * c + k, u);
                        if (mult) acc[4 * c + k + u] += (uint64_t)xa[k] * (mult == 2 ? xv2[u] : xv[u]);
                        if constexpr (HAS_Y) acc[4 * c + k + u] += (uint64_t)ya[k] * yv[u];
                        acc[4 * c + k + u] += (uint64_t)nm[4 * c + k] * q[u];
                    }
                }
            }
        } else {
            // wide windows (NL = 72): stream the operands one chunk ahead and fence the scheduler per chunk so
            // that the chunk loads are not all hoisted to the top (which would spill the accumulator window)
            __builtin_amdgcn_sched_barrier(0);
            uint4 x_cur = ld(X, UC), y_cur = ld(Y, UC);
            uint32_t n_cur[4] = {nm[4 * UC], nm[4 * UC + 1], nm[4 * UC + 2], nm[4 * UC + 3]};
#pragma unroll
            for (int c = UC; c < NC; ++c) {
                const int cn = (c + 1 < NC) ? c + 1 : c;
                const uint4 x_nxt = ld(X, cn), y_nxt = ld(Y, cn);
                const uint32_t n_nxt[4] = {nm[4 * cn], nm[4 * cn + 1], nm[4 * cn + 2], nm[4 * cn + 3]};
                const uint32_t xa[4] = {x_cur.x, x_cur.y, x_cur.z, x_cur.w};
                const uint32_t ya[4] = {y_cur.x, y_cur.y, y_cur.z, y_cur.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int mult = xmult(4 * c + k, u);
                        if (mult) acc[4 * c + k + u] += (uint64_t)xa[k] * (mult == 2 ? xv2[u] : xv[u]);
                        if constexpr (HAS_Y) acc[4 * c + k + u] += (uint64_t)ya[k] * yv[u];
                        acc[4 * c + k + u] += (uint64_t)n_cur[k] * q[u];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                x_cur = x_nxt;
                y_cur = y_nxt;
#pragma unroll
                for (int k = 0; k < 4; ++k) n_cur[k] = n_nxt[k];
            }
        }
        slide(acc);
    }

    // carry-propagate the low NL columns into canonical 29-bit limbs (registers)
    PAI_DEV static void finish(const uint64_t (&acc)[NW], uint32_t (&r)[NL]) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const uint64_t t = acc[j] + c;
            r[j] = (uint32_t)t & RMASK;
            c = t >> RB;
        }
    }
    PAI_DEV static void store_digit(uint4* x, const uint32_t (&r)[NL]) {
#pragma unroll
        for (int c = 0; c < NC; ++c) st(x, c, make_uint4(r[4 * c], r[4 * c + 1], r[4 * c + 2], r[4 * c + 3]));
    }

    // ---- first half of the product rule: w = (X * C + m p) / R, quotient digits m -----------------
    // CSrc: functor (blk, xv) giving the U digits of C for a row block.
    // The quotient digits m are parked in LDS (digit buffer M) so that the row-block loop can stay rolled
    // (a rolled loop cannot index a register array) — the hot loop must fit the 64 KB instruction cache.
    // M may be an LDS digit buffer (stride 64 uint4) or a global scratch column (stride = number of slots)
    struct MBuf {
        uint4* p;
        size_t stride;
    };
    PAI_DEV static void store_q(MBuf M, int blk, const uint32_t (&q)[U]) {
#pragma unroll
        for (int c = 0; c < UC; ++c)
            M.p[(size_t)(UC * blk + c) * M.stride] = make_uint4(q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]);
    }
    template <class CSrc>
    PAI_DEV static void mm1_mul(uint32_t (&w)[NL], MBuf M, const uint4* X, CSrc&& csrc,
                                const uint32_t* __restrict__ nm, uint32_t n0inv) {
        uint64_t acc[NW];
        zero(acc);
        uint32_t dummy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dummy[u] = 0;
        // the digits of the next row block are fetched while the current block is computed (they may come
        // from global memory: table entries)
        uint32_t xn[U];
        csrc(0, xn);
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t xv[U], q[U];
#pragma unroll
            for (int u = 0; u < U; ++u) xv[u] = xn[u];
            csrc(blk + 1 < NB ? blk + 1 : blk, xn);
            block<true, 0, NL, false, false>(acc, X, xv, X, dummy, nm, n0inv, nm, blk, q);
            store_q(M, blk, q);
            if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) normalize(acc);    // 2^59 per row: at most 24 rows
        }
        finish(acc, w);
    }
    // squaring: C = X, symmetric by limb classes of U limbs (row block b multiplies limbs >= U b)
    // Column bound: a column of X^2 holds at most NL/2 doubled pairs (2^59 each) and one square over the WHOLE
    // pass, plus one p*q product (2^58) per row.  For NL <= 40 a single normalisation after about half the rows
    // keeps both halves below 2^64: (NL/2 + 1/2) 2^59 + r 2^58 < 2^64 for r <= 24.  Wider digits use the
    // per-row rule (1.5 * 2^59 per row, at most 16 rows).
    PAI_DEV static constexpr bool sqr1_normalize_after(int B) {
        if (B == NB - 1) return false;
        if (NL <= 40) return (B + 1) * U <= 24 && (B + 2) * U > 24;
        return ((B + 1) * U) % P2 == 0;
    }
    template <int B>
    PAI_DEV static void mm1_sqr_blocks(uint64_t (&acc)[NW], MBuf M, const uint4* X,
                                       const uint32_t* __restrict__ nm, uint32_t n0inv) {
        if constexpr (B < NB) {
            uint32_t xv[U], q[U], dummy[U];
#pragma unroll
            for (int u = 0; u < U; ++u) dummy[u] = 0;
            digits(X, B, xv);
            block<true, U * B, U * (B + 1), false, false, true>(acc, X, xv, X, dummy, nm, n0inv, nm, B, q);
            store_q(M, B, q);
            if (sqr1_normalize_after(B)) normalize(acc);
            mm1_sqr_blocks<B + 1>(acc, M, X, nm, n0inv);
        }
    }
    PAI_DEV static void mm1_sqr(uint32_t (&w)[NL], MBuf M, const uint4* X,
                                const uint32_t* __restrict__ nm, uint32_t n0inv) {
        uint64_t acc[NW];
        zero(acc);
        mm1_sqr_blocks<0>(acc, M, X, nm, n0inv);
        finish(acc, w);
    }

    // ---- second half: v = (X * D + Y * C - m + R p + m' p) / R --------------------------------------
    // initial window = (R - 1 - m) + 1 in the low NL columns; p - 1 enters at the top (pm1 = limbs of p - 1)
    PAI_DEV static void mm2_init(uint64_t (&acc)[NW], MBuf M) {
        wave_lds_fence();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint4 t = M.p[(size_t)c * M.stride];
            acc[4 * c] = (uint64_t)(RMASK - t.x); acc[4 * c + 1] = (uint64_t)(RMASK - t.y);
            acc[4 * c + 2] = (uint64_t)(RMASK - t.z); acc[4 * c + 3] = (uint64_t)(RMASK - t.w);
        }
        acc[0] += 1;
#pragma unroll
        for (int j = NL; j < NW; ++j) acc[j] = 0;
    }
    template <class DSrc, class CSrc>
    PAI_DEV static void mm2_mul(uint32_t (&v)[NL], MBuf M, const uint4* X, const uint4* Y, DSrc&& dsrc,
                                CSrc&& csrc, const uint32_t* __restrict__ nm, const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        uint64_t acc[NW];
        uint32_t xn[U], yn[U];
        dsrc(0, xn);
        csrc(0, yn);
        mm2_init(acc, M);
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t xv[U], yv[U], q[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { xv[u] = xn[u]; yv[u] = yn[u]; }
            dsrc(blk + 1 < NB ? blk + 1 : blk, xn);
            csrc(blk + 1 < NB ? blk + 1 : blk, yn);
            block<true, 0, NL, true, true>(acc, X, xv, Y, yv, nm, n0inv, pm1, blk, q);
            if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc);     // 1.5 * 2^59 per row: at most 16 rows
        }
        finish(acc, v);
    }
    // squaring: v = (2 X * Y - m + R p + m' p) / R   (X = first digit, Y = second digit of the same element)
    PAI_DEV static void mm2_sqr(uint32_t (&v)[NL], MBuf M, const uint4* X, const uint4* Y,
                                const uint32_t* __restrict__ nm, const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        uint64_t acc[NW];
        mm2_init(acc, M);
        uint32_t dummy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dummy[u] = 0;
        // unrolled (three 12-row blocks at 36 limbs): 2 % faster inside the decrypt kernel (476 vs 486 ms); unrolling the
        // product's loops as well overflows the instruction cache (511 ms)
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t xv[U], q[U];
            digits(Y, blk, xv);
            block<true, 0, 0, false, true>(acc, X, xv, X, dummy, nm, n0inv, pm1, blk, q);   // HI = 0: every limb doubled
            if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc);
        }
        finish(acc, v);
    }

    // Variant for wide digits (NL = 72): the first result digit w is parked in a strided scratch buffer (same
    // shape as M) instead of 72 registers, so that nothing but the accumulator window is live inside the loops.
    PAI_DEV static void finish_to_buf(const uint64_t (&acc)[NW], MBuf Wb) {
        uint64_t c = 0;
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t t = acc[4 * ch + k] + c;
                w[k] = (uint32_t)t & RMASK;
                c = t >> RB;
            }
            Wb.p[(size_t)ch * Wb.stride] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    template <class CSrc, class DSrc>
    PAI_DEV static void mul_wbuf(uint4* A, uint4* B, MBuf M, MBuf Wb, CSrc&& csrc, DSrc&& dsrc,
                                 const uint32_t* __restrict__ nm, const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        {   // first half: w -> Wb, quotient digits -> M
            uint64_t acc[NW];
            zero(acc);
            uint32_t dummy[U];
#pragma unroll
            for (int u = 0; u < U; ++u) dummy[u] = 0;
            uint32_t xn[U];
            csrc(0, xn);
#pragma unroll 1
            for (int blk = 0; blk < NB; ++blk) {
                uint32_t xv[U], q[U];
#pragma unroll
                for (int u = 0; u < U; ++u) xv[u] = xn[u];
                csrc(blk + 1 < NB ? blk + 1 : blk, xn);
                block<true, 0, NL, false, false>(acc, A, xv, A, dummy, nm, n0inv, nm, blk, q);
                store_q(M, blk, q);
                if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) normalize(acc);
            }
            finish_to_buf(acc, Wb);
        }
        __builtin_amdgcn_sched_barrier(0);
        {   // second half: v -> B (after the last read of B), then w -> A
            uint64_t acc[NW];
            uint32_t xn[U], yn[U];
            dsrc(0, xn);
            csrc(0, yn);
            mm2_init(acc, M);
#pragma unroll 1
            for (int blk = 0; blk < NB; ++blk) {
                uint32_t xv[U], yv[U], q[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { xv[u] = xn[u]; yv[u] = yn[u]; }
                dsrc(blk + 1 < NB ? blk + 1 : blk, xn);
                csrc(blk + 1 < NB ? blk + 1 : blk, yn);
                block<true, 0, NL, true, true>(acc, A, xv, B, yv, nm, n0inv, pm1, blk, q);
                if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc);
            }
            wave_lds_fence();
            uint64_t c = 0;
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint64_t t = acc[4 * ch + k] + c;
                    w[k] = (uint32_t)t & RMASK;
                    c = t >> RB;
                }
                st(B, ch, make_uint4(w[0], w[1], w[2], w[3]));
                st(A, ch, Wb.p[(size_t)ch * Wb.stride]);
            }
            wave_lds_fence();
        }
    }

    // second result digit over B, the parked first digit back from the scratch column over A
    PAI_DEV static void finish_into(const uint64_t (&acc)[NW], uint4* Bdst, uint4* Adst, MBuf Wb) {
        uint64_t c = 0;
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t t = acc[4 * ch + k] + c;
                w[k] = (uint32_t)t & RMASK;
                c = t >> RB;
            }
            st(Bdst, ch, make_uint4(w[0], w[1], w[2], w[3]));
            st(Adst, ch, Wb.p[(size_t)ch * Wb.stride]);
        }
    }

    // Squaring for wide digits with BOTH halves in rolled loops (nothing to overflow the instruction cache): the first
    // half is the product loop with the element's own first digit as multiplier (a * a, every limb pair twice — the
    // limb-class symmetric first half is fully unrolled code), the second half is the squaring's own
    // v = (2 a b - m + R p + m' p) / R with doubled multiplier digits: ONE pass over a instead of the two (a d + b c)
    // of the product rule.  4 NL^2 limb products per squaring instead of the 5 NL^2 of mul_wbuf(x, x).
    PAI_DEV static void sqr_rolled_wbuf(uint4* A, uint4* B, MBuf M, MBuf Wb, const uint32_t* __restrict__ nm,
                                        const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        {
            uint64_t acc[NW];
            zero(acc);
            uint32_t dummy[U];
#pragma unroll
            for (int u = 0; u < U; ++u) dummy[u] = 0;
            uint32_t xn[U];
            digits(A, 0, xn);
#pragma unroll 1
            for (int blk = 0; blk < NB; ++blk) {
                uint32_t xv[U], q[U];
#pragma unroll
                for (int u = 0; u < U; ++u) xv[u] = xn[u];
                digits(A, blk + 1 < NB ? blk + 1 : blk, xn);
                block<true, 0, NL, false, false>(acc, A, xv, A, dummy, nm, n0inv, nm, blk, q);
                store_q(M, blk, q);
                if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) normalize(acc);
            }
            finish_to_buf(acc, Wb);
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            uint64_t acc[NW];
            mm2_init(acc, M);
            uint32_t dummy[U];
#pragma unroll
            for (int u = 0; u < U; ++u) dummy[u] = 0;
#pragma unroll 1
            for (int blk = 0; blk < NB; ++blk) {
                uint32_t xv[U], q[U];
                digits(B, blk, xv);
                block<true, 0, 0, false, true>(acc, A, xv, A, dummy, nm, n0inv, pm1, blk, q);   // HI = 0: every limb doubled
                if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc);
            }
            wave_lds_fence();
            finish_into(acc, B, A, Wb);
            wave_lds_fence();
        }
    }

    // The same with a limb-class symmetric first half that still fits the instruction cache: per row block, the
    // a-part (the element's own limbs >= U b against its digits of class b: diagonal class once per pair, classes above
    // doubled) is one of NB specialised straight-line routines selected by a wave-uniform switch — NL (NL + U) / 2 limb
    // products of code in total — and the reduction part (quotient chain and p * q, identical for every block) is the
    // shared rolled body.  3.5 NL^2 limb products per squaring.
    template <int B>
    PAI_DEV static void sqr_apart(uint64_t (&acc)[NW], const uint4* X, const uint32_t (&xv)[U]) {
        constexpr int LO = U * B, HI = U * (B + 1);
        uint32_t xv2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv2[u] = xv[u] << 1;
#pragma unroll
        for (int c = LO / 4; c < NC; ++c) {
            const uint4 t = ld(X, c);
            const uint32_t xa[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * c + k;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int mult = j >= HI ? 2 : (j - LO < u ? 0 : (j - LO == u ? 1 : 2));
                    if (mult) acc[j + u] += (uint64_t)xa[k] * (mult == 2 ? xv2[u] : xv[u]);
                }
            }
        }
    }
    template <int B>
    PAI_DEV static void sqr_apart_dispatch(uint64_t (&acc)[NW], const uint4* X, const uint32_t (&xv)[U], int blk) {
        if (blk == B) sqr_apart<B>(acc, X, xv);
        else if constexpr (B + 1 < NB) sqr_apart_dispatch<B + 1>(acc, X, xv, blk);
    }

    // ---- both halves of the product rule in ONE pass over the row blocks -------------------------------------------
    // Row block k of the first half produces the quotient digits m[U k .. U k + U) — exactly the columns the second
    // half's window starts at in ITS row block k — so the two accumulator windows advance together: the quotient digits
    // go from registers straight into the second window as (2^29 - 1 - m_j) and never exist as a stored number, and the
    // first result digit w stays in its window until v is finished as well, so nothing is parked either.  Wide digits
    // (NL = 56 / 72) otherwise bounce both through strided HBM scratch (MBuf): 2 NL limbs written and read per product.
    // Price: two windows of NL + U lazy columns live at once (4 (NL + U) VGPRs; one wave per SIMD has 512).
    PAI_DEV static void finish_pair(const uint64_t (&acc1)[NW], const uint64_t (&acc2)[NW], uint4* Adst, uint4* Bdst) {
        uint64_t c1 = 0, c2 = 0;
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            uint32_t w[4], v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t t1 = acc1[4 * ch + k] + c1;
                w[k] = (uint32_t)t1 & RMASK;
                c1 = t1 >> RB;
                const uint64_t t2 = acc2[4 * ch + k] + c2;
                v[k] = (uint32_t)t2 & RMASK;
                c2 = t2 >> RB;
            }
            st(Adst, ch, make_uint4(w[0], w[1], w[2], w[3]));
            st(Bdst, ch, make_uint4(v[0], v[1], v[2], v[3]));
        }
    }
    template <class CSrc, class DSrc>
    PAI_DEV static void mul_fused(uint4* A, uint4* B, CSrc&& csrc, DSrc&& dsrc, const uint32_t* __restrict__ nm,
                                  const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        uint64_t acc1[NW], acc2[NW];
        zero(acc1);
        zero(acc2);
        acc2[0] = 1;                          // (R - 1 - m) + 1
        uint32_t dummy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dummy[u] = 0;
        uint32_t cn[U], dn[U];
        csrc(0, cn);
        dsrc(0, dn);
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t cv[U], dv[U], q1[U], q2[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { cv[u] = cn[u]; dv[u] = dn[u]; }
            csrc(blk + 1 < NB ? blk + 1 : blk, cn);
            dsrc(blk + 1 < NB ? blk + 1 : blk, dn);
            block<true, 0, NL, false, false>(acc1, A, cv, A, dummy, nm, n0inv, nm, blk, q1);
#pragma unroll
            for (int u = 0; u < U; ++u) acc2[u] += (uint64_t)(RMASK - q1[u]);
            block<true, 0, NL, true, true>(acc2, A, dv, B, cv, nm, n0inv, pm1, blk, q2);
            if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) normalize(acc1);
            if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc2);
        }
        wave_lds_fence();
        finish_pair(acc1, acc2, A, B);
        wave_lds_fence();
    }
    // (A, B) <- (A, B) * (C, 0): the product rule with a right operand whose SECOND digit is zero — w = (a c + m p) / R,
    // v = (b c - m + R p + m' p) / R: 4 NL^2 limb products instead of 5.  The fixed-base tables store such operands
    // (g-factored entries, kernels_padic_enc.hpp): x = (c, 0) * (1 + p)^t with the exponents t summed on the side.
    template <class CSrc>
    PAI_DEV static void mul_fused_c0(uint4* A, uint4* B, CSrc&& csrc, const uint32_t* __restrict__ nm,
                                     const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        uint64_t acc1[NW], acc2[NW];
        zero(acc1);
        zero(acc2);
        acc2[0] = 1;                          // (R - 1 - m) + 1
        uint32_t dummy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dummy[u] = 0;
        uint32_t cn[U];
        csrc(0, cn);
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t cv[U], q1[U], q2[U];
#pragma unroll
            for (int u = 0; u < U; ++u) cv[u] = cn[u];
            csrc(blk + 1 < NB ? blk + 1 : blk, cn);
            block<true, 0, NL, false, false>(acc1, A, cv, A, dummy, nm, n0inv, nm, blk, q1);
#pragma unroll
            for (int u = 0; u < U; ++u) acc2[u] += (uint64_t)(RMASK - q1[u]);
            block<false, 0, NL, true, true>(acc2, A, dummy, B, cv, nm, n0inv, pm1, blk, q2);
            if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) { normalize(acc1); normalize(acc2); }   // two products per row and column each
        }
        wave_lds_fence();
        finish_pair(acc1, acc2, A, B);
        wave_lds_fence();
    }
    // squaring: first half a * a (every limb pair twice), second half 2 a b with doubled multiplier digits — 4 NL^2
    PAI_DEV static void sqr_fused(uint4* A, uint4* B, const uint32_t* __restrict__ nm, const uint32_t* __restrict__ pm1,
                                  uint32_t n0inv) {
        uint64_t acc1[NW], acc2[NW];
        zero(acc1);
        zero(acc2);
        acc2[0] = 1;
        uint32_t dummy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dummy[u] = 0;
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t av[U], bv[U], q1[U], q2[U];
            digits(A, blk, av);
            digits(B, blk, bv);
            block<true, 0, NL, false, false>(acc1, A, av, A, dummy, nm, n0inv, nm, blk, q1);
#pragma unroll
            for (int u = 0; u < U; ++u) acc2[u] += (uint64_t)(RMASK - q1[u]);
            block<true, 0, 0, false, true>(acc2, A, bv, A, dummy, nm, n0inv, pm1, blk, q2);   // HI = 0: every limb doubled
            if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) normalize(acc1);
            if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc2);
        }
        wave_lds_fence();
        finish_pair(acc1, acc2, A, B);
        wave_lds_fence();
    }

    // fused counterpart of sqr_sym_wbuf: limb-class symmetric first half (3.5 NL^2)
    PAI_DEV static void sqr_sym_fused(uint4* A, uint4* B, const uint32_t* __restrict__ nm, const uint32_t* __restrict__ pm1,
                                      uint32_t n0inv) {
        uint64_t acc1[NW], acc2[NW];
        zero(acc1);
        zero(acc2);
        acc2[0] = 1;
        uint32_t dummy[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dummy[u] = 0;
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t av[U], bv[U], q1[U], q2[U];
            digits(A, blk, av);
            digits(B, blk, bv);
            sqr_apart_dispatch<0>(acc1, A, av, blk);
            __builtin_amdgcn_sched_barrier(0);
            block<false, 0, NL, false, false>(acc1, A, dummy, A, dummy, nm, n0inv, nm, blk, q1);
#pragma unroll
            for (int u = 0; u < U; ++u) acc2[u] += (uint64_t)(RMASK - q1[u]);
            block<true, 0, 0, false, true>(acc2, A, bv, A, dummy, nm, n0inv, pm1, blk, q2);
            if (sqr1_normalize_after(blk)) normalize(acc1);
            if (blk != NB - 1 && ((blk + 1) * U) % P2 == 0) normalize(acc2);
        }
        wave_lds_fence();
        finish_pair(acc1, acc2, A, B);
        wave_lds_fence();
    }
    // compile-time choice between the scratch-parked and the fused forms (per kernel: the fused form trades the scratch
    // round trips for register pressure)
    template <bool FUSED, class CSrc, class DSrc>
    PAI_DEV static void mul_w(uint4* A, uint4* B, MBuf M, MBuf Wb, CSrc&& csrc, DSrc&& dsrc, const uint32_t* __restrict__ nm,
                              const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        if constexpr (FUSED) mul_fused(A, B, csrc, dsrc, nm, pm1, n0inv);
        else mul_wbuf(A, B, M, Wb, csrc, dsrc, nm, pm1, n0inv);
    }
    template <bool FUSED>
    PAI_DEV static void sqr_rolled_w(uint4* A, uint4* B, MBuf M, MBuf Wb, const uint32_t* __restrict__ nm,
                                     const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        if constexpr (FUSED) sqr_fused(A, B, nm, pm1, n0inv);
        else sqr_rolled_wbuf(A, B, M, Wb, nm, pm1, n0inv);
    }

    // (A, B) <- (A, B)^2
    PAI_DEV static void sqr(uint4* A, uint4* B, MBuf M, const uint32_t* __restrict__ nm, const uint32_t* __restrict__ pm1,
                            uint32_t n0inv) {
        uint32_t w[NL], v[NL];
        mm1_sqr(w, M, A, nm, n0inv);
        mm2_sqr(v, M, A, B, nm, pm1, n0inv);
        wave_lds_fence();
        store_digit(A, w);
        store_digit(B, v);
        wave_lds_fence();
    }
    // ---- (A, B) <- (A, B)^2 in registers, product columns by signed Karatsuba (NL even) --------------------------------
    // Both digits are split at H = NL / 2 limbs, x = x0 + x1 B^H, y = y0 + y1 B^H (B = 2^29), and the limb-product column
    // k of x y is assembled from three half-size coefficient vectors
    //     X_k = P0_k + (P0 + P2 - D)_(k-H) + P2_(k-2H),   P0 = x0 y0,  P2 = x1 y1,  D = (x0 - x1)(y0 - y1),
    // 3 H^2 limb products instead of NL^2 (3 H (H + 1) / 2 instead of NL (NL + 1) / 2 for a square).  The differences are
    // 32-bit signed limbs in (-2^29, 2^29) and D is accumulated by signed multiply-adds: every partial sum is exact modulo
    // 2^64 and X_k itself, the schoolbook column (at most NL products < 2^58), lies in [0, 2^64) — no carries, no
    // normalisation.  P0_j is used at columns j and j + H, P2_j at j + H and j + 2H: each is computed once, at its
    // first use, and stays live for H columns.
    // The columns are consumed in order by the fused Montgomery reduction (as the product-scanning squaring of round 4):
    // the product column goes through a carry stream of its own (cc) and only its low 29 bits, doubled for 2 a b, enter
    // the reduction column with the quotient products, so neither 64-bit sum can wrap:  cc <= 2^63.2 + 2^35 and
    // d <= NL 2^58 + 2^36 + 2^30.
    // FORM (compile time):
    //   KARA_SQR   w = (x^2 + m p) / R, quotient digits to mq (y = x; pairs i < l doubled, the diagonal once).
    //   KARA_SQR2  v = (2 x y - min + R p + m' p) / R: the low 29 bits of the product stream enter doubled.
    //   KARA_MUL   w = (x y + m p) / R with x != y, not doubled, quotient digits to mq.
    //   KARA_MUL2  v = (x y + x2 y2 - min + R p + m' p) / R, the SUM of two products (a d + b c of the product rule).
    // (R p - min = (R - 1 - min) + 1 + (p - 1) R; p - 1 = p with limb 0 less.)
    // Cells of KARA_MUL2.  One product column is < NL 2^58 < 2^64, the sum of two is up to 2 NL 2^58 > 2^64, so the sum never
    // sits in one 64-bit cell.  The half products of the two pairs ARE summed, P0 = x0 y0 + x2_0 y2_0 and likewise P2: a
    // coefficient has at most H products per pair, 2 H 2^58 = NL 2^58 < 2^64, and only one set of 2 x H of them is live, as
    // for a single product.  The outer part of column k (P0_k, or P2_(k-2H): never both) goes through the carry stream cc
    // first and leaves 29 bits; the middle part P0_j + P2_j - D_j, j = k - H (the x0 y1 + x1 y0 terms of both pairs, up to
    // 4 H = 2 NL products) is then added to those 29 bits in a 128-bit cell: P0_j, P2_j < 2^63.2 unsigned, -D_j of EITHER pair
    // a sum of H signed products, |.| < 2^62.2, exact in int64 at every partial sum (the two together can pass 2^63, so each
    // has its own cell and is sign-extended into the wide one); the cell is in [0, 2 NL 2^58 + 2^29) = [0, 2^64.2) and its carry joins cc:
    // cc < 2^34.2 + 2^35.2 < 2^35.8, outer + cc < 2^63.3.  The reduction column is d <= NL 2^58 + 2^30 + 2^36 as before.
    // w and v equal those of the row-wise sqr() / mul() exactly (the quotient digits are unique modulo R).  The difference
    // limbs depend on one operand each: after inlining, the two passes of one product share those of the left digit a and of
    // the right digit c (common subexpressions), so each is formed once per product.
    // KRED (compile time): the quotient products sum_i mq[i] nm[k - i] of the reduction are a product of two NL-limb numbers
    // as well, m p, and take the same column form:  Y_k = Q0_k + (Q0 + Q2 - E)_(k-H) + Q2_(k-2H),  Q0 = m0 p0, Q2 = m1 p1,
    // E = (m0 - m1)(p0 - p1): 3 H^2 + H multiply-adds per pass (990) instead of NL^2 (1 296).  One operand is the wave-uniform
    // modulus: its differences ndp[l] = nm[H + l] - nm[l] are H scalars.  Written with U_k = Q0_k + Q2_(k-H), ONE chain of at
    // most H products (< H 2^58 < 2^62.2) that is stored once and kept for H columns:  Y_k = U_k + U_(k-H) - E_(k-H).
    // The digits appear one per column, and column k needs none beyond mq[k].  For H <= k < NL the terms of the column's own
    // digit are mq[k] nm[H] (in U_k) and mq[k] (nm[0] - nm[H]) (in -E_(k-H), from (mq[k-H] - mq[k]) ndp[0]): together mq[k] nm[0], the
    // one product the schoolbook column has.  So the column is formed without mq[k] (its -E term takes mq[k-H] alone), mq[k]
    // follows from it as before, mq[k] nm[0] is added, and U_k is completed with mq[k] nm[H] off the critical path; for k < H,
    // U_k = Q0_k completed with mq[k] nm[0] is the column's last product.  -E is accumulated by signed multiply-adds onto the
    // column: it is the schoolbook column (< NL 2^58 + 2^36 + 2^30), every partial sum is exact modulo 2^64, |partial sums of
    // -E| < H 2^58.  mq, out and the carry are bit for bit those of the schoolbook columns.
    // VF (compile time; all forms but KARA_MUL2): the product stream likewise as V_k = P0_k + P2_(k-H), one chain kept for H
    // columns, X_k = V_k + V_(k-H) - D_(k-H): one stored sum and two 64-bit additions per column instead of two and four.  A
    // square takes the pairs i < l once and doubles their sum (and that of their signed products in -D) instead of keeping
    // doubled copies of the limbs.  Cells: tools/kara_model.py (kred, vf).
    static constexpr int KARA_SQR = 0, KARA_SQR2 = 1, KARA_MUL = 2, KARA_MUL2 = 3;
    template <int FORM, bool KRED = false, bool VF = false>
    PAI_DEV static void kara_pass(uint32_t (&out)[NL], uint32_t (&mq)[NL], const uint32_t (&x)[NL], const uint32_t (&y)[NL],
                                  const uint32_t (&x2)[NL], const uint32_t (&y2)[NL], const uint32_t (&min)[NL],
                                  const uint32_t* __restrict__ nm, uint32_t n0inv) {
        static_assert(NL % 2 == 0, "even limb count");
        static_assert(!(VF && FORM == KARA_MUL2), "the sum of two products keeps its summed half products");
        constexpr bool SYM = FORM == KARA_SQR, DBL = FORM == KARA_SQR2, SUM = FORM == KARA_MUL2;
        constexpr bool SECOND = DBL || SUM;               // - min + R p enters the reduction columns
        constexpr int H = NL / 2, NP = 2 * H - 1;         // half-product coefficients 0 .. NP - 1
        int32_t nx[H], dy[H];                             // nx = x1 - x0, dy = y0 - y1: nx * dy = -(x0 - x1)(y0 - y1)
        int32_t nx2[H], dy2[H];                           // SUM: the same for the second pair; SYM: dy doubled
        uint32_t yd[NL];                                  // doubled limbs for the symmetric square
#pragma unroll
        for (int i = 0; i < H; ++i) {
            nx[i] = (int32_t)x[i + H] - (int32_t)x[i];
            dy[i] = (int32_t)y[i] - (int32_t)y[i + H];
            nx2[i] = SUM ? (int32_t)x2[i + H] - (int32_t)x2[i] : 0;
            dy2[i] = SUM ? (int32_t)y2[i] - (int32_t)y2[i + H] : dy[i] * 2;
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) yd[i] = y[i] << 1;
        // half product of limbs [o, o + H) of x and y, coefficient j (a square: pairs i < l doubled, the diagonal once;
        // SUM: both pairs)
        auto half = [&](int o, int j) -> uint64_t {
            uint64_t s = 0;
            const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
            for (int i = lo; i <= hi; ++i) {
                const int l = j - i;
                if (!SYM) s += (uint64_t)x[o + i] * y[o + l];
                else if (i < l) s += (uint64_t)x[o + i] * yd[o + l];
                else if (i == l) s += (uint64_t)x[o + i] * y[o + i];
                if (SUM) s += (uint64_t)x2[o + i] * y2[o + l];
            }
            return s;
        };
        uint64_t p0[NP], p2[NP];
        uint64_t pv[H + NP];                              // VF: V_k = P0_k + P2_(k-H) of the product stream
        uint64_t ru[H + NP];                              // KRED: U_k = Q0_k + Q2_(k-H) of the quotient stream
        int32_t dm[H], ndp[H];                            // KRED: mq[i] - mq[H + i]; nm[H + l] - nm[l] (wave-uniform)
        if constexpr (KRED) {
#pragma unroll
            for (int l = 0; l < H; ++l) ndp[l] = (int32_t)nm[H + l] - (int32_t)nm[l];
        }
        uint64_t cc = 0, carry = 0;
#pragma unroll
        for (int k = 0; k < 2 * NL - 1; ++k) {
            uint64_t t = 0;
            int64_t nd = 0, nd2 = 0;                      // SUM: -D_j of either pair
            if constexpr (VF && !SUM) {
                // V_k = P0_k + P2_(k-H) as ONE chain of multiply-adds, kept for H columns: X_k = V_k + V_(k-H) - D_(k-H).
                // A square takes the pairs i < l once and doubles their sum.
                const bool mid = k >= H && k - H < NP;
                uint64_t vk = 0, off = 0;
                if (k < NP) {
                    const int lo = k < H ? 0 : k - H + 1, hi = k < H ? k : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = k - i;
                        if (!SYM) vk += (uint64_t)x[i] * y[l];
                        else if (i < l) off += (uint64_t)x[i] * y[l];
                        else if (i == l) vk += (uint64_t)x[i] * y[i];
                    }
                }
                if (mid) {
                    const int j = k - H;
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (!SYM) vk += (uint64_t)x[H + i] * y[H + l];
                        else if (i < l) off += (uint64_t)x[H + i] * y[H + l];
                        else if (i == l) vk += (uint64_t)x[H + i] * y[H + i];
                    }
                }
                if (SYM) vk += off << 1;
                if (k < H + NP) pv[k] = vk;
                t = vk;
                if (k >= H) t += pv[k - H];
                if (mid) {
                    const int j = k - H;
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (!SYM) t += (uint64_t)((int64_t)nx[i] * (int64_t)dy[l]);
                        else if (i < l) nd += (int64_t)nx[i] * (int64_t)dy[l];
                        else if (i == l) t += (uint64_t)((int64_t)nx[i] * (int64_t)dy[i]);
                    }
                    if (SYM) t += (uint64_t)nd << 1;
                }
            } else {
                if (k < NP) { p0[k] = half(0, k); t += p0[k]; }
                if (k >= H && k - H < NP) {
                    const int j = k - H;
                    p2[j] = half(H, j);
                    if (!SUM) t += p0[j] + p2[j];
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (SUM) { nd += (int64_t)nx[i] * (int64_t)dy[l]; nd2 += (int64_t)nx2[i] * (int64_t)dy2[l]; }
                        else if (!SYM) t += (uint64_t)((int64_t)nx[i] * (int64_t)dy[l]);
                        else if (i < l) t += (uint64_t)((int64_t)nx[i] * (int64_t)dy2[l]);
                        else if (i == l) t += (uint64_t)((int64_t)nx[i] * (int64_t)dy[i]);
                    }
                }
                if (k >= 2 * H) t += p2[k - 2 * H];
            }
            uint64_t c = t + cc;
            cc = c >> RB;
            if (SUM && k >= H && k - H < NP) {
                const unsigned __int128 e = (unsigned __int128)p0[k - H] + p2[k - H] + (unsigned __int128)(__int128)nd +
                                           (unsigned __int128)(__int128)nd2 + ((uint32_t)c & RMASK);
                cc += (uint64_t)(e >> RB);
                c = (uint64_t)e;
            }
            const uint64_t lowc = DBL ? (uint64_t)(((uint32_t)c & RMASK) << 1) : (uint64_t)((uint32_t)c & RMASK);
            uint64_t d = lowc;
            if (SECOND) d += k < NL ? (uint64_t)((RMASK - min[k]) + (k == 0 ? 1u : 0u)) : (uint64_t)(nm[k - NL] - (k == NL ? 1u : 0u));
            if constexpr (KRED) {
                // quotient products m p by Karatsuba columns (see above).  U_k = Q0_k + Q2_(k-H) is ONE chain of multiply-adds,
                // kept for H columns; the column is U_k + U_(k-H) - E_(k-H).  The terms of the newest known digit mq[k - 1]
                // close their chains; the column's own digit mq[k] is taken from the column without its terms.
                constexpr int NU = H + NP;                // U_0 .. U_(NU-1)
                const bool has_u = k < NU, mid = k >= H && k - H < NP;
                uint64_t u = 0;
                if (k < NP) {
                    const int lo0 = k < H ? 0 : k - H + 1, hi0 = k < H ? k - 1 : H - 1;
#pragma unroll
                    for (int i = lo0; i <= hi0; ++i)
                        if (i != k - 1) u += (uint64_t)mq[i] * nm[k - i];
                }
                if (mid) {
                    const int j = k - H;
                    const int lo2 = j < H ? 0 : j - H + 1, hi2 = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo2; i <= hi2; ++i) {
                        const int l = j - i;
                        if (i == j && k < NL) {           // mq[k] unknown: the share of mq[j] alone; mq[k] (nm[H] - ndp[0]) = mq[k] nm[0] follows
                            d += (uint64_t)((int64_t)(int32_t)mq[i] * (int64_t)ndp[0]);
                        } else if (H + i != k - 1) {
                            u += (uint64_t)mq[H + i] * nm[H + l];
                            d += (uint64_t)((int64_t)dm[i] * (int64_t)ndp[l]);
                        }
                    }
                }
                if (k >= H) d += ru[k - H];
                d += carry;
                if (k >= 1 && k <= H) u += (uint64_t)mq[k - 1] * nm[1];
                if (k - 1 >= H && k - 1 < NL) {           // i = j - 1, l = 1
                    u += (uint64_t)mq[k - 1] * nm[H + 1];
                    d += (uint64_t)((int64_t)dm[k - 1 - H] * (int64_t)ndp[1]);
                }
                if (k < H) {
                    mq[k] = (((uint32_t)d + (uint32_t)u) * n0inv) & RMASK;
                    u += (uint64_t)mq[k] * nm[0];
                    d += u;
                } else {
                    if (has_u) d += u;
                    if (k < NL) {
                        mq[k] = ((uint32_t)d * n0inv) & RMASK;
                        d += (uint64_t)mq[k] * nm[0];
                        u += (uint64_t)mq[k] * nm[H];
                        dm[k - H] = (int32_t)mq[k - H] - (int32_t)mq[k];
                    } else {
                        out[k - NL] = (uint32_t)d & RMASK;
                    }
                }
                if (has_u) ru[k] = u;
            } else {
                const int lo = k < NL ? 0 : k - NL + 1, hi = k < NL ? k - 1 : NL - 1;
                // the quotient products that do not wait for the previous column, then its carry and newest digit
#pragma unroll
                for (int i = lo; i <= hi; ++i)
                    if (i != k - 1) d += (uint64_t)mq[i] * nm[k - i];
                d += carry;
                if (k >= 1 && k - 1 < NL) d += (uint64_t)mq[k - 1] * nm[1];
                if (k < NL) {
                    mq[k] = ((uint32_t)d * n0inv) & RMASK;
                    d += (uint64_t)mq[k] * nm[0];
                } else {
                    out[k - NL] = (uint32_t)d & RMASK;
                }
            }
            carry = d >> RB;
        }
        out[NL - 1] = (uint32_t)(carry + (DBL ? cc << 1 : cc) + (SECOND ? nm[NL - 1] : 0u)) & RMASK;
    }
    PAI_DEV static void load_digit(const uint4* x, uint32_t (&r)[NL]) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint4 t = ld(x, c);
            r[4 * c] = t.x; r[4 * c + 1] = t.y; r[4 * c + 2] = t.z; r[4 * c + 3] = t.w;
        }
    }
    PAI_DEV static void sqr_kara(uint4* A, uint4* B, const uint32_t* __restrict__ nm, uint32_t n0inv) {
        uint32_t a[NL], m[NL], w[NL];
        load_digit(A, a);
        kara_pass<KARA_SQR>(w, m, a, a, a, a, m, nm, n0inv);
        // a stays in registers for the second pass: w can take its place in LDS now
        wave_lds_fence();
        store_digit(A, w);
        uint32_t b[NL], m2[NL], v[NL];
        load_digit(B, b);
        kara_pass<KARA_SQR2>(v, m2, a, b, a, b, m, nm, n0inv);
        wave_lds_fence();
        store_digit(B, v);
        wave_lds_fence();
    }
    // ---- the same on digits that STAY in registers from one operation to the next (kernels_padic.hpp: PADIC_LDS_KM) -----
    // RED (compile time): bit FORM set = that pass takes its quotient products by Karatsuba columns (kara_pass<FORM, true>);
    // KRED_VF = the product streams of the squaring's two passes in the one-chain form V_k, KRED_VFM = that of a product's
    // first pass (the second, a sum of two products, keeps its summed half products and the 128-bit middle cell)
    static constexpr int KRED_VF = 16, KRED_VFM = 32;
    static constexpr int PADIC_KMR_RED = (1 << KARA_SQR) | (1 << KARA_SQR2) | (1 << KARA_MUL) | KRED_VF | KRED_VFM;
    static constexpr bool kred(int RED, int FORM) { return (RED >> FORM) & 1; }
    // (a, b) <- (a, b)^2
    template <int RED = 0>
    PAI_DEV static void sqr_kara_reg(uint32_t (&a)[NL], uint32_t (&b)[NL], const uint32_t* __restrict__ nm, uint32_t n0inv) {
        constexpr bool VF = (RED & KRED_VF) != 0;
        uint32_t m[NL], w[NL], m2[NL], v[NL];
        kara_pass<KARA_SQR, kred(RED, KARA_SQR), VF>(w, m, a, a, a, a, m, nm, n0inv);
        kara_pass<KARA_SQR2, kred(RED, KARA_SQR2), VF>(v, m2, a, b, a, b, m, nm, n0inv);
#pragma unroll
        for (int j = 0; j < NL; ++j) { a[j] = w[j]; b[j] = v[j]; }
    }
    // (a, b) <- (a, b) * (c, d): w = (a c + m p) / R, v = (a d + b c - m + R p + m' p) / R, 3 H^2 + 6 H^2 + 2 NL^2 limb
    // products (5 508 at 36 limbs) instead of the row-wise 5 NL^2 (6 480).  rsrc(g, ch): chunk ch of the right operand's
    // digit g (0 = c, 1 = d), each chunk loaded once; d is fetched behind the first pass.
    template <int RED = 0, class RSrc>
    PAI_DEV static void mul_kara_reg(uint32_t (&a)[NL], uint32_t (&b)[NL], RSrc&& rsrc, const uint32_t* __restrict__ nm,
                                     uint32_t n0inv) {
        uint32_t c[NL], d[NL], m[NL], w[NL], m2[NL], v[NL];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const uint4 t = rsrc(0, ch);
            c[4 * ch] = t.x; c[4 * ch + 1] = t.y; c[4 * ch + 2] = t.z; c[4 * ch + 3] = t.w;
        }
        kara_pass<KARA_MUL, kred(RED, KARA_MUL), (RED & KRED_VFM) != 0>(w, m, a, c, a, c, m, nm, n0inv);
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const uint4 t = rsrc(1, ch);
            d[4 * ch] = t.x; d[4 * ch + 1] = t.y; d[4 * ch + 2] = t.z; d[4 * ch + 3] = t.w;
        }
        kara_pass<KARA_MUL2, kred(RED, KARA_MUL2)>(v, m2, a, d, b, c, m, nm, n0inv);
#pragma unroll
        for (int j = 0; j < NL; ++j) { a[j] = w[j]; b[j] = v[j]; }
    }

    // ---- the same on BALANCED digits: one carry stream per column (kernels_padic.hpp: PADIC_LDS_KMRB) -------------------------
    // Every limb is a signed digit in [-2^28, 2^28) (int32; the top limb holds whatever small signed carry is left), the
    // modulus limbs nm likewise, and so are the quotient digits: m == -x y / p (mod R) with digits in [-2^28, 2^28), i.e.
    // |m| <= (2^28 / (2^29 - 1)) R < R/2 (1 + 2^-28).  The product rule loses its offsets:
    //        w = (a c + m p) / R,        v = (a d + b c - m + m' p) / R
    // and w + v p == (a + b p)(c + d p) R^-1 (mod p^2) as before (a c = R w - m p, R v = a d + b c - m + m' p).
    // Cells.  A limb product is at most 2^56 in magnitude, so with NL <= 36 the finished column
    //        d_k = [2] X_k  - min_k  + sum_i mq_i nm_(k-i)  + carry        (X_k: NL products, or 2 NL for a d + b c)
    // is below 36 (2^57 + 2^56) + 2^28 + 2^35 < 2^62.76 in magnitude for all four FORMs and lies inside ONE signed 64-bit
    // cell: there is no second stream (cc), no low-bits hand-over and no 128-bit middle cell.  Every stored sum (V_k, U_k,
    // P0 / P2, -D, -E) and every partial sum need only be exact modulo 2^64; only the finished d_k is shifted, arithmetically.
    // Differences of balanced digits are below 2^29, D_j and E_j below 18 2^58 in magnitude as in the unsigned form.
    // Digits.  k < NL: mq_k = the signed 29-bit field of d_k n0inv, then d_k + mq_k nm_0 == 0 (mod 2^29) and the carry
    // d_k >> 29 is exact.  k >= NL: out_(k-NL) = the signed 29-bit field of d_k and the carry is (d_k + 2^28) >> 29; the last
    // carry is the top limb.  |carry| <= 2^62.76 / 2^29 + 1 < 2^34.
    // Invariant.  For |a|, |b|, |c|, |d| < 0.51 p and R / p >= 2^20:  |w| <= (0.2601 p^2 + |m| p) / R < (0.2601 2^-20 + 0.5
    // (1 + 2^-28)) p < 0.51 p, and |v| <= (0.5202 p^2 + |m| + |m'| p) / R < (0.5202 2^-20 + 0.5 (1 + 2^-28)) p + 0.51 < 0.51 p.
    // (Operands up to 2.01 p, the digit-form entry's lazy range, give |w|, |v| < (8.1 2^-20 + 0.5 (1 + 2^-28)) p + 0.51 as well.)
    // The Karatsuba identities of kara_pass (X_k, KRED: Y_k = U_k + U_(k-H) - E_(k-H), VF: X_k = V_k + V_(k-H) - D_(k-H)) are
    // identities over the integers and hold for signed limbs unchanged.  VF here serves all four FORMs: the sum of two
    // products is one chain V_k as well.  Cells: tools/kara_model.py (kara_pass_bal).
#ifndef PAI_KMRBT_LAZY_DIFFS
#define PAI_KMRBT_LAZY_DIFFS 1        // a fenced pass forms its half differences at the first column that takes them (0: at its head)
#endif
    PAI_DEV static int32_t sfield(uint32_t v) { return (int32_t)(v << (32 - RB)) >> (32 - RB); }
    PAI_DEV static uint64_t smul(int32_t a, int32_t b) { return (uint64_t)((int64_t)a * (int64_t)b); }
    template <int FORM, bool KRED = false, bool VF = false, int ONES = 0, bool DSYM = false, int FENCE = 0>
    PAI_DEV static void kara_pass_bal(int32_t (&out)[NL], int32_t (&mq)[NL], const int32_t (&x)[NL], const int32_t (&y)[NL],
                                      const int32_t (&x2)[NL], const int32_t (&y2)[NL], const int32_t (&min)[NL],
                                      const int32_t* __restrict__ nm, uint32_t n0inv) {
        static_assert(NL % 2 == 0 && NL <= 36, "even limb count; NL (2^57 + 2^56) < 2^63");
        constexpr bool SYM = FORM == KARA_SQR, DBL = FORM == KARA_SQR2, SUM = FORM == KARA_MUL2;
        constexpr bool SECOND = DBL || SUM;               // - min enters the reduction columns
        constexpr int H = NL / 2, NP = 2 * H - 1;
        int32_t nx[H], dy[H], nx2[H], dy2[H];             // as in kara_pass; SYM without VF: dy2 = dy doubled
        int32_t yd[NL];
        // with fences the differences are formed at the first column that takes them (k == H): a fence keeps them from
        // sinking there by themselves, and until then they would only hold registers
        constexpr bool LAZY = FENCE > 0 && PAI_KMRBT_LAZY_DIFFS;
        auto diffs = [&]() {
#pragma unroll
            for (int i = 0; i < H; ++i) {
                nx[i] = x[i + H] - x[i];
                dy[i] = y[i] - y[i + H];
                nx2[i] = SUM ? x2[i + H] - x2[i] : 0;
                dy2[i] = SUM ? y2[i] - y2[i + H] : dy[i] * 2;
            }
        };
        if (!LAZY) diffs();
#pragma unroll
        for (int i = 0; i < NL; ++i) yd[i] = y[i] * 2;
        auto half = [&](int o, int j) -> uint64_t {
            uint64_t s = 0;
            const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
            for (int i = lo; i <= hi; ++i) {
                const int l = j - i;
                if (!SYM) s += smul(x[o + i], y[o + l]);
                else if (i < l) s += smul(x[o + i], yd[o + l]);
                else if (i == l) s += smul(x[o + i], y[o + i]);
                if (SUM) s += smul(x2[o + i], y2[o + l]);
            }
            return s;
        };
        uint64_t p0[NP], p2[NP];
        uint64_t pv[H + NP];
        uint64_t ru[H + NP];
        int32_t dm[H], ndp[H];
        if constexpr (KRED) {
#pragma unroll
            for (int l = 0; l < H; ++l) ndp[l] = nm[H + l] - nm[l];
        }
        // -1 as a run-time scalar (n0inv is odd): - min[k] then is ONE signed multiply-add onto the column; with the literal
        // the compiler emits sign extension, subtract and borrow (three instructions, 36 columns)
        const int32_t neg1 = -(int32_t)(n0inv & 1u);
        uint64_t carry = 0;
        if constexpr (ONES != 0 && KRED && VF) {
            // ONE stored sum per column.  V_k and U_k are both kept for H columns and both enter column k and column k + H, never
            // apart: S_k = [2] V_k + U_k is all that is needed, and the column is
            //        d_k = S_k + S_(k-H) - [2] D_(k-H) - E_(k-H) - min_k + carry,
            // H live 64-bit sums instead of 2 H and two joining additions per column instead of four.  The chains of V and U run
            // on one register (the first multiply-add of U takes the finished [2] V_k as its addend); the doubled pass takes the
            // doubled right operand (yd, dy2) instead of shifting the column.  What does not wait for the previous column
            // (S_(k-H), -D, -E, -min) is one chain e; s joins it, the carry comes last.  S_k is used modulo 2^64 only; d_k is the
            // same integer as in the two-sum form, so mq, out and carry are bit for bit the same.  ONES == 1: the terms of the
            // newest digit mq[k - 1] go onto s before the column is formed; ONES == 2: onto s and onto the column, one
            // multiply-add more and s off the column's dependency chain.  Cells: tools/kara_model.py (ones).
            // SUM (the second pass of a product, a d + b c; PADIC_KMRBT_RED only): V_k sums both pairs' products and -D both
            // pairs' signed products, the latter on e, the chain that does not wait for the carry.  The parts of S_k double
            // their bounds (|V_k| <= 2 H 2^56) and wrap as before; the finished column is the one of the two-sum form, below
            // 2^62.76.  Cells: tools/kara_model.py (kara_pass_bal_sum).
            // DSYM (the first pass of a squaring; KRED_DSYM): the off-diagonal products x_i x_l, i < l, take the doubled operand
            // (yd, dy2) as the doubled pass does and go straight onto s and e: no chain of their own (off, nd), no 64-bit shift
            // and no joining addition for it.  |2 x_l| <= 2^29 and |2 (x_l - x_(l+H))| <= 2^30 are int32, a product is at most
            // 2^59, and x_i (2 x_l) == (x_i x_l) << 1 modulo 2^64, which is all a stored sum needs: S_k, e and with them d_k, mq,
            // out and every carry are bit for bit those of the shifted form.  Cells: tools/kara_model.py (ones, dsym).
            constexpr int NU = H + NP;                    // S_0 .. S_(NU-1)
            uint64_t ss[NU];
#pragma unroll
            for (int k = 0; k < 2 * NL - 1; ++k) {
                const bool mid = k >= H && k - H < NP;
                const int j = k - H;
                uint64_t s = 0, off = 0;
                if (LAZY && k == H) diffs();
                if (k < NP) {
                    const int lo = k < H ? 0 : k - H + 1, hi = k < H ? k : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = k - i;
                        if (DBL) s += smul(x[i], yd[l]);
                        else if (!SYM) s += smul(x[i], y[l]);
                        else if (i < l && DSYM) s += smul(x[i], yd[l]);
                        else if (i < l) off += smul(x[i], y[l]);
                        else if (i == l) s += smul(x[i], y[i]);
                        if (SUM) s += smul(x2[i], y2[l]);
                    }
                }
                if (mid) {
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (DBL) s += smul(x[H + i], yd[H + l]);
                        else if (!SYM) s += smul(x[H + i], y[H + l]);
                        else if (i < l && DSYM) s += smul(x[H + i], yd[H + l]);
                        else if (i < l) off += smul(x[H + i], y[H + l]);
                        else if (i == l) s += smul(x[H + i], y[H + i]);
                        if (SUM) s += smul(x2[H + i], y2[H + l]);
                    }
                }
                if (SYM && !DSYM) s += off << 1;
                // quotient terms of the digits known before the previous column
                if (k < NP) {
                    const int lo0 = k < H ? 0 : k - H + 1, hi0 = k < H ? k - 1 : H - 1;
#pragma unroll
                    for (int i = lo0; i <= hi0; ++i)
                        if (i != k - 1) s += smul(mq[i], nm[k - i]);
                }
                if (mid) {
                    const int lo2 = j < H ? 0 : j - H + 1, hi2 = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo2; i <= hi2; ++i)
                        if (!(i == j && k < NL) && H + i != k - 1) s += smul(mq[H + i], nm[H + j - i]);
                }
                // the one term of the newest digit: mq[k-1] nm[1] (in Q0_k) or mq[k-1] nm[H+1] (in Q2_(k-H))
                const bool newest = k >= 1 && k <= NL;
                const int nn = k <= H ? 1 : H + 1;
                if (ONES == 1 && newest) s += smul(mq[k - 1], nm[nn]);
                // what does not wait for the previous column's carry
                uint64_t e = k >= H ? ss[k - H] : 0;
                if (mid) {
                    uint64_t nd = 0;
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (DBL) e += smul(nx[i], dy2[l]);
                        else if (!SYM) e += smul(nx[i], dy[l]);
                        else if (i < l && DSYM) e += smul(nx[i], dy2[l]);
                        else if (i < l) nd += smul(nx[i], dy[l]);
                        else if (i == l) e += smul(nx[i], dy[i]);
                        if (SUM) e += smul(nx2[i], dy2[l]);
                    }
                    if (SYM && !DSYM) e += nd << 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        if (i == j && k < NL) e += smul(mq[i], ndp[0]);
                        else if (H + i != k - 1) e += smul(dm[i], ndp[j - i]);
                    }
                }
                if (SECOND && k < NL) e += smul(min[k], neg1);
                if (k - 1 >= H && k - 1 < NL) e += smul(dm[k - 1 - H], ndp[1]);
                uint64_t d = e + s + carry;
                if (ONES == 2 && newest) {
                    s += smul(mq[k - 1], nm[nn]);
                    d += smul(mq[k - 1], nm[nn]);
                }
                if (k < NL) {
                    mq[k] = sfield((uint32_t)d * n0inv);
                    d += smul(mq[k], nm[0]);
                    if (k < H) {
                        s += smul(mq[k], nm[0]);
                    } else {
                        s += smul(mq[k], nm[H]);
                        dm[k - H] = mq[k - H] - mq[k];
                    }
                } else {
                    out[k - NL] = sfield((uint32_t)d);
                }
                if (k < NU) ss[k] = s;
                carry = (uint64_t)((int64_t)(k < NL ? d : d + (1ull << (RB - 1))) >> RB);
                if (FENCE > 0 && k % FENCE == FENCE - 1) __builtin_amdgcn_sched_barrier(0);
            }
            out[NL - 1] = (int32_t)carry;
            return;
        }
#pragma unroll
        for (int k = 0; k < 2 * NL - 1; ++k) {
            uint64_t t = 0;                               // the product column X_k, exact modulo 2^64
            if (LAZY && k == H) diffs();
            if constexpr (VF) {
                const bool mid = k >= H && k - H < NP;
                uint64_t vk = 0, off = 0, nd = 0;
                if (k < NP) {
                    const int lo = k < H ? 0 : k - H + 1, hi = k < H ? k : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = k - i;
                        if (!SYM) vk += smul(x[i], y[l]);
                        else if (i < l) off += smul(x[i], y[l]);
                        else if (i == l) vk += smul(x[i], y[i]);
                        if (SUM) vk += smul(x2[i], y2[l]);
                    }
                }
                if (mid) {
                    const int j = k - H;
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (!SYM) vk += smul(x[H + i], y[H + l]);
                        else if (i < l) off += smul(x[H + i], y[H + l]);
                        else if (i == l) vk += smul(x[H + i], y[H + i]);
                        if (SUM) vk += smul(x2[H + i], y2[H + l]);
                    }
                }
                if (SYM) vk += off << 1;
                if (k < H + NP) pv[k] = vk;
                t = vk;
                if (k >= H) t += pv[k - H];
                if (mid) {
                    const int j = k - H;
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (!SYM) t += smul(nx[i], dy[l]);
                        else if (i < l) nd += smul(nx[i], dy[l]);
                        else if (i == l) t += smul(nx[i], dy[i]);
                        if (SUM) t += smul(nx2[i], dy2[l]);
                    }
                    if (SYM) t += nd << 1;
                }
            } else {
                if (k < NP) { p0[k] = half(0, k); t += p0[k]; }
                if (k >= H && k - H < NP) {
                    const int j = k - H;
                    p2[j] = half(H, j);
                    t += p0[j] + p2[j];
                    const int lo = j < H ? 0 : j - H + 1, hi = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo; i <= hi; ++i) {
                        const int l = j - i;
                        if (!SYM) t += smul(nx[i], dy[l]);
                        else if (i < l) t += smul(nx[i], dy2[l]);
                        else if (i == l) t += smul(nx[i], dy[i]);
                        if (SUM) t += smul(nx2[i], dy2[l]);
                    }
                }
                if (k >= 2 * H) t += p2[k - 2 * H];
            }
            uint64_t d = DBL ? t << 1 : t;
            if (SECOND && k < NL) d += smul(min[k], neg1);
            if constexpr (KRED) {
                constexpr int NU = H + NP;
                const bool has_u = k < NU, mid = k >= H && k - H < NP;
                uint64_t u = 0;
                if (k < NP) {
                    const int lo0 = k < H ? 0 : k - H + 1, hi0 = k < H ? k - 1 : H - 1;
#pragma unroll
                    for (int i = lo0; i <= hi0; ++i)
                        if (i != k - 1) u += smul(mq[i], nm[k - i]);
                }
                if (mid) {
                    const int j = k - H;
                    const int lo2 = j < H ? 0 : j - H + 1, hi2 = j < H ? j : H - 1;
#pragma unroll
                    for (int i = lo2; i <= hi2; ++i) {
                        const int l = j - i;
                        if (i == j && k < NL) {
                            d += smul(mq[i], ndp[0]);
                        } else if (H + i != k - 1) {
                            u += smul(mq[H + i], nm[H + l]);
                            d += smul(dm[i], ndp[l]);
                        }
                    }
                }
                if (k >= H) d += ru[k - H];
                d += carry;
                if (k >= 1 && k <= H) u += smul(mq[k - 1], nm[1]);
                if (k - 1 >= H && k - 1 < NL) {
                    u += smul(mq[k - 1], nm[H + 1]);
                    d += smul(dm[k - 1 - H], ndp[1]);
                }
                if (k < H) {
                    mq[k] = sfield(((uint32_t)d + (uint32_t)u) * n0inv);
                    u += smul(mq[k], nm[0]);
                    d += u;
                } else {
                    if (has_u) d += u;
                    if (k < NL) {
                        mq[k] = sfield((uint32_t)d * n0inv);
                        d += smul(mq[k], nm[0]);
                        u += smul(mq[k], nm[H]);
                        dm[k - H] = mq[k - H] - mq[k];
                    } else {
                        out[k - NL] = sfield((uint32_t)d);
                    }
                }
                if (has_u) ru[k] = u;
            } else {
                const int lo = k < NL ? 0 : k - NL + 1, hi = k < NL ? k - 1 : NL - 1;
#pragma unroll
                for (int i = lo; i <= hi; ++i)
                    if (i != k - 1) d += smul(mq[i], nm[k - i]);
                d += carry;
                if (k >= 1 && k - 1 < NL) d += smul(mq[k - 1], nm[1]);
                if (k < NL) {
                    mq[k] = sfield((uint32_t)d * n0inv);
                    d += smul(mq[k], nm[0]);
                } else {
                    out[k - NL] = sfield((uint32_t)d);
                }
            }
            carry = (uint64_t)((int64_t)(k < NL ? d : d + (1ull << (RB - 1))) >> RB);
            if (FENCE > 0 && k % FENCE == FENCE - 1) __builtin_amdgcn_sched_barrier(0);
        }
        out[NL - 1] = (int32_t)carry;
    }
    // RED as for sqr_kara_reg / mul_kara_reg; KRED_VFS = the sum of two products (second pass of a product) as one chain V_k
    // too, which the single cell makes possible: 449.8 -> 444.3 ms per step against the summed half products; that pass's
    // reduction by U_k on top was not faster in the unsigned form (profiles/r14/) and costs registers here (profiles/r15/)
    static constexpr int KRED_VFS = 64;
    static constexpr int PADIC_KMRB_RED = PADIC_KMR_RED | KRED_VFS;
    // KRED_ONES = the passes that have both KRED and VF (both of a squaring, the first of a product) keep ONE stored sum per
    // column, S_k = [2] V_k + U_k (kara_pass_bal: ONES); KRED_ONES2 on top = the terms of the newest quotient digit are added
    // to the sum and to the column separately.  Kernel mode PADIC_LDS_KMRBS.  The second pass of a product keeps its form in
    // this mode; in the one-sum form with Karatsuba quotient products (PADIC_KMRBT_RED below) it is shorter, gained nothing by
    // itself on top of the staged right operand (profiles/r20/README.md) and runs in mode PADIC_LDS_KMRBT since the product's
    // columns are fenced (profiles/r25/README.md).
    static constexpr int KRED_ONES = 128, KRED_ONES2 = 256;
#ifndef PAI_KMRBS_NEWEST_TWICE
#define PAI_KMRBS_NEWEST_TWICE 0      // 1: build the other placement of the newest digit's terms (profiles/r17/README.md)
#endif
    static constexpr int PADIC_KMRBS_RED = PADIC_KMRB_RED | KRED_ONES | (PAI_KMRBS_NEWEST_TWICE ? KRED_ONES2 : 0);
    static constexpr int ones(int RED) { return (RED & KRED_ONES) ? ((RED & KRED_ONES2) ? 2 : 1) : 0; }
    // KRED_DSYM = the first pass of a squaring in the one-sum form sums its off-diagonal products on the doubled operand
    // (kara_pass_bal: DSYM).  Kernel mode PADIC_LDS_KMRBT with PAI_KMRBT_PARTS & 4 (profiles/r25/README.md).
    static constexpr int KRED_DSYM = 512;
    // SQF / MULF: a scheduling fence (sched_barrier) after every SQF resp. MULF columns of either pass (0: none), as
    // kara2_step_bal has: the scheduler works on a few columns at a time instead of a whole pass (profiles/r25/README.md)
    template <int RED = 0, int SQF = 0>
    PAI_DEV static void sqr_kara_reg_bal(int32_t (&a)[NL], int32_t (&b)[NL], const int32_t* __restrict__ nm, uint32_t n0inv) {
        constexpr bool VF = (RED & KRED_VF) != 0;
        int32_t m[NL], w[NL], m2[NL], v[NL];
        kara_pass_bal<KARA_SQR, kred(RED, KARA_SQR), VF, ones(RED), (RED & KRED_DSYM) != 0, SQF>(w, m, a, a, a, a, m, nm, n0inv);
        kara_pass_bal<KARA_SQR2, kred(RED, KARA_SQR2), VF, ones(RED), false, SQF>(v, m2, a, b, a, b, m, nm, n0inv);
#pragma unroll
        for (int j = 0; j < NL; ++j) { a[j] = w[j]; b[j] = v[j]; }
    }
    template <int RED = 0, class RSrc>
    PAI_DEV static void mul_kara_reg_bal(int32_t (&a)[NL], int32_t (&b)[NL], RSrc&& rsrc, const int32_t* __restrict__ nm,
                                         uint32_t n0inv) {
        int32_t c[NL], d[NL], m[NL], w[NL], m2[NL], v[NL];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const uint4 t = rsrc(0, ch);
            c[4 * ch] = (int32_t)t.x; c[4 * ch + 1] = (int32_t)t.y; c[4 * ch + 2] = (int32_t)t.z; c[4 * ch + 3] = (int32_t)t.w;
        }
        kara_pass_bal<KARA_MUL, kred(RED, KARA_MUL), (RED & KRED_VFM) != 0, ones(RED)>(w, m, a, c, a, c, m, nm, n0inv);
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const uint4 t = rsrc(1, ch);
            d[4 * ch] = (int32_t)t.x; d[4 * ch + 1] = (int32_t)t.y; d[4 * ch + 2] = (int32_t)t.z; d[4 * ch + 3] = (int32_t)t.w;
        }
        kara_pass_bal<KARA_MUL2, kred(RED, KARA_MUL2), (RED & KRED_VFS) != 0, kred(RED, KARA_MUL2) ? ones(RED) : 0>(v, m2, a, d, b, c, m, nm, n0inv);
#pragma unroll
        for (int j = 0; j < NL; ++j) { a[j] = w[j]; b[j] = v[j]; }
    }
    // The same product with the right operand (c, d) STAGED in this wave's LDS digit buffers C and D (kernels_padic.hpp:
    // PADIC_LDS_KMRBT, which loads them from the table ahead of the step's squarings) and, with 1 << KARA_MUL2 in RED, the second
    // pass in the one-sum form with Karatsuba quotient products as well (PADIC_KMRBT_RED).  The caller has waited for the staged
    // loads.  REREAD: c is read from LDS again at the head of the second pass instead of being kept in 36 registers across the
    // first (the empty asm keeps the compiler from merging the two reads).
    static constexpr int PADIC_KMRBT_RED = PADIC_KMRBS_RED | (1 << KARA_MUL2);
    PAI_DEV static void load_digit_bal(const uint4* x, int32_t (&r)[NL]) {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const uint4 t = ld(x, ch);
            r[4 * ch] = (int32_t)t.x; r[4 * ch + 1] = (int32_t)t.y; r[4 * ch + 2] = (int32_t)t.z; r[4 * ch + 3] = (int32_t)t.w;
        }
    }
    template <int RED, bool REREAD, int MULF = 0>
    PAI_DEV static void mul_kara_lds_bal(int32_t (&a)[NL], int32_t (&b)[NL], const uint4* C, const uint4* D,
                                         const int32_t* __restrict__ nm, uint32_t n0inv) {
        constexpr int ONES2ND = kred(RED, KARA_MUL2) ? ones(RED) : 0;
        int32_t c[NL], d[NL], m[NL], w[NL], m2[NL], v[NL];
        load_digit_bal(C, c);
        kara_pass_bal<KARA_MUL, kred(RED, KARA_MUL), (RED & KRED_VFM) != 0, ones(RED), false, MULF>(w, m, a, c, a, c, m, nm, n0inv);
        load_digit_bal(D, d);
        if constexpr (REREAD) {
            int32_t c2[NL];
            asm volatile("" ::: "memory");
            load_digit_bal(C, c2);
            kara_pass_bal<KARA_MUL2, kred(RED, KARA_MUL2), (RED & KRED_VFS) != 0, ONES2ND, false, MULF>(v, m2, a, d, b, c2, m, nm, n0inv);
        } else {
            kara_pass_bal<KARA_MUL2, kred(RED, KARA_MUL2), (RED & KRED_VFS) != 0, ONES2ND, false, MULF>(v, m2, a, d, b, c, m, nm, n0inv);
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) { a[j] = w[j]; b[j] = v[j]; }
    }
    // lazy unsigned limbs (value < R / 2) -> balanced digits of the same integer; the top limb keeps the rest
    PAI_DEV static void to_balanced(const uint32_t (&x)[NL], int32_t (&r)[NL]) {
        int32_t c = 0;
#pragma unroll
        for (int j = 0; j < NL - 1; ++j) {
            const int32_t t = (int32_t)x[j] + c;
            r[j] = sfield((uint32_t)t);
            c = (t + (1 << (RB - 1))) >> RB;
        }
        r[NL - 1] = (int32_t)x[NL - 1] + c;
    }
    // balanced digits of x, |x| < R / 4, plus the balanced modulus (less `less`: 0 or 1) -> limbs in [0, 2^29) of x + p - less
    // (> 0 for |x| < 0.51 p)
    PAI_DEV static void from_balanced_plus_p(const int32_t (&x)[NL], const int32_t* __restrict__ nm, int32_t less, uint32_t (&r)[NL]) {
        int32_t c = -less;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int32_t t = x[j] + nm[j] + c;
            r[j] = (uint32_t)t & RMASK;
            c = t >> RB;
        }
    }

    // ---- (a, b) <- (a, b) * (c, 0) beyond 36 limbs: the balanced columns in TWO half-width steps --------------------------------
    // kara_pass_bal keeps a whole column in one signed cell, which holds for NL <= 36 only.  With HL = NL / 2, X = 2^(29 HL),
    // R = X^2 and c = c0 + c1 X the same Montgomery product is reduced by X twice:
    //        w:  T = (a c0 + q0 n) / X            w = (T + a c1 + q1 n) / X
    //        v:  S = (b c0 - q0 + q0' n) / X      v = (S + b c1 - q1 + q1' n) / X
    // m = q0 + X q1 and m' = q0' + X q1' are the balanced quotients of the one-step rule (they are unique), so w and v are
    // those of kara_pass_bal's rule at R; the invariant |w|, |v| < 0.51 n carries over.
    // One step (kara2_step_bal) is NL + HL - 1 columns.  A column has at most HL product terms (c_h has HL limbs), HL quotient
    // terms (q_h has HL digits), one carried-in digit, one digit of the first quotient and the carry:
    // 36 (2^56 + 2^56) + 2^32 + 2^28 + 2^35 < 2^62.2 at NL = 72, inside one signed cell.
    // Karatsuba.  The step's four products are HL x HL: x_lo c_h and q_h n_lo enter at column 0, x_hi c_h and q_h n_hi at
    // column HL, each split at H = HL / 2 as in kara_pass_bal:  X_j = V_j + V_(j-H) - D_(j-H) with V_j = P0_j + P2_(j-H), and
    // U_j, E_j for the quotient products.  All four share H, so ONE stored sum serves them all,
    //        S_k = V^lo_k + V^hi_(k-HL) + U^lo_k + U^hi_(k-HL),        d_k = S_k + S_(k-H) - (D, E terms) + tin_k - qin_k + carry,
    // H live sums, needed modulo 2^64 only.  q_h n_lo is the quotient product whose digits appear one per column: for
    // H <= k < HL the column is formed without q[k] (its -E term takes q[k-H] alone), then q[k] n[0] is added (kara_pass_bal:
    // KRED).  q_h is complete from column HL on, so q_h n_hi is a plain product.  3 H^2 multiply-adds per product and H more for
    // the collapse: 3 906 per step at NL = 72, 15 624 per (a, b) * (c, 0) against 4 NL^2 = 20 736 (executed: 4 032 and 16 128,
    // see the digits taken twice below and the run-time scalars of the one body).
    // ndp: the half differences of the modulus, ndp[l] = nm[H + l] - nm[l] and ndp[H + l] = nm[HL + H + l] - nm[HL + l].
    // Cells: tools/kara_model.py (kara2_step_bal).
#ifndef PAI_KARA2_SCHED_EVERY
#define PAI_KARA2_SCHED_EVERY 4       // columns between scheduling fences of kara2_step_bal (0: none)
#endif
    // t is the carried-in vector on entry (zero in the first step of a stream) and the step's result on return: digit j is
    // written at column HL + j, after t[j] was read at column j.  qsel = -1 subtracts the first quotient's digits qin (the v
    // stream), 0 leaves them out: ONE body serves all four steps of a product, which keeps the loop inside the instruction cache.
    PAI_DEV static void kara2_step_bal(int32_t (&t)[NL], int32_t (&q)[NL / 2], const int32_t (&x)[NL], const int32_t (&ch)[NL / 2],
                                       const int32_t (&qin)[NL / 2], int32_t qsel, const int32_t* __restrict__ nm,
                                       const int32_t* __restrict__ ndp, uint32_t n0inv) {
        static_assert(NL % 4 == 0 && NL <= 72, "two splits; (NL / 2) (2^57) + 2^36 < 2^63");
        constexpr int HL = NL / 2, H = NL / 4, NP = 2 * H - 1, NU = HL + H + NP, NK = NL + HL - 1;
        int32_t nx[HL], dy[H], dm[H];                     // nx: x1 - x0 of either half of x; dy = ch0 - ch1; dm = q0 - q1
#pragma unroll
        for (int i = 0; i < H; ++i) {
            nx[i] = x[H + i] - x[i];
            nx[H + i] = x[HL + H + i] - x[HL + i];
            dy[i] = ch[i] - ch[H + i];
        }
        const int32_t one = (int32_t)(n0inv & 1u);        // a run-time 1 (n0inv is odd): the carried-in digit is ONE multiply-add (see kara_pass_bal)
        uint64_t ss[NU];
        uint64_t carry = 0;
        // the index range of i in sum_(i + l = j), 0 <= i, l < H
        auto lo_of = [](int j) { return j < H ? 0 : j - H + 1; };
        auto hi_of = [](int j) { return j < H ? j : H - 1; };
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int kh = k - HL;                        // column of the products that enter at HL
            uint64_t s = 0;
            // V: x_lo c_h at k, x_hi c_h at kh
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int c = o ? kh : k, xo = o ? HL : 0;
                if (c >= 0 && c < NP) {
#pragma unroll
                    for (int i = lo_of(c); i <= hi_of(c); ++i) s += smul(x[xo + i], ch[c - i]);
                }
                if (c >= H && c - H < NP) {
                    const int j = c - H;
#pragma unroll
                    for (int i = lo_of(j); i <= hi_of(j); ++i) s += smul(x[xo + H + i], ch[H + j - i]);
                }
            }
            // U: q_h n_hi at kh (every digit known) ...
            if (kh >= 0 && kh < NP) {
#pragma unroll
                for (int i = lo_of(kh); i <= hi_of(kh); ++i) s += smul(q[i], nm[HL + kh - i]);
            }
            if (kh >= H && kh - H < NP) {
                const int j = kh - H;
#pragma unroll
                for (int i = lo_of(j); i <= hi_of(j); ++i) s += smul(q[H + i], nm[HL + H + j - i]);
            }
            // ... and q_h n_lo at k: the digits below k, the newest (q[k - 1]) last; the column's own digit follows below
            if (k < NP) {
#pragma unroll
                for (int i = lo_of(k); i <= hi_of(k); ++i)
                    if (i < k) s += smul(q[i], nm[k - i]);
            }
            if (k >= H && k - H < NP) {
                const int j = k - H;
#pragma unroll
                for (int i = lo_of(j); i <= hi_of(j); ++i)
                    if (!(i == j && k < HL)) s += smul(q[H + i], nm[H + j - i]);
            }
            // what does not wait for the previous column: S_(k-H), -D, -E, the carried-in digit, the first quotient's digit
            uint64_t e = k >= H && k - H < NU ? ss[k - H] : 0;
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                const int j = (o ? kh : k) - H;
                if (j >= 0 && j < NP) {
#pragma unroll
                    for (int i = lo_of(j); i <= hi_of(j); ++i) e += smul(nx[o * H + i], dy[j - i]);
#pragma unroll
                    for (int i = lo_of(j); i <= hi_of(j); ++i) {
                        if (o == 0 && i == j && k < HL) e += smul(q[i], ndp[0]);
                        else e += smul(dm[i], ndp[o * H + j - i]);
                    }
                }
            }
            if (k < NL) e += smul(t[k], one);
            if (k < HL) e += smul(qin[k], qsel);
            uint64_t d = e + s + carry;
            if (k < HL) {
                q[k] = sfield((uint32_t)d * n0inv);
                d += smul(q[k], nm[0]);
                if (k < H) {
                    s += smul(q[k], nm[0]);
                } else {
                    s += smul(q[k], nm[H]);
                    dm[k - H] = q[k - H] - q[k];
                }
            } else {
                t[k - HL] = sfield((uint32_t)d);
            }
            if (k < NU) ss[k] = s;
            carry = (uint64_t)((int64_t)(k < HL ? d : d + (1ull << (RB - 1))) >> RB);
            // the chains of later columns wait for nothing but registers: without a fence the scheduler starts them far ahead
            // and the block spills (profiles/r19/variants.jsonl)
            if (PAI_KARA2_SCHED_EVERY > 0 && k % PAI_KARA2_SCHED_EVERY == PAI_KARA2_SCHED_EVERY - 1) __builtin_amdgcn_sched_barrier(0);
        }
        t[NL - 1] = (int32_t)carry;
    }
    // (a, b) <- (a, b) * (c, 0), c = (c0, c1) in balanced digits (balance_half): the four steps in the order w, w, v, v (the
    // quotient digits of w stay for v, one of T / S is live at a time) as ONE rolled loop around one inlined step;
    // csrc(step, ch), step = 0 .. 3, fills half (step & 1) of c.  Only one digit of the pair is in use at a time: x is a on
    // entry with b parked, and park(y, x) parks y and fetches the parked digit into x (the kernel's LDS digit buffer), so
    // the idle digit costs no registers; on return x is the new a and the new b is parked.
    template <class CSrc, class Park>
    PAI_DEV static void mul_kara2_c0_bal(int32_t (&x)[NL], CSrc&& csrc, Park&& park, const int32_t* __restrict__ nm,
                                         const int32_t* __restrict__ ndp, uint32_t n0inv) {
        int32_t ch[NL / 2], q[NL / 2], qin[NL / 2], qa[NL / 2], qb[NL / 2], t[NL];
#pragma unroll
        for (int j = 0; j < NL / 2; ++j) qin[j] = qa[j] = qb[j] = 0;
#pragma unroll 1
        for (int step = 0; step < 4; ++step) {
            csrc(step, ch);
            if ((step & 1) == 0) {
#pragma unroll
                for (int j = 0; j < NL; ++j) t[j] = 0;
            }
            if (step >= 2) {
#pragma unroll
                for (int j = 0; j < NL / 2; ++j) qin[j] = step == 2 ? qa[j] : qb[j];
            }
            kara2_step_bal(t, q, x, ch, qin, step >= 2 ? -1 : 0, nm, ndp, n0inv);
            if (step < 2) {
#pragma unroll
                for (int j = 0; j < NL / 2; ++j) {
                    if (step == 0) qa[j] = q[j];
                    else qb[j] = q[j];
                }
            }
            if (step & 1) park(t, x);
        }
    }
    // half h of an entry's unsigned limbs -> balanced digits; cy is the carry between the halves (0 into half 0), the top
    // limb of half 1 keeps the rest
    PAI_DEV static void balance_half(const uint32_t (&u)[NL / 2], int h, int32_t& cy, int32_t (&r)[NL / 2]) {
        if (h == 0) cy = 0;
#pragma unroll
        for (int j = 0; j < NL / 2; ++j) {
            const int32_t t = (int32_t)u[j] + cy;
            r[j] = sfield((uint32_t)t);
            cy = (t + (1 << (RB - 1))) >> RB;
        }
        r[NL / 2 - 1] += h == 1 ? cy << RB : 0;
    }

    // (A, B) <- (A, B) * (C, D), the second operand's digits supplied per row block
    template <class CSrc, class DSrc>
    PAI_DEV static void mul(uint4* A, uint4* B, MBuf M, CSrc&& csrc, DSrc&& dsrc, const uint32_t* __restrict__ nm,
                            const uint32_t* __restrict__ pm1, uint32_t n0inv) {
        uint32_t w[NL], v[NL];
        mm1_mul(w, M, A, csrc, nm, n0inv);
        mm2_mul(v, M, A, B, dsrc, csrc, nm, pm1, n0inv);
        wave_lds_fence();
        store_digit(A, w);
        store_digit(B, v);
        wave_lds_fence();
    }

    // Plain product with addend, no reduction:  X * D + W  (X in LDS, D digits per block, W < 2^(29 NL) in registers).
    // The low NL limbs are written to the LDS digit buffer LO (chunk-major), the high NL limbs returned in hi.
    template <class DSrc>
    PAI_DEV static void mul_plain(uint32_t (&hi)[NL], uint4* LO, const uint32_t (&W)[NL], const uint4* X, DSrc&& dsrc) {
        uint64_t acc[NW];
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[j] = W[j];
#pragma unroll
        for (int j = NL; j < NW; ++j) acc[j] = 0;
#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            uint32_t xv[U], low[U];
            dsrc(blk, xv);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const uint4 t = ld(X, c);
                const uint32_t xa[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[4 * c + k + u] += (uint64_t)xa[k] * xv[u];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                low[u] = (uint32_t)acc[u] & RMASK;
                acc[u + 1] += acc[u] >> RB;
            }
#pragma unroll
            for (int c = 0; c < UC; ++c)
                st(LO, UC * blk + c, make_uint4(low[4 * c], low[4 * c + 1], low[4 * c + 2], low[4 * c + 3]));
            slide(acc);
            if (blk != NB - 1 && ((blk + 1) * U) % P1 == 0) normalize(acc);
        }
        finish(acc, hi);
    }

    // x (NL limbs, < 4p say) -> canonical [0, p) by up to `times` conditional subtractions, in registers
    PAI_DEV static void cond_sub(uint32_t (&x)[NL], const uint32_t* __restrict__ nm) {
        uint32_t d[NL];
        int32_t borrow = 0;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int32_t t = (int32_t)x[j] - (int32_t)nm[j] + borrow;
            d[j] = (uint32_t)t & RMASK;
            borrow = t >> RB;
        }
        const bool ge = (borrow == 0);
#pragma unroll
        for (int j = 0; j < NL; ++j) x[j] = ge ? d[j] : x[j];
    }
};

}  // namespace pai
