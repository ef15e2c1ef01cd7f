// Packed plaintexts (extension; no reference counterpart): k signed fixed-point slots of b bits in one residue mod n.
//   k_fp_pack     float64 / int64 [N] -> residues [G][nw] of P_g = sum_j m_(g k + j) 2^(b j) mod n,  G = ceil(N / k)
//   k_fp_unpack   residues [G][nw] -> signed mantissas [G k] (int64 for b <= 64, (low uint64, high int64) pairs above)
//   k_pack_plan   the member list of pai_ct_pack's Horner chains for k_segprod (rows in descending slot order, every shift = b)
//   k_fp_quantize float64 / int64 weights [K][M] at any strides -> |w| words [K][M][ew], signs [K][M] and exact sums of |w| per column
//                 or per segment: the operands of pai_ct_multiexp / pai_ct_sparse_multiexp at one common exponent (packed rows)
// The format: element i lives in row i / k, slot i % k, bits [j b, (j + 1) b); with the bias B = sum_j 2^(b - 1) 2^(b j) the
// biased row Q = P + B has the unsigned fields m_j + 2^(b - 1) side by side, so no borrow crosses a slot: pack writes Q - B
// (+ n when P < 0), unpack reads the fields of (residue + B) mod n.  k b <= bits(n) - 2, hence |P| < n / 4 and one conditional
// addition / subtraction of n is all the reduction there is.  HBM-bound: one lane per row streams the row through a 192-bit
// window; rows are stored 16 bytes at a time.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pai {

// word w of the bias B: bits b j + b - 1 for j < k
__device__ __forceinline__ uint32_t pack_bias_word(int w, int b, int k) {
    uint32_t v = 0;
    const int lo = 32 * w;
    int j = lo / b;                                    // the first slot whose top bit is not below this word
    for (int p = b * j + b - 1; j < k && p < lo + 32; ++j, p += b)
        if (p >= lo) v |= 1u << (p - lo);
    return v;
}

// a 192-bit window over a little-endian bit stream: fields of up to 128 bits in, 32-bit words out (pack), or the reverse (unpack)
struct BitWindow {
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    int n = 0;                                         // bits held
    __device__ __forceinline__ void shr(int s) {       // 0 <= s <= 128
        if (s >= 64) { w0 = w1; w1 = w2; w2 = 0; s -= 64; }
        if (s >= 64) { w0 = w1; w1 = w2; w2 = 0; s -= 64; }
        if (s) {
            w0 = (w0 >> s) | (w1 << (64 - s));
            w1 = (w1 >> s) | (w2 << (64 - s));
            w2 >>= s;
        }
    }
    // appends the b-bit field (lo, hi), n < 32 on entry
    __device__ __forceinline__ void push_field(uint64_t lo, uint64_t hi, int b) {
        w0 |= lo << n;
        w1 |= (n ? lo >> (64 - n) : 0ull) | (hi << n);
        w2 |= n ? hi >> (64 - n) : 0ull;
        n += b;
    }
    __device__ __forceinline__ uint32_t pop_word() {   // n >= 32, or the stream has ended (zeros follow)
        const uint32_t v = (uint32_t)w0;
        shr(32);
        n = n >= 32 ? n - 32 : 0;
        return v;
    }
    // appends a 32-bit word, n <= 159 on entry
    __device__ __forceinline__ void push_word(uint32_t v) {
        const int i = n >> 6, s = n & 63;
        const uint64_t a = (uint64_t)v << s, c = s > 32 ? (uint64_t)v >> (64 - s) : 0ull;
        if (i == 0) { w0 |= a; w1 |= c; }
        else if (i == 1) { w1 |= a; w2 |= c; }
        else w2 |= a;
        n += 32;
    }
    __device__ __forceinline__ void pop_field(int b, uint64_t& lo, uint64_t& hi) {     // n >= b
        lo = w0;
        hi = w1;
        if (b < 64) { lo &= (1ull << b) - 1; hi = 0; }
        else if (b < 128) hi &= (1ull << (b - 64)) - 1;
        shr(b);
        n -= b;
    }
};

// The signed mantissa of element i at exponent E as a 128-bit two's-complement pair (lo, hi); status bits as pai_fp_pack's flag:
// 1 = |mantissa| >= 2^vbits, 2 = NaN or infinity.  float64: rint(x 2^E), ties to even, exact for every finite x (the product is
// formed on the 53-bit significand, not in floating point); int64: x << E.
// (raw: the 64 bits of the double or of the int64 — k_fp_quantize hands its values over from LDS.)
template <bool IS_F64>
__device__ __forceinline__ int pack_mantissa_raw(uint64_t raw, int E, int vbits, uint64_t& lo, uint64_t& hi) {
    uint64_t mag;
    bool neg;
    long long q;                                       // the value is +-mag 2^q
    if constexpr (IS_F64) {
        const uint64_t bits = raw;
        const int e = (int)((bits >> 52) & 0x7FF);
        neg = bits >> 63;
        if (e == 0x7FF) { lo = hi = 0; return 2; }
        mag = e ? ((bits & 0xFFFFFFFFFFFFFull) | (1ull << 52)) : (bits & 0xFFFFFFFFFFFFFull);
        q = (long long)(e ? e : 1) - 1075 + E;
    } else {
        const int64_t v = (int64_t)raw;
        neg = v < 0;
        mag = neg ? (0ull - (uint64_t)v) : (uint64_t)v;
        q = E;
    }
    uint64_t mlo = 0, mhi = 0;
    int bad = 0;
    if (mag != 0) {
        if (q >= 0) {
            const int len = 64 - __clzll((long long)mag);
            if (q + len > 127) bad = 1;                // >= 2^127 >= 2^vbits
            else {
                const int s = (int)q;
                mlo = s >= 64 ? 0ull : mag << s;
                mhi = s >= 64 ? mag << (s - 64) : (s ? mag >> (64 - s) : 0ull);
            }
        } else if (q > -64) {
            const int r = (int)-q;
            const uint64_t fl = mag >> r, rem = mag & ((1ull << r) - 1), half = 1ull << (r - 1);
            mlo = fl + ((rem > half || (rem == half && (fl & 1))) ? 1ull : 0ull);
        } else if (q == -64) {
            mlo = mag > (1ull << 63) ? 1ull : 0ull;    // floor 0 is even: a tie rounds down
        }
    }
    // |m| < 2^vbits, vbits <= 127
    if (vbits >= 64 ? (mhi >> (vbits - 64)) != 0 : (mhi != 0 || (mlo >> vbits) != 0)) bad = 1;
    if (neg) {
        lo = 0ull - mlo;
        hi = ~mhi + (mlo == 0 ? 1ull : 0ull);
    } else {
        lo = mlo;
        hi = mhi;
    }
    return bad;
}

template <bool IS_F64>
__device__ __forceinline__ int pack_mantissa(const void* __restrict__ x_, size_t i, int E, int vbits, uint64_t& lo, uint64_t& hi) {
    return pack_mantissa_raw<IS_F64>(reinterpret_cast<const uint64_t*>(x_)[i], E, vbits, lo, hi);
}

// One lane per output row.  The sign of P is that of its highest non-zero slot (the slots below sum to less than 2^(b j)), so
// one pass suffices: word = Q - B (+ n) with a signed carry.  Rows whose inputs set a flag are undefined (never out of bounds).
template <bool IS_F64>
__global__ void __launch_bounds__(256)
k_fp_pack(const void* __restrict__ x, const uint32_t* __restrict__ n_words_ptr, int nw, size_t N, int E, int vbits, int b, int k,
          uint32_t* __restrict__ out, size_t G, int* __restrict__ flag) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const size_t i0 = g * (size_t)k;
    const int len = (int)((N - i0) < (size_t)k ? (N - i0) : (size_t)k);
    bool negP = false;
    for (int j = len - 1; j >= 0; --j) {
        uint64_t lo, hi;
        pack_mantissa<IS_F64>(x, i0 + j, E, vbits, lo, hi);
        if (lo | hi) { negP = hi >> 63; break; }
    }
    const uint64_t blo = b <= 64 ? 1ull << (b - 1) : 0ull, bhi = b <= 64 ? 0ull : 1ull << (b - 65);
    BitWindow win;
    uint32_t* row = out + g * (size_t)nw;
    const bool vec = (nw & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    int j = 0, st = 0;
    long long carry = 0;
    uint32_t q4[4];
    for (int w = 0; w < nw; ++w) {
        while (win.n < 32 && j < k) {
            uint64_t lo = 0, hi = 0;
            if (j < len) st |= pack_mantissa<IS_F64>(x, i0 + j, E, vbits, lo, hi);
            // the biased field (m + 2^(b-1)) mod 2^b
            uint64_t flo = lo + blo, fhi = hi + bhi + (flo < lo ? 1ull : 0ull);
            if (b < 64) { flo &= (1ull << b) - 1; fhi = 0; }
            else if (b < 128) fhi &= b == 64 ? 0ull : (1ull << (b - 64)) - 1;
            win.push_field(flo, fhi, b);
            ++j;
        }
        const long long t = (long long)win.pop_word() - (long long)pack_bias_word(w, b, k) + (negP ? (long long)n_words_ptr[w] : 0ll) + carry;
        carry = t >> 32;
        q4[w & 3] = (uint32_t)t;
        if (!vec) row[w] = (uint32_t)t;
        else if ((w & 3) == 3) *reinterpret_cast<uint4*>(row + w - 3) = make_uint4(q4[0], q4[1], q4[2], q4[3]);
    }
    if (st) atomicOr(flag, st);
}

// One lane per row: pass 1 decides residue >= n (flag 2) and whether residue + B reaches n; pass 2 streams Q = residue + B (- n)
// through the window and writes the k fields minus 2^(b-1).  Bits of Q at or above k b put the row into the overflow zone (flag 1).
// WIDE: slots of more than 64 bits, out[slot] = (low uint64, high int64).
template <bool WIDE>
__global__ void __launch_bounds__(256)
k_fp_unpack(const uint32_t* __restrict__ res, const uint32_t* __restrict__ n_words_ptr, int nw, size_t G, int b, int k,
            int64_t* __restrict__ out, int32_t* __restrict__ flag) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const uint32_t* row = res + g * (size_t)nw;
    uint32_t c = 0, br_r = 0, br_t = 0;                 // carry of r + B, borrows of r - n and (r + B) - n
    for (int w = 0; w < nw; ++w) {
        const uint32_t r = row[w], nn = n_words_ptr[w];
        const uint64_t t = (uint64_t)r + pack_bias_word(w, b, k) + c;
        c = (uint32_t)(t >> 32);
        br_r = (uint32_t)(((uint64_t)r - nn - br_r) >> 63);
        br_t = (uint32_t)(((uint64_t)(uint32_t)t - nn - br_t) >> 63);
    }
    const bool corrupt = br_r == 0;                     // residue >= n
    const bool sub = c != 0 || br_t == 0;               // residue + B >= n
    BitWindow win;
    int64_t* o = out + g * (size_t)k * (WIDE ? 2 : 1);
    const uint64_t blo = b <= 64 ? 1ull << (b - 1) : 0ull, bhi = b <= 64 ? 0ull : 1ull << (b - 65);
    uint32_t over = 0, br = 0;
    c = 0;
    int j = 0;
    for (int w = 0; w < nw; ++w) {
        const uint64_t t = (uint64_t)row[w] + pack_bias_word(w, b, k) + c;
        c = (uint32_t)(t >> 32);
        const uint64_t d = (uint64_t)(uint32_t)t - (sub ? n_words_ptr[w] : 0u) - br;
        br = (uint32_t)(d >> 63);
        if (j >= k && win.n == 0) { over |= (uint32_t)d; continue; }       // above the last slot
        win.push_word((uint32_t)d);
        while (j < k && win.n >= b) {
            uint64_t lo, hi;
            win.pop_field(b, lo, hi);
            // field - 2^(b-1) in wrapping 64 / 128-bit arithmetic IS the two's-complement mantissa (field < 2^b)
            const uint64_t mlo = lo - blo, mhi = hi - bhi - (lo < blo ? 1ull : 0ull);
            if constexpr (WIDE) {
                o[2 * j] = (int64_t)mlo;
                o[2 * j + 1] = (int64_t)mhi;
            } else {
                o[j] = (int64_t)mlo;
            }
            ++j;
        }
        if (j >= k) {                                   // what the window still holds lies above the last slot
            over |= (uint32_t)(win.w0 | (win.w0 >> 32) | win.w1 | (win.w1 >> 32) | win.w2 | (win.w2 >> 32));
            win = BitWindow();
        }
    }
    flag[g] = corrupt ? 2 : (over ? 1 : 0);
}

// The chains of pai_ct_pack as k_segprod members: chain g = rows g k + len - 1 ... g k (the highest slot first), every step b bits
// (pai_ct_pack_step: k = the rows per chain, b = the step, whatever its width — the step is only ever copied into shift[])
__global__ void __launch_bounds__(256)
k_pack_plan(size_t N, int k, int b, size_t G, uint32_t* __restrict__ rows, int32_t* __restrict__ shift, int64_t* __restrict__ offsets) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        const size_t g = i / (size_t)k, t = i - g * (size_t)k, i0 = g * (size_t)k;
        const size_t len = (N - i0) < (size_t)k ? (N - i0) : (size_t)k;
        rows[i] = (uint32_t)(i0 + (len - 1 - t));
        shift[i] = b;
    }
    if (i <= G) offsets[i] = (int64_t)(i * (size_t)k < N ? i * (size_t)k : N);
}

// ---- pai_fp_quantize: a weight matrix at ONE exponent as multi-exponentiation operands ---------------------------------------------
// Weight (l, j) = x[l sk + j sm] -> w = rint(x 2^E) (pack_mantissa_raw), |w| to e[(l M + j) ew ..], w < 0 to sign[l M + j], and the
// sum of |w| over l per column j (or, offsets given and M = 1, per segment [offsets[s], offsets[s + 1])).
// A workgroup owns TJ = 2^tj_log2 columns (the smallest power of two >= min(M, 64)) and a run of rows; thread t works on column
// t % TJ and rows t / TJ + n TL, TL = 256 / TJ, so the words and signs leave with the lanes along j — the order they are stored in.
// The loads run along j too when sm is the unit stride (DIRECT).  When sk is (VIA_LDS) a tile of RM = max(64, TL) rows x TJ columns
// is loaded with the lanes along l and read back transposed from LDS; the pitch RM + 1 (in 8-byte words) spreads the 32 lanes of a
// ds_read_b64 group over all 64 banks.
// Sums: |w| < 2^126 and up to 2^28 rows need 154 bits, so a sum is kept as four sums of 32-bit limbs (each < 2^60: no 64-bit word can
// wrap) and put together by k_fp_quantize_sums.  Column mode: a thread keeps the limb sums of its column in registers over all its
// rows, the lanes of a wave that share a column are folded by shuffles (strides TJ, 2 TJ, ...), the four waves through LDS, and one
// lane per column and workgroup adds to acc[].  Segment mode (TJ = 1, lanes along l, the segment of a row by bisection of offsets):
// a segmented inclusive scan over the wave, the last lane of each run adds.  acc[]: [sums][4] 64-bit words, zeroed by the caller.
constexpr int QZ_THREADS = 256;
constexpr int QZ_TILE_WORDS = 64 * 65;                 // TJ (RM + 1) at its largest: 64 x 65 (2 x 129, 4 x 65, ... are smaller)

struct QuantArgs {
    const uint64_t* x;                                 // the 64 bits of every weight
    size_t K, M;
    long long sk, sm;                                  // strides in elements
    int E, wbits, ew, tj_log2, vec;                    // vec: e is 8-byte (ew = 2) / 16-byte (ew = 4) aligned
    size_t rows_per_block, ncb;                        // a multiple of RM; column blocks
    const int64_t* offsets;                            // NULL: column sums
    size_t S;
    uint32_t* e;
    uint8_t* sign;
    unsigned long long* acc;
    int32_t* flag;
};

template <bool IS_F64, bool VIA_LDS>
__global__ void __launch_bounds__(QZ_THREADS)
k_fp_quantize(QuantArgs a) {
    __shared__ uint64_t tile[VIA_LDS ? QZ_TILE_WORDS : 1];
    __shared__ unsigned long long red[QZ_THREADS / 64][64][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int TJ = 1 << a.tj_log2, TL = QZ_THREADS >> a.tj_log2, RM = TL > 64 ? TL : 64;
    const int tj = t & (TJ - 1), tl = t >> a.tj_log2;
    const size_t cb = (size_t)blockIdx.x % a.ncb, rb = (size_t)blockIdx.x / a.ncb;
    const size_t j0 = cb * (size_t)TJ, j = j0 + (size_t)tj;
    const size_t l_begin = rb * a.rows_per_block;
    const size_t l_end = a.K - l_begin < a.rows_per_block ? a.K : l_begin + a.rows_per_block;
    const bool col_ok = j < a.M;
    const long long S = (long long)a.S;
    unsigned long long sum[4] = {0, 0, 0, 0};
    int st = 0;
    for (size_t lm = l_begin; lm < l_end; lm += (size_t)RM) {
        if constexpr (VIA_LDS) {
            const int rm_log2 = 31 - __clz(RM);
            for (int idx = t; idx < RM * TJ; idx += QZ_THREADS) {
                const int ll = idx & (RM - 1), jj = idx >> rm_log2;
                const size_t l = lm + (size_t)ll, jc = j0 + (size_t)jj;
                if (l < l_end && jc < a.M) tile[jj * (RM + 1) + ll] = a.x[(long long)l * a.sk + (long long)jc * a.sm];
            }
            __syncthreads();
        }
        for (int p = tl; p < RM; p += TL) {            // RM / TL trips for every thread
            const size_t l = lm + (size_t)p;
            const bool ok = col_ok && l < l_end;
            uint64_t mlo = 0, mhi = 0;
            if (ok) {
                uint64_t raw;
                if constexpr (VIA_LDS) raw = tile[tj * (RM + 1) + p];
                else raw = a.x[(long long)l * a.sk + (long long)j * a.sm];
                uint64_t lo, hi;
                st |= pack_mantissa_raw<IS_F64>(raw, a.E, a.wbits, lo, hi);
                const bool neg = hi >> 63;
                mlo = neg ? 0ull - lo : lo;
                mhi = neg ? ~hi + (lo == 0 ? 1ull : 0ull) : hi;
                const size_t o = l * a.M + j;
                uint32_t* w = a.e + o * (size_t)a.ew;
                if (a.ew == 1) w[0] = (uint32_t)mlo;
                else if (a.ew == 2 && a.vec) *reinterpret_cast<uint2*>(w) = make_uint2((uint32_t)mlo, (uint32_t)(mlo >> 32));
                else if (a.ew == 4 && a.vec)
                    *reinterpret_cast<uint4*>(w) = make_uint4((uint32_t)mlo, (uint32_t)(mlo >> 32), (uint32_t)mhi, (uint32_t)(mhi >> 32));
                else
                    for (int i = 0; i < a.ew; ++i) w[i] = (uint32_t)((i < 2 ? mlo : mhi) >> (32 * (i & 1)));
                a.sign[o] = neg ? 1 : 0;
            }
            const unsigned long long limb[4] = {mlo & 0xFFFFFFFFull, mlo >> 32, mhi & 0xFFFFFFFFull, mhi >> 32};
            if (a.offsets == nullptr) {
                for (int i = 0; i < 4; ++i) sum[i] += limb[i];
            } else {
                // the segment of row l: (entries of offsets[0 .. S] that are <= l) - 1; rows of no segment get -1 / S, which keeps
                // the keys of a wave nondecreasing
                long long seg = S;
                if (ok) {
                    long long lo_ = 0, hi_ = S + 1;
                    while (lo_ < hi_) {
                        const long long mid = (lo_ + hi_) >> 1;
                        if (a.offsets[mid] <= (long long)l) lo_ = mid + 1; else hi_ = mid;
                    }
                    seg = lo_ - 1;
                }
                unsigned long long v[4] = {limb[0], limb[1], limb[2], limb[3]};
                for (int d = 1; d < 64; d <<= 1) {
                    const long long oseg = __shfl_up(seg, d);
                    for (int i = 0; i < 4; ++i) {
                        const unsigned long long ov = __shfl_up(v[i], d);
                        if (lane >= d && oseg == seg) v[i] += ov;
                    }
                }
                const long long nseg = __shfl_down(seg, 1);
                if ((lane == 63 || nseg != seg) && seg >= 0 && seg < S)
                    for (int i = 0; i < a.ew; ++i)
                        if (v[i]) atomicAdd(a.acc + (size_t)seg * 4 + i, v[i]);
            }
        }
        if constexpr (VIA_LDS) __syncthreads();        // the tile is free for the next load
    }
    if (a.offsets == nullptr) {
        for (int d = TJ; d < 64; d <<= 1)
            for (int i = 0; i < 4; ++i) {
                const unsigned long long ov = __shfl_down(sum[i], d);
                if (lane + d < 64) sum[i] += ov;
            }
        if (lane < TJ)
            for (int i = 0; i < 4; ++i) red[wave][lane][i] = sum[i];
        __syncthreads();
        if (wave == 0 && lane < TJ && col_ok)
            for (int i = 0; i < a.ew; ++i) {
                const unsigned long long v = red[0][lane][i] + red[1][lane][i] + red[2][lane][i] + red[3][lane][i];
                if (v) atomicAdd(a.acc + j * 4 + i, v);
            }
    }
    if (st) atomicOr(a.flag, st);
}

// acc[s] = the four limb sums of sum s -> sum[s] = (low, high) 64 bits of a0 + a1 2^32 + a2 2^64 + a3 2^96; a total of 2^128 or
// more is stored as 2^128 - 1 (it fails every headroom test a caller can make: slots have at most 128 bits)
__global__ void __launch_bounds__(256)
k_fp_quantize_sums(const unsigned long long* __restrict__ acc, size_t n, uint64_t* __restrict__ sum) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint64_t a0 = acc[4 * s], a1 = acc[4 * s + 1], a2 = acc[4 * s + 2], a3 = acc[4 * s + 3];
    uint64_t lo = a0 + (a1 << 32);
    uint64_t hi = (a1 >> 32) + (lo < a0 ? 1ull : 0ull);                    // < 2^33
    bool over = (a3 >> 32) != 0;
    uint64_t h2 = hi + a2;
    over |= h2 < hi;
    hi = h2 + (a3 << 32);
    over |= hi < h2;
    sum[2 * s] = over ? ~0ull : lo;
    sum[2 * s + 1] = over ? ~0ull : hi;
}

}  // namespace pai
