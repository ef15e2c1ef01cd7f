// SHA-256 on the device (FIPS 180-4): the Fiat-Shamir transcript of verifiable threshold decryption.
//   k_sha256_rows    one digest per ROW of up to four limb matrices read side by side: row j's message is the concatenation of row j
//                    of every part, its words exactly as they lie in memory.  One row per lane, a grid-stride loop over tiles of
//                    BLOCK_THREADS rows; every lane loads its own 64-byte block (four 16-byte loads at the row stride).  A variant
//                    that loaded the blocks of 64 rows coalesced (four lanes per block) and handed them over through LDS at a row
//                    stride of 17 dwords was measured level with this form at every size (the kernel is bound
//                    by its rounds, not by its loads) and is not kept.
//   k_sha256_expand  row j: the leading words of SHA-256(seed || tag || LE64(first_index + j)), a one-block message
// Messages are whole 32-bit words (k_sha256_rows) or one block prepared on the host (k_sha256_expand), so the padding is word
// arithmetic.  The 16-word message schedule rolls in registers; the 64 rounds are unrolled with the constants as literals.
#pragma once
#include "kernels_common.hpp"

namespace pai {

constexpr int SHA_MAX_PARTS = 4;
constexpr int SHA_MAX_WORDS = 4096;          // per part

__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int r) { return __builtin_amdgcn_alignbit(x, x, r); }     // funnel shift

__device__ __forceinline__ void sha256_init(uint32_t (&st)[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// one compression: w holds the block's sixteen big-endian words and is overwritten by the rolling schedule
__device__ __forceinline__ void sha256_block(uint32_t (&st)[8], uint32_t (&w)[16]) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        if (t >= 16) {
            const uint32_t x = w[(t + 1) & 15], y = w[(t + 14) & 15];
            w[t & 15] += (sha_rotr(x, 7) ^ sha_rotr(x, 18) ^ (x >> 3)) + w[(t + 9) & 15] + (sha_rotr(y, 17) ^ sha_rotr(y, 19) ^ (y >> 10));
        }
        const uint32_t t1 = h + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t & 15];
        const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

struct Sha256RowsParams {
    const uint32_t* part[SHA_MAX_PARTS];     // [n][words[k]] each
    int words[SHA_MAX_PARTS];
    int K;
    int total_words;                         // sum of words[k]: the message is 4 total_words bytes
};

__device__ __forceinline__ const uint32_t* sha_part(const Sha256RowsParams& P, int k) {
    return k == 0 ? P.part[0] : (k == 1 ? P.part[1] : (k == 2 ? P.part[2] : P.part[3]));
}
__device__ __forceinline__ int sha_part_words(const Sha256RowsParams& P, int k) {
    return k == 0 ? P.words[0] : (k == 1 ? P.words[1] : (k == 2 ? P.words[2] : P.words[3]));
}

// digest: [n][8] words — the 32 digest bytes of row j in their standard order
__global__ void __launch_bounds__(BLOCK_THREADS)
k_sha256_rows(Sha256RowsParams P, uint32_t* __restrict__ digest, int n) {
    const int TW = P.total_words;
    const int nblocks = (TW + 1 + 2 + 15) / 16;                   // the 0x80 word and the 64-bit length behind the message
    const int tiles = (int)(((long long)n + BLOCK_THREADS - 1) / BLOCK_THREADS);      // n up to 2^31 - 1
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row = tile * BLOCK_THREADS + (int)threadIdx.x;  // tile * 256 + 255 < 2^31 + 255 only when n <= 2^31 - 1: no wrap
        const bool live = row < n;
        uint32_t st[8];
        sha256_init(st);
        int k = 0, o = 0;                                         // the cursor: word o of part k — the same for every lane
        for (int blk = 0; blk < nblocks; ++blk) {
            uint32_t w[16];
            const int kw = k < P.K ? sha_part_words(P, k) : 0;
            const uint32_t* base = k < P.K ? sha_part(P, k) : nullptr;
            // the whole block inside one part, every row's block on a 16-byte boundary: vector loads
            const bool vec = k < P.K && o + 16 <= kw && (kw & 3) == 0 && (o & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
            if (vec) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (live) v = *reinterpret_cast<const uint4*>(base + (size_t)row * (size_t)kw + (size_t)(o + 4 * q));
                    w[4 * q] = __builtin_bswap32(v.x); w[4 * q + 1] = __builtin_bswap32(v.y);
                    w[4 * q + 2] = __builtin_bswap32(v.z); w[4 * q + 3] = __builtin_bswap32(v.w);
                }
                o += 16;
                if (o == kw) { ++k; o = 0; }
            } else {
                // word by word: part boundaries, rows off the 16-byte grid, the padding
                const int g0 = blk * 16;
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int g = g0 + t;
                    uint32_t v = 0;
                    if (g < TW) {
                        const int kk = sha_part_words(P, k);
                        if (live) v = __builtin_bswap32(sha_part(P, k)[(size_t)row * (size_t)kk + (size_t)o]);
                        if (++o == kk) { ++k; o = 0; }
                    } else if (g == TW) {
                        v = 0x80000000u;
                    } else if (g == nblocks * 16 - 1) {
                        v = (uint32_t)TW * 32u;                   // the message's bits: below 2^32 for 4 parts of 4096 words
                    }
                    w[t] = v;
                }
            }
            sha256_block(st, w);
        }
        if (live) {
            uint32_t* out = digest + (size_t)row * 8;
            if ((reinterpret_cast<uintptr_t>(digest) & 15) == 0) {
                reinterpret_cast<uint4*>(out)[0] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]),
                                                              __builtin_bswap32(st[3]));
                reinterpret_cast<uint4*>(out)[1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]),
                                                              __builtin_bswap32(st[7]));
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) out[i] = __builtin_bswap32(st[i]);
            }
        }
    }
}

// The one-block message seed || tag || LE64(index) || 0x80 || 0 .. || bit length as sixteen big-endian words with the index bytes
// zero (prepared on the host); the lane puts its index in at byte `pos` = 32 + tag_len (32 .. 47) and stores the first e_words words
// of the digest bytes, read little-endian, the top one masked.
struct Sha256ExpandParams {
    uint32_t block[16];
    int pos;
    uint64_t first_index;
    int e_words;
    uint32_t top_mask;
};

__global__ void __launch_bounds__(BLOCK_THREADS)
k_sha256_expand(Sha256ExpandParams P, uint32_t* __restrict__ out, int n) {
    const int tiles = (int)(((long long)n + BLOCK_THREADS - 1) / BLOCK_THREADS);      // n up to 2^31 - 1
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int row = tile * BLOCK_THREADS + (int)threadIdx.x;
        if (row >= n) continue;
        const uint64_t idx = P.first_index + (uint64_t)row;
        uint32_t w[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) w[t] = P.block[t];
#pragma unroll
        for (int t = 8; t < 14; ++t) {                            // bytes 32 .. 55 hold the index
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int rel = 4 * t + c - P.pos;
                if (rel >= 0 && rel < 8) w[t] |= (uint32_t)((idx >> (8 * rel)) & 0xffu) << (24 - 8 * c);
            }
        }
        uint32_t st[8];
        sha256_init(st);
        sha256_block(st, w);
        uint32_t* o = out + (size_t)row * (size_t)P.e_words;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < P.e_words) o[i] = __builtin_bswap32(st[i]) & (i == P.e_words - 1 ? P.top_mask : 0xffffffffu);
    }
}

}  // namespace pai
