// The Fiat-Shamir transcript of verifiable threshold decryption: pai_sha256_rows, pai_sha256_expand
// (kernels_sha256.hpp).  The ciphertexts and partial decryptions stay on the device: 32 digest bytes per row come back, not the rows.
//   rows     one SHA-256 digest per row over the row's words in up to four limb matrices (the leaves of the transcript)
//   expand   row j = the leading bits of SHA-256(seed || tag || LE64(first_index + j)) (the fold's coefficients rho_j)
// PAI_TUNE sha_grid caps the workgroups of both (a small batch then walks the tile loop).
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once

static int sha_grid_for(const pai_pubkey* pk, size_t N) {
    const size_t tiles = (N + BLOCK_THREADS - 1) / BLOCK_THREADS;
    int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu * 8));
    long long cap = 0;
    if (knob_tune("sha_grid", &cap) && cap >= 1) grid = (int)std::min<long long>(grid, cap);
    return grid;
}

int pai_sha256_rows(const pai_pubkey* pk, const uint32_t* const* h_parts, const int32_t* h_words, int K, size_t N, uint32_t* d_digest,
                    void* stream) {
    return guarded([&] {
        require(pk && h_parts && h_words, "NULL argument");
        require(K >= 1 && K <= SHA_MAX_PARTS, "pai_sha256_rows: 1 <= K <= 4");
        require(N <= (size_t)0x7fffffff, "pai_sha256_rows: batch too large");
        Sha256RowsParams P{};
        P.K = K;
        for (int k = 0; k < K; ++k) {
            require(h_words[k] >= 1 && h_words[k] <= SHA_MAX_WORDS, "pai_sha256_rows: 1 <= words <= 4096 per part");
            P.words[k] = h_words[k];
            P.total_words += h_words[k];
        }
        g_last_times.clear();
        if (N == 0) return;
        require(d_digest != nullptr, "NULL argument");
        for (int k = 0; k < K; ++k) {
            require(h_parts[k] != nullptr, "NULL argument");
            require_no_overlap(d_digest, N * 32, h_parts[k], N * (size_t)h_words[k] * 4, false, "pai_sha256_rows: d_digest overlaps a part");
            P.part[k] = h_parts[k];
        }
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        const int grid = sha_grid_for(pk, N);
        std::lock_guard<std::mutex> lk(pk->mu);
        OrderScope order_(pk->order, s);
        ScopedKernelTimer t("k_sha256_rows", s);
        hipLaunchKernelGGL(k_sha256_rows, dim3((unsigned)grid), dim3(BLOCK_THREADS), 0, s, P, d_digest, (int)N);
        t.stop();
        HIP_CHECK(hipGetLastError());
        order_.done();
    });
}

int pai_sha256_expand(const pai_pubkey* pk, const uint8_t* h_seed32, const uint8_t* h_tag, int tag_len, uint64_t first_index, size_t N,
                      int bits, uint32_t* d_e, int e_words, void* stream) {
    return guarded([&] {
        require(pk && h_seed32 && (h_tag || tag_len == 0), "NULL argument");
        require(tag_len >= 0 && tag_len <= 15, "pai_sha256_expand: tag_len <= 15 (a one-block message)");
        require(bits >= 32 && bits <= 256 && e_words == (bits + 31) / 32, "pai_sha256_expand: 32 <= bits <= 256, e_words = ceil(bits / 32)");
        require(N <= (size_t)0x7fffffff, "pai_sha256_expand: batch too large");
        g_last_times.clear();
        if (N == 0) return;
        require(d_e != nullptr, "NULL argument");
        uint8_t msg[64] = {};
        std::memcpy(msg, h_seed32, 32);
        if (tag_len) std::memcpy(msg + 32, h_tag, (size_t)tag_len);
        const int pos = 32 + tag_len, len = pos + 8;               // the index bytes stay zero here: the lanes' own
        msg[len] = 0x80;
        msg[62] = (uint8_t)((len * 8) >> 8);
        msg[63] = (uint8_t)(len * 8);
        Sha256ExpandParams P{};
        for (int t = 0; t < 16; ++t)
            P.block[t] = (uint32_t)msg[4 * t] << 24 | (uint32_t)msg[4 * t + 1] << 16 | (uint32_t)msg[4 * t + 2] << 8 | (uint32_t)msg[4 * t + 3];
        P.pos = pos;
        P.first_index = first_index;
        P.e_words = e_words;
        P.top_mask = (bits & 31) ? ((1u << (bits & 31)) - 1u) : 0xffffffffu;
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        const int grid = sha_grid_for(pk, N);
        std::lock_guard<std::mutex> lk(pk->mu);
        OrderScope order_(pk->order, s);
        ScopedKernelTimer t("k_sha256_expand", s);
        hipLaunchKernelGGL(k_sha256_expand, dim3((unsigned)grid), dim3(BLOCK_THREADS), 0, s, P, d_e, (int)N);
        t.stop();
        HIP_CHECK(hipGetLastError());
        order_.done();
    });
}
