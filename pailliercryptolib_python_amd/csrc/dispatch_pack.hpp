// pai_fp_pack / pai_fp_unpack / pai_ct_pack / pai_ct_pack_step / pai_fp_quantize: packed ciphertexts, k fixed-point slots of b bits
// (kernels_pack.hpp).
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C", after dispatch_reduce.hpp.)
#pragma once

// the layout rule shared by the three calls: 8 <= b <= 128, k >= 1, k b <= bits(n) - 2
static void require_pack_layout(const pai_pubkey* pk, int slot_bits, int slots) {
    require(slot_bits >= 8 && slot_bits <= 128, "packed layout: slot_bits must lie in 8 .. 128");
    require(slots >= 1 && (long long)slots * slot_bits <= (long long)hbn::bitlen(pk->n) - 2,
            "packed layout: slots * slot_bits must not exceed bits(n) - 2");
}

int pai_fp_pack(const pai_pubkey* pk, const void* d_x, int is_f64, size_t N, int exponent, int value_bits, int slot_bits, int slots,
                uint32_t* d_m, int32_t* d_flag, void* stream) {
    return guarded([&] {
        require(pk && d_x && d_m && d_flag, "NULL argument");
        require_pack_layout(pk, slot_bits, slots);
        require(value_bits >= 1 && value_bits + 1 <= slot_bits, "packed layout: value_bits must lie in 1 .. slot_bits - 1");
        require(exponent > -(1 << 20) && exponent < (1 << 20), "exponent out of range");
        if (N == 0) return;
        DeviceScope scope_(pk->device);
        const size_t G = (N + (size_t)slots - 1) / (size_t)slots;
        const dim3 grid((unsigned)((G + 255) / 256)), block(256);
        if (is_f64)
            hipLaunchKernelGGL(k_fp_pack<true>, grid, block, 0, (hipStream_t)stream, d_x, pk->d_nexp, pk->n_words, N, exponent, value_bits,
                               slot_bits, slots, d_m, G, d_flag);
        else
            hipLaunchKernelGGL(k_fp_pack<false>, grid, block, 0, (hipStream_t)stream, d_x, pk->d_nexp, pk->n_words, N, exponent, value_bits,
                               slot_bits, slots, d_m, G, d_flag);
        HIP_CHECK(hipGetLastError());
    });
}

int pai_fp_unpack(const pai_pubkey* pk, const uint32_t* d_m, size_t G, int slot_bits, int slots, int64_t* d_out, int32_t* d_flag,
                  void* stream) {
    return guarded([&] {
        require(pk && d_m && d_out && d_flag, "NULL argument");
        require_pack_layout(pk, slot_bits, slots);
        if (G == 0) return;
        DeviceScope scope_(pk->device);
        const dim3 grid((unsigned)((G + 255) / 256)), block(256);
        if (slot_bits > 64)
            hipLaunchKernelGGL(k_fp_unpack<true>, grid, block, 0, (hipStream_t)stream, d_m, pk->d_nexp, pk->n_words, G, slot_bits, slots,
                               d_out, d_flag);
        else
            hipLaunchKernelGGL(k_fp_unpack<false>, grid, block, 0, (hipStream_t)stream, d_m, pk->d_nexp, pk->n_words, G, slot_bits, slots,
                               d_out, d_flag);
        HIP_CHECK(hipGetLastError());
    });
}

// Row g of the output is the Horner chain acc <- acc^(2^step) * ct[g count + j], j = len_g - 1 ... 0 (pai_ct_pack: step = b,
// count = k; pai_ct_pack_step: any step >= 8 with count step <= bits(n) - 2, the repacking of packed rows).
// Route A (every key size): the member list (rows, steps, chain offsets) is written on the device (k_pack_plan) and run by the
// level driver of pai_ct_segment_prod — k-member chains are cut into chunks when there are too few of them to fill the device,
// and the partials joined at shift step * (chunk length).
// Route B (keys the base-n digit engine serves, wire-form input, pack_padic_min_rows chains or more): the rows are brought to
// digit form once (k_mexp_table_padic at one window bit: entry 0 = one, entry 1 = the ciphertext), then one chain per lane with
// digit-pair squarings (k_ct_pack_padic).  false: the digit forms do not fit the device (the caller takes route A).
static bool ct_pack_padic_locked(const pai_pubkey* pk, hipStream_t s, const uint32_t* d_ct, size_t N, int step, int count, size_t G,
                                 uint32_t* d_out) {
    const int pnl = pk->penc_nl;
    const size_t table_bytes = N * 2 * 2 * (size_t)pnl * 4;
    size_t mem_free = 0, mem_total = 0;
    HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
    if (table_bytes > mem_total / 8 || table_bytes > mem_free + pk->mexp_table.bytes) return false;
    OrderScope order_(pk->order, s);
    pk->mexp_table.ensure(table_bytes);
    MexpPadicParams Q;
    Q.nctx = pk->nmod.d_ctx;
    Q.nm1 = pk->d_nm1;
    Q.nsq = pk->d_nsq29;
    Q.kdig = pk->d_ct_kdig;
    Q.one_dig = pk->d_one_dig;
    Q.mscratch = reinterpret_cast<uint4*>(pk->d_mscratch);
    Q.table = pk->mexp_table.as<uint4>();
    Q.nd = pk->ct_nd;
    Q.ct_words = pk->ct_words;
    Q.R = 1; Q.K = (int)N; Q.M = 1; Q.chunk = count; Q.nsigns = 1;
    Q.e_words = 1; Q.ebits_max = 1; Q.by_rows = 0;
    Q.wbits = 1;
    {
        const size_t tiles = (N + BLOCK_THREADS - 1) / BLOCK_THREADS;
        const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
        ScopedKernelTimer t("k_mexp_table", s);
        launcher(padic_enc_ops(pnl), &PadicEncOps::mexp_table, "no digit-form kernel for this limb count")(s, grid, Q, d_ct, nullptr, (int)N);
        t.stop();
        HIP_CHECK(hipGetLastError());
    }
    {
        const size_t tiles = (G + BLOCK_THREADS - 1) / BLOCK_THREADS;
        const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
        ScopedKernelTimer t("k_ct_pack_padic", s);
        launcher(padic_enc_ops(pnl), &PadicEncOps::ct_pack, "no pack kernel for this limb count")(s, grid, Q, (int)N, count, step, d_out, (int)G);
        t.stop();
        HIP_CHECK(hipGetLastError());
    }
    order_.done();
    return true;
}

// The shared body of pai_ct_pack (step = slot_bits, count = slots) and pai_ct_pack_step: chains of `count` rows, `step` squarings
// between members; the caller has checked count >= 1 and count * step <= bits(n) - 2.  Neither route ties the step to a slot:
// k_ct_pack_padic squares `step` times between members, and k_segprod counts a member's shift down one squaring at a time in an
// int — a chunk join carries the sum of its chunk's shifts, at most count * step < bits(n), so steps in the thousands of bits stay
// far inside the driver's int32 shifts and the chunk length needs no clamp.
static void ct_pack_body(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int step, int count, uint32_t* d_out,
                         void* stream) {
    require(N == 0 || (d_ct && d_out), "NULL argument");
    require(std::abs(tag) <= RPOW_SPAN - 2, "pai_ct_pack: domain tag out of range");
    require(N < ((size_t)1 << 31), "pai_ct_pack: too many rows for one call");
    if (N == 0) return;
    const size_t G = (N + (size_t)count - 1) / (size_t)count;
    require_no_overlap(d_out, G * (size_t)pk->ct_words * 4, d_ct, N * (size_t)pk->ct_words * 4, false, "pai_ct_pack: d_out must not alias d_ct");
    std::lock_guard<std::mutex> lk(pk->mu);
    DeviceScope scope_(pk->device);
    hipStream_t s = (hipStream_t)stream;
    g_last_times.clear();
    if (pk->penc_nl != 0 && tag == 0 && N < ((size_t)1 << 28) && !knob_disabled("pack_padic") &&
        G >= pack_padic_min_rows((size_t)pk->dev.ncu) && ct_pack_padic_locked(pk, s, d_ct, N, step, count, G, d_out))
        return;
    uint32_t* rows;
    int32_t* shift;
    int64_t* offsets;
    {
        OrderScope order_(pk->order, s);
        pk->pack_plan.ensure((G + 1) * sizeof(int64_t) + N * 8);
        offsets = pk->pack_plan.as<int64_t>();
        rows = reinterpret_cast<uint32_t*>(offsets + G + 1);
        shift = reinterpret_cast<int32_t*>(rows + N);
        hipLaunchKernelGGL(k_pack_plan, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, N, count, step, G, rows, shift, offsets);
        HIP_CHECK(hipGetLastError());
        order_.done();
    }
    segment_prod_locked(pk, s, d_ct, N, tag, rows, shift, offsets, G, d_out);
}

int pai_ct_pack(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int slot_bits, int slots, uint32_t* d_out, void* stream) {
    return guarded([&] {
        require(pk != nullptr, "NULL argument");
        require_pack_layout(pk, slot_bits, slots);
        ct_pack_body(pk, d_ct, N, tag, slot_bits, slots, d_out, stream);
    });
}

int pai_ct_pack_step(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int step_bits, int count, uint32_t* d_out,
                     void* stream) {
    return guarded([&] {
        require(pk != nullptr, "NULL argument");
        require(step_bits >= 8, "pai_ct_pack_step: step_bits must be at least 8");
        require(count >= 1 && (long long)count * step_bits <= (long long)hbn::bitlen(pk->n) - 2,
                "pai_ct_pack_step: count * step_bits must not exceed bits(n) - 2");
        ct_pack_body(pk, d_ct, N, tag, step_bits, count, d_out, stream);
    });
}

// Weights at one exponent as multi-exponentiation operands (kernels_pack.hpp: k_fp_quantize, k_fp_quantize_sums).  The limb sums
// live on the handle's scratch (32 bytes per sum, zeroed here on the stream), so the call holds the handle's mutex like the chain
// runners; nothing is read back.
int pai_fp_quantize(const pai_pubkey* pk, const void* d_x, int is_f64, size_t K, size_t M, long long stride_k, long long stride_m,
                    int exponent, int weight_bits, const int64_t* d_offsets, size_t S, uint32_t* d_e, int e_words, uint8_t* d_sign,
                    uint64_t* d_sum, int32_t* d_flag, void* stream) {
    return guarded([&] {
        require(pk && d_flag, "NULL argument");
        require(e_words >= 1 && e_words <= 4, "pai_fp_quantize: e_words must lie in 1 .. 4");
        require(weight_bits >= 1 && weight_bits <= 126 && weight_bits <= 32 * e_words,
                "pai_fp_quantize: weight_bits must lie in 1 .. min(126, 32 e_words)");
        require(exponent > -(1 << 20) && exponent < (1 << 20), "exponent out of range");
        require(d_offsets == nullptr || M == 1, "pai_fp_quantize: segment sums need M = 1");
        require(K < ((size_t)1 << 31) && M < ((size_t)1 << 31) && S < ((size_t)1 << 31), "pai_fp_quantize: too many weights for one call");
        const size_t nsums = d_offsets ? S : M;
        require(nsums == 0 || d_sum, "NULL argument");
        require(K * M == 0 || (d_x && d_e && d_sign), "NULL argument");
        if (nsums == 0 && K * M == 0) return;              // (S = 0 with weights: words and signs are still written)
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        g_last_times.clear();
        OrderScope order_(pk->order, s);
        if (K * M == 0) {                                  // no weights: every sum is 0
            HIP_CHECK(hipMemsetAsync(d_sum, 0, nsums * 16, s));
            return;
        }
        pk->quant_acc.ensure(std::max<size_t>(nsums, 1) * 32);
        if (nsums) HIP_CHECK(hipMemsetAsync(pk->quant_acc.p, 0, nsums * 32, s));
        QuantArgs a;
        a.x = reinterpret_cast<const uint64_t*>(d_x);
        a.K = K; a.M = M; a.sk = stride_k; a.sm = stride_m;
        a.E = exponent; a.wbits = weight_bits; a.ew = e_words;
        a.tj_log2 = 0;
        while (a.tj_log2 < 6 && ((size_t)1 << a.tj_log2) < M) ++a.tj_log2;
        a.vec = (reinterpret_cast<uintptr_t>(d_e) & (size_t)(4 * e_words - 1)) == 0;
        const size_t TJ = (size_t)1 << a.tj_log2, TL = QZ_THREADS / TJ, RM = std::max<size_t>(64, TL);
        a.ncb = (M + TJ - 1) / TJ;
        // about four workgroups per CU in all: long runs of rows per thread keep the sums in registers and the atomics few
        // (PAI_TUNE quantize_blocks: the workgroup count aimed at — tests make one workgroup walk many tiles with it)
        size_t blocks = (size_t)4 * pk->dev.ncu;
        if (long long v; knob_tune("quantize_blocks", &v) && v > 0) blocks = (size_t)v;
        const size_t macros = (K + RM - 1) / RM, want = std::max<size_t>(1, blocks / a.ncb);
        a.rows_per_block = (macros + std::min(macros, want) - 1) / std::min(macros, want) * RM;
        const size_t nrb = (K + a.rows_per_block - 1) / a.rows_per_block;
        require(nrb * a.ncb < ((size_t)1 << 31), "pai_fp_quantize: too many weights for one call");
        a.offsets = d_offsets; a.S = S;
        a.e = d_e; a.sign = d_sign;
        a.acc = pk->quant_acc.as<unsigned long long>();
        a.flag = d_flag;
        const bool via_lds = M > 1 && stride_k == 1 && stride_m != 1;
        const dim3 grid((unsigned)(nrb * a.ncb)), block(QZ_THREADS);
        ScopedKernelTimer t("k_fp_quantize", s);
        if (is_f64) {
            if (via_lds) hipLaunchKernelGGL((k_fp_quantize<true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_fp_quantize<true, false>), grid, block, 0, s, a);
        } else {
            if (via_lds) hipLaunchKernelGGL((k_fp_quantize<false, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_fp_quantize<false, false>), grid, block, 0, s, a);
        }
        HIP_CHECK(hipGetLastError());
        if (nsums)
            hipLaunchKernelGGL(k_fp_quantize_sums, dim3((unsigned)((nsums + 255) / 256)), dim3(256), 0, s, a.acc, nsums, d_sum);
        t.stop();
        HIP_CHECK(hipGetLastError());
        order_.done();
    });
}
