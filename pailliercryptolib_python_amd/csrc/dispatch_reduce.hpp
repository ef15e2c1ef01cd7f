// pai_ct_prod / pai_ct_multiexp / pai_ct_invert*: the reductions of ipcl_python.py:746-930 (sum, dot, matmul) and the batch
// inversion behind negative multipliers (ipcl_python.py:426-437).
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once
// one level of a product tree on single Montgomery products: out[i] = a[i] * b[i] * R^-1 mod n^2
static void tree_mul(const pai_pubkey* pk, hipStream_t s, const uint32_t* a, const uint32_t* b, int b_bcast, uint32_t* out, size_t n) {
    if (n == 0) return;
    const GeoOps* g = pk->msq.geo;
    g->modmul(s, grid_for(g, n, pk->dev.ncu), pk->msq.d_ctx, a, b, out, (int)n, pk->ct_words, b_bcast, MODMUL_MONT, nullptr);
    HIP_CHECK(hipGetLastError());
}

// the caller holds pk->mu and has selected the device
static void ct_prod_locked(const pai_pubkey* pk, hipStream_t s, const uint32_t* d_ct, size_t count, size_t groups, uint32_t* d_out,
                           bool clear_times = true) {
    {
        const size_t W = (size_t)pk->ct_words, ROW = W * 4;
        size_t members = count / groups;
        if (members == 1) {
            if (d_out != d_ct) HIP_CHECK(hipMemcpyAsync(d_out, d_ct, count * ROW, hipMemcpyDeviceToDevice, s));
            return;
        }
        // Product over halves, member-major rows [member][group]: level k + 1 has h = ceil(members / 2) members,
        // P[i] = X[i] * X[i + h] for i < members - h (one k_modmul launch over (members - h) * groups contiguous rows);
        // a member without a partner is multiplied by tree_c[k] so that the whole level shares the form R^(1 - 2^(k+1)).
        const size_t h0 = (members + 1) / 2;
        pk->prod_a.ensure(h0 * groups * ROW);
        pk->prod_b.ensure(((h0 + 1) / 2) * groups * ROW);
        OrderScope order_10(pk->order, s);
        if (clear_times) g_last_times.clear();
        ScopedKernelTimer t("k_modmul(tree)", s);
        const uint32_t* src = d_ct;
        uint32_t* bufs[2] = {pk->prod_a.as<uint32_t>(), pk->prod_b.as<uint32_t>()};
        int level = 0;
        while (members > 1) {
            require(level < pai_pubkey::TREE_LEVELS, "ct_prod: too many levels");
            const size_t h = (members + 1) / 2, lo = members - h;
            uint32_t* dst = bufs[level & 1];
            tree_mul(pk, s, src, src + h * groups * W, 0, dst, lo * groups);
            if (lo < h) tree_mul(pk, s, src + lo * groups * W, pk->d_tree_c + (size_t)level * W, 1, dst + lo * groups * W, groups);
            src = dst;
            members = h;
            ++level;
        }
        tree_mul(pk, s, src, pk->d_tree_fix + (size_t)level * W, 1, d_out, groups);     // R^(1 - 2^L) * R^(2^L) * R^-1 = 1
        t.stop();
        order_10.done();
    }
}

int pai_ct_prod(const pai_pubkey* pk, const uint32_t* d_ct, size_t count, size_t groups, uint32_t* d_out, void* stream) {
    return guarded([&] {
        require(pk && d_ct && d_out, "NULL argument");
        require(groups > 0 && count >= groups && count % groups == 0, "count must be a positive multiple of groups");
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        ct_prod_locked(pk, (hipStream_t)stream, d_ct, count, groups, d_out);
    });
}

// Segment products behind PaillierEncryptedNumber.segment_sum (extension).  Segments are badly unbalanced in practice (one bin
// often holds most rows), so no chain runs over a whole segment: every level cuts each segment's member list into chunks of at
// most C members (k_seg_chunk_scan / k_seg_chunk_expand), runs one chain per chunk into a partial row (k_segprod) and hands the
// partials on as the next level's members — row k = chunk k, tag 0 (wire form), shift = the sum of the chunk's member shifts
// (the partial carries the exponent of its last member; the first chunk's shift is ignored like any first member's).  The
// last level runs one chain per segment into d_out.  C of the first level fills the device with chains; later levels hold a
// few partials per segment and take short chunks (latency: one product per member and level).
// The level driver, under pk->mu on the key's device (also the combine step of pai_ct_sparse_multiexp); S > 0.
static void segment_prod_locked(const pai_pubkey* pk, hipStream_t s, const uint32_t* d_ct, size_t N, int tag, const uint32_t* d_rows,
                                const int32_t* d_shift, const int64_t* d_offsets, size_t S, uint32_t* d_out) {
        const uint32_t* rpow = rpow_table(pk);
        const GeoOps* g = pk->msq.geo;
        const size_t W = (size_t)pk->ct_words;
        // the member count and the longest segment (one read-back: the sizes of the levels).  seg_plan is the handle's scratch that
        // an earlier call on another stream may still read: ordered like every other user (OrderScope), closed before the sync
        int64_t stats[2] = {0, 0};
        {
            OrderScope order_0(pk->order, s);
            pk->seg_plan.ensure(2 * sizeof(int64_t));
            hipLaunchKernelGGL(k_seg_stats, dim3(1), dim3(SEG_PLAN_THREADS), 0, s, d_offsets, (int)S, pk->seg_plan.as<int64_t>());
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(stats, pk->seg_plan.p, sizeof(stats), hipMemcpyDeviceToHost, s));
            order_0.done();
        }
        HIP_CHECK(hipStreamSynchronize(s));
        const size_t M = stats[0] > 0 ? (size_t)stats[0] : 0;
        size_t lmax = stats[1] > 0 ? (size_t)stats[1] : 0;
        require(M == 0 || d_ct != nullptr, "NULL argument");
        const size_t C = segprod_chunk((size_t)pk->dev.ncu, g->epb, M);   // first-level chunk (path_ranges.hpp)
        // level sizes: a level of m members in S segments has at most m / C + S chunks
        size_t levels = 0, rows_max = 0;
        {
            size_t m = M, l = lmax, c = C;
            while (l > c) {
                m = std::min(m, m / c + S);
                rows_max = std::max(rows_max, m);
                l = (l + c - 1) / c;
                c = std::min<size_t>(C, 4) < 2 ? 2 : std::min<size_t>(C, 4);
                ++levels;
            }
        }
        uint32_t* part[2] = {nullptr, nullptr};
        int32_t* ssum[2] = {nullptr, nullptr};
        int64_t *cstart[2] = {nullptr, nullptr}, *coff = nullptr;
        OrderScope order_(pk->order, s);
        if (levels) {
            const size_t rb = rows_max * W * 4;
            pk->seg_partial.ensure(2 * rb);
            part[0] = pk->seg_partial.as<uint32_t>();
            part[1] = part[0] + rows_max * W;
            const size_t n64 = 2 * (S + 1) + (rows_max + 1), n32 = 2 * rows_max;
            pk->seg_plan.ensure(n64 * 8 + n32 * 4);
            cstart[0] = pk->seg_plan.as<int64_t>();
            cstart[1] = cstart[0] + (S + 1);
            coff = cstart[1] + (S + 1);
            ssum[0] = reinterpret_cast<int32_t*>(coff + rows_max + 1);
            ssum[1] = ssum[0] + rows_max;
        }
        int* status = status_word(pk, s);
        auto chains = [&](const uint32_t* ct, size_t n, int tg, const uint32_t* rows, const int32_t* sh, const int64_t* off, size_t count,
                          uint32_t* out, int32_t* shift_sum) {
            SegArgs A;
            A.ct = ct; A.rows = rows; A.shift = sh; A.offsets = off; A.out = out; A.shift_sum = shift_sum; A.status = status;
            A.n = (int)n; A.tag = tg; A.chains = (int)count;
            ScopedKernelTimer t("k_segprod", s);
            g->segprod(s, grid_for(g, count, pk->dev.ncu), pk->msq.d_ctx, A, pk->ct_words, rpow);
            t.stop();
            HIP_CHECK(hipGetLastError());
        };
        const uint32_t* ct = d_ct;
        const uint32_t* rows = d_rows;
        const int32_t* sh = d_shift;
        const int64_t* off = d_offsets;
        size_t n = N, m = M, c = C;
        int tg = tag;
        for (size_t lev = 0; lev < levels; ++lev) {
            const int b = (int)(lev & 1);
            const size_t mn = std::min(m, m / c + S);              // chains of this level (the chunks; the tail of them empty)
            hipLaunchKernelGGL(k_seg_chunk_scan, dim3(1), dim3(SEG_PLAN_THREADS), 0, s, off, (int)S, (int64_t)c, cstart[b]);
            HIP_CHECK(hipGetLastError());
            const int eg = (int)std::min<size_t>((mn + 1 + 255) / 256, 1024);
            hipLaunchKernelGGL(k_seg_chunk_expand, dim3(eg), dim3(256), 0, s, off, cstart[b], (int)S, (int64_t)c, coff, mn);
            HIP_CHECK(hipGetLastError());
            chains(ct, n, tg, rows, sh, coff, mn, part[b], ssum[b]);
            ct = part[b]; n = mn; tg = 0; rows = nullptr; sh = ssum[b]; off = cstart[b];
            m = mn;
            c = std::min<size_t>(C, 4) < 2 ? 2 : std::min<size_t>(C, 4);
        }
        chains(ct, n, tg, rows, sh, off, S, d_out, nullptr);
        order_.done();
}

int pai_ct_segment_prod(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, const uint32_t* d_rows, const int32_t* d_shift,
                        const int64_t* d_offsets, size_t S, uint32_t* d_out, void* stream) {
    return guarded([&] {
        require(pk && d_offsets && d_out, "NULL argument");
        require(std::abs(tag) <= RPOW_SPAN - 2, "pai_ct_segment_prod: domain tag out of range");
        require(N < ((size_t)1 << 31) && S < ((size_t)1 << 30), "pai_ct_segment_prod: too many rows or segments for one call");
        if (S == 0) return;
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        g_last_times.clear();
        segment_prod_locked(pk, (hipStream_t)stream, d_ct, N, tag, d_rows, d_shift, d_offsets, S, d_out);
    });
}

// Sparse matrix products (PaillierEncryptedNumber.csr_matmul / csr_rmatmul, extension): T terms (base[t], e[t], sign[t]) in
// segment order, out[s] = prod over the terms of segment s of (ct or ct_inv)[base[t]]^e[t].  Three stages:
//   1. tables: k_mexp_table_padic / k_mexp_table over the N bases (one table per base and sign, shared by all its terms);
//   2. terms: the segment offsets made safe (k_smexp_offsets), cut into chunks of <= C terms (k_seg_chunk_scan / _expand), one
//      Straus chain per chunk into a partial (k_smexp_padic / k_smexp);
//   3. combine: the partials of a segment multiplied by the levels of pai_ct_segment_prod at shift 0 (an empty segment gives 1).
// The chunk plan a sparse product ran on (valid until the handle's next sparse product): pai_opening_fold folds r and m over the same chunks
struct SmexpPlan {
    const int64_t* cstart = nullptr;   // [S + 1] chunks before every segment
    const int64_t* coff = nullptr;     // [nlanes + 1] first term of every chunk
    size_t nlanes = 0, chunk = 0;
};
// The three stages, under pk->mu on the key's device; S > 0.  chunk_force != 0 sets the terms per lane (pai_opening_fold's open_chunk).
static void sparse_multiexp_locked(const pai_pubkey* pk, hipStream_t s, const uint32_t* d_ct, const uint32_t* d_ct_inv, size_t N,
                                   const int32_t* d_base, const uint32_t* d_e, int e_words, int ebits_max, const uint8_t* d_sign, size_t T,
                                   const int64_t* d_offsets, size_t S, uint32_t* d_out, size_t chunk_force = 0, SmexpPlan* plan = nullptr) {
    const GeoOps* lg = pk->msq.geo;                   // lane-group engine when the digit engine does not serve the key
    const bool digit = pk->penc_nl != 0;
    const int nsigns = d_sign ? 2 : 1;
    const int pnl = digit ? pk->penc_nl : (lg->nl + 1) / 2;
    const int lanes_per_wg = digit ? BLOCK_THREADS : lg->epb;
    size_t want_lanes = (size_t)pk->dev.ncu * lanes_per_wg * (digit ? 2 : 4);
    if (long long v; knob_tune("mexp_lanes", &v) && v > 0) want_lanes = (size_t)v;
    const size_t C = chunk_force ? chunk_force : smexp_chunk(want_lanes, T);      // path_ranges.hpp
    // chunks: at most ceil(len / C) per segment, i.e. <= T / C + (nonempty segments); the tail of them empty
    const size_t nlanes = T == 0 ? 0 : std::min(T, T / C + std::min(S, T));
    size_t mem_free = 0, mem_total = 0;
    HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
    // window width: as pai_ct_multiexp, with the table cost of a base amortised over its T / N terms
    int wbits = 2;
    {
        double best = 1e300;
        const double uses = N ? std::max(1.0, (double)T / (double)N) : 1.0;
        for (int w = 2; w <= 7; ++w) {
            const double tb = (double)N * nsigns * (double)((size_t)1 << w) * 2.0 * pnl * 4.0;
            if (w > 2 && tb > (double)mem_total / 16.0) break;
            const double cost = (double)((ebits_max + w - 1) / w) + (double)nsigns * (double)(((size_t)1 << w) - 2) / uses;
            if (cost < best) { best = cost; wbits = w; }
        }
        if (long long v; knob_tune("mexp_wbits", &v) && v >= 1 && v <= 8) wbits = (int)v;
    }
    const size_t table_bytes = N * nsigns * ((size_t)1 << wbits) * 2 * (size_t)pnl * 4;
    const size_t part_bytes = nlanes * (size_t)pk->ct_words * 4;
    if (T && (table_bytes > mem_total / 8 ||
              table_bytes + part_bytes > mem_free + pk->mexp_table.bytes + pk->mexp_partial.bytes))
        throw PaiError(PAI_E_UNSUPPORTED, "power tables of this sparse product do not fit the device");
    // plan scratch: clean offsets [S + 1], chunk starts per segment [S + 1], first term per chunk [nlanes + 1]
    pk->smexp_plan.ensure((2 * (S + 1) + nlanes + 1) * sizeof(int64_t));
    int64_t* clean = pk->smexp_plan.as<int64_t>();
    int64_t* cstart = clean + (S + 1);
    int64_t* coff = cstart + (S + 1);
    int* status = status_word(pk, s);
    {
        OrderScope order_(pk->order, s);
        hipLaunchKernelGGL(k_smexp_offsets, dim3(1), dim3(SEG_PLAN_THREADS), 0, s, d_offsets, (int)S, (int64_t)T, clean, status);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_seg_chunk_scan, dim3(1), dim3(SEG_PLAN_THREADS), 0, s, clean, (int)S, (int64_t)C, cstart);
        HIP_CHECK(hipGetLastError());
        if (nlanes) {
            pk->mexp_table.ensure(table_bytes);
            pk->mexp_partial.ensure(part_bytes);
            const int eg = (int)std::min<size_t>((nlanes + 1 + 255) / 256, 1024);
            hipLaunchKernelGGL(k_seg_chunk_expand, dim3(eg), dim3(256), 0, s, clean, cstart, (int)S, (int64_t)C, coff, nlanes);
            HIP_CHECK(hipGetLastError());
            SmexpArgs A;
            A.base = d_base; A.coff = coff; A.status = status; A.nbases = (int)N;
            if (digit) {
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
                Q.R = 1; Q.K = (int)N; Q.M = 1; Q.chunk = (int)C; Q.nsigns = nsigns;
                Q.e_words = e_words;
                Q.ebits_max = ebits_max;
                Q.by_rows = 0;
                Q.wbits = wbits;
                if (N) {
                    const size_t tl = N * nsigns, tiles = (tl + BLOCK_THREADS - 1) / BLOCK_THREADS;
                    const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
                    ScopedKernelTimer t("k_mexp_table", s);
                    launcher(padic_enc_ops(pnl), &PadicEncOps::mexp_table, "no multi-exponentiation kernel for this limb count")(
                        s, grid, Q, d_ct, d_ct_inv, (int)tl);
                    t.stop();
                    HIP_CHECK(hipGetLastError());
                }
                {
                    const size_t tiles = (nlanes + BLOCK_THREADS - 1) / BLOCK_THREADS;
                    const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
                    ScopedKernelTimer t("k_smexp", s);
                    launcher(padic_enc_ops(pnl), &PadicEncOps::smexp, "no multi-exponentiation kernel for this limb count")(
                        s, grid, Q, A, d_e, d_sign, pk->mexp_partial.as<uint32_t>(), (int)nlanes);
                    t.stop();
                    HIP_CHECK(hipGetLastError());
                }
            } else {
                MexpParams P;
                P.R = 1; P.K = (int)N; P.M = 1; P.chunk = (int)C; P.nsigns = nsigns;
                P.e_words = e_words; P.ebits_max = ebits_max; P.wbits = wbits; P.w32 = pk->ct_words;
                if (N) {
                    const size_t tl = N * nsigns;
                    ScopedKernelTimer t("k_mexp_table", s);
                    lg->mexp_table(s, grid_for(lg, tl, pk->dev.ncu), pk->msq.d_ctx, d_ct, d_ct_inv, pk->ct_words, pk->mexp_table.as<uint32_t>(),
                                   (int)tl, nsigns, wbits);
                    t.stop();
                    HIP_CHECK(hipGetLastError());
                }
                {
                    ScopedKernelTimer t("k_smexp", s);
                    lg->smexp(s, grid_for(lg, nlanes, pk->dev.ncu), pk->msq.d_ctx, P, A, pk->mexp_table.as<uint32_t>(), d_e, d_sign,
                              pk->mexp_partial.as<uint32_t>(), (int)nlanes);
                    t.stop();
                    HIP_CHECK(hipGetLastError());
                }
            }
        }
        order_.done();
    }
    // the partials of segment s are rows cstart[s] .. cstart[s + 1] - 1, in the wire form (tag 0), all at shift 0
    segment_prod_locked(pk, s, nlanes ? pk->mexp_partial.as<uint32_t>() : nullptr, nlanes, 0, nullptr, nullptr, cstart, S, d_out);
    if (plan) { plan->cstart = cstart; plan->coff = coff; plan->nlanes = nlanes; plan->chunk = C; }
}

int pai_ct_sparse_multiexp(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_ct_inv, size_t N, const int32_t* d_base,
                           const uint32_t* d_e, int e_words, int ebits_max, const uint8_t* d_sign, size_t T, const int64_t* d_offsets,
                           size_t S, uint32_t* d_out, void* stream) {
    return guarded([&] {
        require(pk && d_offsets && d_out, "NULL argument");
        require(T == 0 || (d_ct && d_base && d_e), "NULL argument");
        require(T == 0 || N > 0, "pai_ct_sparse_multiexp: terms without bases");
        require(e_words > 0 && ebits_max > 0 && ebits_max <= 32 * e_words, "bad shape");
        require((d_sign == nullptr) == (d_ct_inv == nullptr), "signs and inverses come together");
        if (T >= ((size_t)1 << 31) || N >= ((size_t)1 << 28) || S >= ((size_t)1 << 30))
            throw PaiError(PAI_E_UNSUPPORTED, "sparse product too large for one call");
        if (S == 0) return;
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        g_last_times.clear();
        sparse_multiexp_locked(pk, (hipStream_t)stream, d_ct, d_ct_inv, N, d_base, d_e, e_words, ebits_max, d_sign, T, d_offsets, S, d_out);
    });
}

// Multi-exponentiation behind the matrix products (kernels_padic_enc.hpp: k_mexp_table_padic, k_mexp_padic)
int pai_ct_multiexp(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_ct_inv, size_t R, size_t K, size_t M,
                    const uint32_t* d_e, int e_words, int ebits_max, const uint8_t* d_sign, uint32_t* d_out, void* stream) {
    return guarded([&] {
        require(pk && d_ct && d_e && d_out, "NULL argument");
        require(R > 0 && K > 0 && M > 0 && e_words > 0 && ebits_max > 0 && ebits_max <= 32 * e_words, "bad shape");
        require((d_sign == nullptr) == (d_ct_inv == nullptr), "signs and inverses come together");
        const size_t G = R * M, bases = R * K;
        if (G * K >= ((size_t)1 << 31) || bases >= ((size_t)1 << 28)) throw PaiError(PAI_E_UNSUPPORTED, "matrix product too large for one call");
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        const GeoOps* lg = pk->msq.geo;                   // lane-group engine when the digit engine does not serve the key
        const bool digit = pk->penc_nl != 0;
        const int nsigns = d_sign ? 2 : 1;
        // words of one table entry: a digit pair of 2 pnl limbs, or a Montgomery residue of nl limbs
        const int pnl = digit ? pk->penc_nl : (lg->nl + 1) / 2;
        const int lanes_per_wg = digit ? BLOCK_THREADS : lg->epb;
        // members per lane: enough lanes to fill the device (one workgroup of 256 lanes per CU, several rounds), the
        // rest of the sharing goes into longer chunks (the squarings are shared by a chunk)
        size_t want_lanes = (size_t)pk->dev.ncu * lanes_per_wg * (digit ? 2 : 4);
        if (long long v; knob_tune("mexp_lanes", &v) && v > 0) want_lanes = (size_t)v;
        size_t chunk = std::max<size_t>(1, (G * K + want_lanes - 1) / want_lanes);
        chunk = std::min(chunk, K);
        const size_t chunks = (K + chunk - 1) / chunk;
        const size_t nlanes = chunks * G;
        size_t mem_free = 0, mem_total = 0;
        HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
        // window width: a term costs ebits / w table products and every base (2^w - 2) products per sign for its table,
        // which M output columns share; the widest tables must fit 1/16 of the device memory
        int wbits = 2;
        {
            double best = 1e300;
            for (int w = 2; w <= 7; ++w) {
                const double tb = (double)bases * nsigns * (double)((size_t)1 << w) * 2.0 * pnl * 4.0;
                if (w > 2 && tb > (double)mem_total / 16.0) break;
                const double cost = (double)((ebits_max + w - 1) / w) + (double)nsigns * (double)(((size_t)1 << w) - 2) / (double)M;
                if (cost < best) { best = cost; wbits = w; }
            }
            if (long long v; knob_tune("mexp_wbits", &v) && v >= 1 && v <= 8) wbits = (int)v;
        }
        const size_t table_bytes = bases * nsigns * ((size_t)1 << wbits) * 2 * (size_t)pnl * 4;
        if (table_bytes > mem_total / 8 || table_bytes + nlanes * (size_t)pk->ct_words * 4 > mem_free + pk->mexp_table.bytes + pk->mexp_partial.bytes)
            throw PaiError(PAI_E_UNSUPPORTED, "power tables of this matrix product do not fit the device");
        pk->mexp_table.ensure(table_bytes);
        pk->mexp_partial.ensure(nlanes * (size_t)pk->ct_words * 4);
        g_last_times.clear();
        OrderScope order_(pk->order, s);
        if (digit) {
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
            Q.R = (int)R; Q.K = (int)K; Q.M = (int)M; Q.chunk = (int)chunk; Q.nsigns = nsigns;
            Q.e_words = e_words;
            Q.ebits_max = ebits_max;
            Q.by_rows = 0;
            Q.wbits = wbits;
            if (long long v; knob_tune("mexp_by_rows", &v)) Q.by_rows = v != 0;
            {
                const size_t tl = bases * nsigns, tiles = (tl + BLOCK_THREADS - 1) / BLOCK_THREADS;
                const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
                ScopedKernelTimer t("k_mexp_table", s);
                launcher(padic_enc_ops(pnl), &PadicEncOps::mexp_table, "no multi-exponentiation kernel for this limb count")(
                    s, grid, Q, d_ct, d_ct_inv, (int)tl);
                t.stop();
                HIP_CHECK(hipGetLastError());
            }
            {
                const size_t tiles = (nlanes + BLOCK_THREADS - 1) / BLOCK_THREADS;
                const int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
                ScopedKernelTimer t("k_mexp", s);
                launcher(padic_enc_ops(pnl), &PadicEncOps::mexp, "no multi-exponentiation kernel for this limb count")(
                    s, grid, Q, d_e, d_sign, pk->mexp_partial.as<uint32_t>(), (int)nlanes);
                t.stop();
                HIP_CHECK(hipGetLastError());
            }
        } else {
            // lane-group engine (keys above 2048 bits): Montgomery residues modulo n^2 as table entries
            MexpParams P;
            P.R = (int)R; P.K = (int)K; P.M = (int)M; P.chunk = (int)chunk; P.nsigns = nsigns;
            P.e_words = e_words; P.ebits_max = ebits_max; P.wbits = wbits; P.w32 = pk->ct_words;
            {
                const size_t tl = bases * nsigns;
                ScopedKernelTimer t("k_mexp_table", s);
                lg->mexp_table(s, grid_for(lg, tl, pk->dev.ncu), pk->msq.d_ctx, d_ct, d_ct_inv, pk->ct_words, pk->mexp_table.as<uint32_t>(),
                               (int)tl, nsigns, wbits);
                t.stop();
                HIP_CHECK(hipGetLastError());
            }
            {
                ScopedKernelTimer t("k_mexp", s);
                lg->mexp(s, grid_for(lg, nlanes, pk->dev.ncu), pk->msq.d_ctx, P, pk->mexp_table.as<uint32_t>(), d_e, d_sign,
                         pk->mexp_partial.as<uint32_t>(), (int)nlanes);
                t.stop();
                HIP_CHECK(hipGetLastError());
            }
        }
        order_.done();
        ct_prod_locked(pk, s, pk->mexp_partial.as<uint32_t>(), nlanes, G, d_out, false);
    });
}

static int ct_invert_impl(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream, bool sync, int* d_flag);
int pai_ct_invert(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream) {
    return ct_invert_impl(pk, d_ct, N, d_out, stream, true, nullptr);
}
int pai_ct_invert_async(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream) {
    return ct_invert_impl(pk, d_ct, N, d_out, stream, false, nullptr);
}
int pai_ct_invert_flag(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, int32_t* d_flag, void* stream) {
    if (!d_flag) return guarded([&] { require(false, "NULL argument"); });
    return ct_invert_impl(pk, d_ct, N, d_out, stream, false, d_flag);
}
int pai_pubkey_status(const pai_pubkey* pk, int* status_out, int clear, void* stream) {
    return guarded([&] {
        require(pk && status_out, "NULL argument");
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        int* w = status_word(pk, s);
        int v = 0;
        HIP_CHECK(hipMemcpyAsync(&v, w, 4, hipMemcpyDeviceToHost, s));
        if (clear) HIP_CHECK(hipMemsetAsync(w, 0, 4, s));
        HIP_CHECK(hipStreamSynchronize(s));
        *status_out = v;
    });
}

static int ct_invert_impl(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream, bool sync, int* d_flag) {
    return guarded([&] {
        require(pk && d_ct && d_out, "NULL argument");
        if (N == 0) return;
        require_no_overlap(d_out, N * (size_t)pk->ct_words * 4, d_ct, N * (size_t)pk->ct_words * 4, true,
                           "ct_invert: d_out overlaps d_ct (an output may be exactly an operand, nothing else)");
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        const size_t W = (size_t)pk->ct_words, ROW = W * 4;
        // product tree over halves (kernels_invert.hpp): level k + 1 has ceil(count_k / 2) products; the tree stops
        // at <= `top` values, each inverted by one wave's extended GCD.  Every tree product is ONE Montgomery
        // product: level k holds (true value) * R^(1 - 2^k) on the way up (a value without a partner is brought to
        // its level's form by the constant tree_c[k]); the extended GCD inverts the stored top values, and on the
        // way down level k holds (true inverse) * R^(2^k - 1) — the powers of R telescope, so the leaves come out as
        // plain canonical inverses.
        size_t top = 64;
        if (long long v; knob_tune("invert_chunk", &v) && v >= 1 && v <= 65536) top = (size_t)v;     // test hook: where the tree stops
        std::vector<size_t> cnt{N};
        while (cnt.back() > top) cnt.push_back((cnt.back() + 1) / 2);
        const int L = (int)cnt.size() - 1;
        require(L < pai_pubkey::TREE_LEVELS, "ct_invert: too many levels");
        size_t upper = 0;                                              // rows of all levels above the leaves
        std::vector<size_t> off(L + 1, 0);
        for (int k = 1; k <= L; ++k) { off[k] = upper; upper += cnt[k]; }
        const bool alias = (d_out == d_ct);
        pk->inv_prod.ensure(std::max<size_t>(1, upper + (alias ? N : 0)) * ROW);
        pk->inv_inv.ensure(std::max<size_t>(1, upper + (L == 0 ? N : 0)) * ROW);
        pk->inv_fail.ensure(4);
        OrderScope order_(pk->order, s);
        HIP_CHECK(hipMemsetAsync(pk->inv_fail.p, 0, 4, s));
        uint32_t* prod = pk->inv_prod.as<uint32_t>();
        uint32_t* inv = pk->inv_inv.as<uint32_t>();
        const uint32_t* leaves = d_ct;
        if (alias) {                                                    // the way down reads both halves after writing one
            uint32_t* copy = prod + upper * W;
            HIP_CHECK(hipMemcpyAsync(copy, d_ct, N * ROW, hipMemcpyDeviceToDevice, s));
            leaves = copy;
        }
        auto level = [&](int k) -> const uint32_t* { return k == 0 ? leaves : prod + off[k] * W; };
        auto tree_c = [&](int k) -> const uint32_t* { return pk->d_tree_c + (size_t)k * W; };
        g_last_times.clear();
        ScopedKernelTimer t("k_invert", s);
        for (int k = 0; k < L; ++k) {                                   // up
            const size_t h = cnt[k + 1], lo = cnt[k] - h;
            const uint32_t* src = level(k);
            uint32_t* dst = prod + off[k + 1] * W;
            tree_mul(pk, s, src, src + h * W, 0, dst, lo);
            if (lo < h) tree_mul(pk, s, src + lo * W, tree_c(k), 1, dst + lo * W, 1);
        }
        uint32_t* top_out = (L == 0) ? d_out : inv + off[L] * W;
        if (L == 0 && alias) top_out = inv;                             // in-place single level: stage, then copy back
        if (!launch_inv_eea(s, (int)W, pk->d_nsq_words, level(L), top_out, (int)cnt[L], 2 * 32 * (int)W + 64, pk->inv_fail.as<int>()))
            throw PaiError(PAI_E_UNSUPPORTED, "ct_invert: key size without an extended-GCD instantiation");
        HIP_CHECK(hipGetLastError());
        if (L == 0 && alias) HIP_CHECK(hipMemcpyAsync(d_out, inv, N * ROW, hipMemcpyDeviceToDevice, s));
        for (int k = L - 1; k >= 0; --k) {                              // down
            const size_t h = cnt[k + 1], lo = cnt[k] - h;
            const uint32_t* src = level(k);
            const uint32_t* pinv = inv + off[k + 1] * W;
            uint32_t* dst = (k == 0) ? d_out : inv + off[k] * W;
            tree_mul(pk, s, pinv, src + h * W, 0, dst, lo);             // a[i]^-1     = P[i]^-1 a[i + h]
            tree_mul(pk, s, pinv, src, 0, dst + h * W, lo);             // a[i + h]^-1 = P[i]^-1 a[i]
            if (lo < h) tree_mul(pk, s, pinv + lo * W, tree_c(k), 1, dst + lo * W, 1);
        }
        t.stop();
        if (!sync) {
            // asynchronous forms: a non-unit is remembered in the caller's flag word (pai_ct_invert_flag: the outcome travels
            // with the result) or in the handle's sticky status word (pai_ct_invert_async + pai_pubkey_status)
            hipLaunchKernelGGL(k_status_or, dim3(1), dim3(1), 0, s, d_flag ? d_flag : status_word(pk, s), pk->inv_fail.as<int>(), 1);
            HIP_CHECK(hipGetLastError());
            order_.done();
            return;
        }
        int fail = 0;
        HIP_CHECK(hipMemcpyAsync(&fail, pk->inv_fail.p, 4, hipMemcpyDeviceToHost, s));
        order_.done();
        HIP_CHECK(hipStreamSynchronize(s));
        if (fail) throw PaiError(PAI_E_INVALID, "ct_invert: a ciphertext is not invertible modulo n^2");
    });
}
