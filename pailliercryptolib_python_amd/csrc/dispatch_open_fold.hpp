// pai_opening_fold: the two sides of the small-exponent batch test of ciphertext openings.  For segments of seg_len
// consecutive rows,  lhs[s] = prod ct_i^(e_i) mod n^2  and  rhs[s] = (1 + n M_s) B_s^n mod n^2  with  M_s = sum e_i m_i mod n,
// B_s = prod r_i^(e_i) mod n — one exponentiation by n per segment instead of one per row.  Two routes, bit-identical results:
//   fused        (keys the digit engine serves)  lhs by the sparse multi-exponentiation with the identity term list; B and M parts per
//                chunk of the SAME chunk plan by k_open_fold (arithmetic modulo n: kernels_open_fold.hpp); M parts -> 1 + n M by the raw
//                encryption; both combined per segment by the k_segprod levels at shift 0 (products modulo n^2 of residues modulo n keep
//                the residue modulo n, and prod (1 + n M_k) = 1 + n sum M_k)
//   composition  (wider keys, PAI_DISABLE=open_fold)  three sparse multi-exponentiations modulo n^2: over the ciphertexts, over the r rows
//                zero-extended, over the raw encryptions of m
// then B_s^n by pai_ct_mul with the broadcast exponent n (its small-batch routes serve the few segments), times 1 + n M_s by pai_ct_add,
// and the unit test of B_s by pai_ct_invert_flag.
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once

static void open_sub(int rc) {                         // a stage that is a public call of its own: its error is this call's
    if (rc != PAI_OK) throw PaiError(rc, g_err);
}

// segments [s0, s1) of the call: rows r0 .. r0 + n - 1
static void opening_fold_block(const pai_pubkey* pk, hipStream_t s, const uint32_t* d_ct, const uint32_t* d_m, const uint32_t* d_r, size_t n,
                               const uint32_t* d_e, int e_words, int ebits_max, size_t seg_len, size_t Sb, uint32_t* d_lhs, uint32_t* d_rhs,
                               int32_t* d_flag, bool fused, std::vector<KernelTime>& times) {
    const size_t W = (size_t)pk->ct_words, NW = (size_t)pk->n_words;
    // PAI_E_UNSUPPORTED from here or from a stage's table sizing is not the call's answer: pai_opening_fold halves the block and comes
    // again (the sparse product's limit of 2^28 bases included).  PAI_TUNE open_block_rows (test hook): most rows of a block of several
    // segments, so that a small batch runs through the halving; a single segment runs whole whatever its length.
    if (n >= ((size_t)1 << 28)) throw PaiError(PAI_E_UNSUPPORTED, "opening fold too large for one block");
    if (long long cap; knob_tune("open_block_rows", &cap) && cap >= 1 && Sb > 1 && n > (size_t)cap)
        throw PaiError(PAI_E_UNSUPPORTED, "opening fold: block above open_block_rows");
    auto keep = [&] {
        times.insert(times.end(), g_last_times.begin(), g_last_times.end());
        g_last_times.clear();
    };
    // plan scratch: off [Sb + 1] | cstart copy [Sb + 1] | coff copy [n + 1] | base [n]
    int64_t *off = nullptr, *cstart = nullptr, *coff = nullptr;
    int32_t* base = nullptr;
    uint32_t *Bs = nullptr, *Es = nullptr, *Bn = nullptr;
    size_t nlanes = 0;
    {
        std::lock_guard<std::mutex> lk(pk->mu);
        pk->open_plan.ensure((2 * (Sb + 1) + n + 1) * sizeof(int64_t) + n * sizeof(int32_t));
        off = pk->open_plan.as<int64_t>();
        cstart = off + (Sb + 1);
        coff = cstart + (Sb + 1);
        base = reinterpret_cast<int32_t*>(coff + n + 1);
        pk->open_rows.ensure(3 * Sb * W * 4);
        Bs = pk->open_rows.as<uint32_t>();
        Es = Bs + Sb * W;
        Bn = Es + Sb * W;
        OrderScope order_(pk->order, s);
        hipLaunchKernelGGL(k_open_plan, dim3((unsigned)std::min<size_t>((std::max(n, Sb + 1) + 255) / 256, 1024)), dim3(256), 0, s, (int64_t)n,
                           (int64_t)seg_len, (int)Sb, off, base);
        HIP_CHECK(hipGetLastError());
        long long v;
        const size_t chunk_force = knob_tune("open_chunk", &v) && v >= 1 ? (size_t)v : 0;
        SmexpPlan plan;
        sparse_multiexp_locked(pk, s, d_ct, nullptr, n, base, d_e, e_words, ebits_max, nullptr, n, off, Sb, d_lhs, chunk_force, &plan);
        if (fused) {
            nlanes = plan.nlanes;
            require(nlanes >= 1 && nlanes <= n && plan.chunk >= 1 && plan.chunk < ((size_t)1 << 30), "opening fold: bad chunk plan");
            // the plan lives in the sparse product's scratch: copied, the next sparse product of this handle may come before the M parts' combine
            HIP_CHECK(hipMemcpyAsync(cstart, plan.cstart, (Sb + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
            HIP_CHECK(hipMemcpyAsync(coff, plan.coff, (nlanes + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
            const size_t tiles = (nlanes + BLOCK_THREADS - 1) / BLOCK_THREADS;
            int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
            if (knob_tune("open_grid", &v) && v >= 1) grid = (int)std::min<long long>(grid, v);      // test hook: a small batch walks the tile loop
            int wbits = 2;
            if (knob_tune("open_wbits", &v) && v >= 1 && v <= 4) wbits = (int)v;
            size_t mem_free = 0, mem_total = 0;
            HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
            size_t tb = open_fold_table_bytes(pk->penc_nl, (int)plan.chunk, wbits, (size_t)grid);
            if (tb > mem_total / 8) {                      // bit-serial: one table entry per member
                wbits = 1;
                tb = open_fold_table_bytes(pk->penc_nl, (int)plan.chunk, wbits, (size_t)grid);
            }
            if (tb > mem_total / 8 || tb > mem_free + pk->open_table.bytes)
                throw PaiError(PAI_E_UNSUPPORTED, "power tables of this opening fold do not fit the device");
            pk->open_table.ensure(tb);
            pk->open_parts.ensure(nlanes * (2 * W + NW) * 4);
            uint32_t* Bp = pk->open_parts.as<uint32_t>();          // B parts | 1 + n M parts | M parts
            uint32_t* Mp = Bp + 2 * nlanes * W;
            OpenFoldParams Q;
            Q.nctx = pk->nmod.d_ctx;
            Q.mscratch = reinterpret_cast<uint4*>(pk->d_mscratch);
            Q.table = pk->open_table.as<uint4>();
            Q.coff = coff;
            Q.n_words = pk->n_words;
            Q.ct_words = pk->ct_words;
            Q.chunk = (int)plan.chunk;
            Q.e_words = e_words;
            Q.ebits_max = ebits_max;
            Q.wbits = wbits;
            {
                ScopedKernelTimer t("k_open_fold", s, "padic");
                if (!launch_open_fold(pk->penc_nl, s, grid, Q, d_r, d_m, d_e, Bp, Mp, (int)nlanes))
                    throw PaiError(PAI_E_INTERNAL, "no opening-fold kernel for this limb count");
                t.stop();
                HIP_CHECK(hipGetLastError());
            }
            segment_prod_locked(pk, s, Bp, nlanes, 0, nullptr, nullptr, cstart, Sb, Bs);
        } else {
            pk->open_wide.ensure(n * W * 4);
            hipLaunchKernelGGL(k_open_widen, dim3((unsigned)std::min<size_t>((n * W + 255) / 256, 4096)), dim3(256), 0, s, d_r, pk->n_words,
                               pk->open_wide.as<uint32_t>(), pk->ct_words, n);
            HIP_CHECK(hipGetLastError());
            sparse_multiexp_locked(pk, s, pk->open_wide.as<uint32_t>(), nullptr, n, base, d_e, e_words, ebits_max, nullptr, n, off, Sb, Bs,
                                   chunk_force);
        }
        order_.done();
    }
    keep();
    // 1 + n M: per chunk (fused) or per row (composition), then the product per segment
    if (fused) {
        uint32_t* Bp = pk->open_parts.as<uint32_t>();
        uint32_t* Ep = Bp + nlanes * W;
        uint32_t* Mp = Ep + nlanes * W;
        open_sub(pai_raw_encrypt(pk, Mp, nlanes, Ep, s));
        keep();
        std::lock_guard<std::mutex> lk(pk->mu);
        segment_prod_locked(pk, s, Ep, nlanes, 0, nullptr, nullptr, cstart, Sb, Es);
    } else {
        open_sub(pai_raw_encrypt(pk, d_m, n, pk->open_wide.as<uint32_t>(), s));
        keep();
        std::lock_guard<std::mutex> lk(pk->mu);
        long long v;
        const size_t chunk_force = knob_tune("open_chunk", &v) && v >= 1 ? (size_t)v : 0;
        sparse_multiexp_locked(pk, s, pk->open_wide.as<uint32_t>(), nullptr, n, base, d_e, e_words, ebits_max, nullptr, n, off, Sb, Es, chunk_force);
    }
    keep();
    // the one full-width exponentiation per segment, the product of the two factors, the unit test of B_s
    open_sub(pai_ct_mul(pk, Bs, pk->d_nexp, pk->n_words, hbn::bitlen(pk->n), 1, Sb, Bn, s));
    keep();
    open_sub(pai_ct_add(pk, Bn, Es, 0, Sb, d_rhs, s));
    keep();
    open_sub(pai_ct_invert_flag(pk, Bs, Sb, Bn, d_flag, s));
    keep();
}

int pai_opening_fold(const pai_pubkey* pk, const uint32_t* d_ct, const uint32_t* d_m, const uint32_t* d_r, size_t N, const uint32_t* d_e,
                     int e_words, int ebits_max, size_t seg_len, uint32_t* d_lhs, uint32_t* d_rhs, int32_t* d_flag, void* stream) {
    return guarded([&] {
        require(pk && d_flag, "NULL argument");
        require(N == 0 || (d_ct && d_m && d_r && d_e && d_lhs && d_rhs), "NULL argument");
        require(e_words >= 1 && e_words <= 8 && ebits_max > 0 && ebits_max <= 32 * e_words, "pai_opening_fold: bad coefficient shape");
        require(seg_len >= 1, "pai_opening_fold: empty segments");
        if (N == 0) return;
        const size_t S = (N + seg_len - 1) / seg_len;
        const size_t W = (size_t)pk->ct_words;
        std::lock_guard<std::mutex> open_lk(pk->open_mu);
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        const bool fused = pk->penc_nl != 0 && !knob_disabled("open_fold");
        std::vector<KernelTime> times;
        g_last_times.clear();
        // row blocks on segment boundaries: a block whose power tables do not fit the device is halved
        size_t per = S;
        for (size_t s0 = 0; s0 < S;) {
            const size_t s1 = std::min(S, s0 + per), r0 = s0 * seg_len, r1 = std::min(N, s1 * seg_len);
            try {
                opening_fold_block(pk, s, d_ct + r0 * W, d_m + r0 * (size_t)pk->n_words, d_r + r0 * (size_t)pk->n_words, r1 - r0,
                                   d_e + r0 * (size_t)e_words, e_words, ebits_max, seg_len, s1 - s0, d_lhs + s0 * W, d_rhs + s0 * W, d_flag, fused,
                                   times);
            } catch (const PaiError& err) {
                if (err.code != PAI_E_UNSUPPORTED || s1 - s0 <= 1) throw;
                per = (s1 - s0 + 1) / 2;
                g_last_times.clear();
                continue;
            }
            s0 = s1;
        }
        {   // the last stages ran outside the handle's scratch order: the next user of the fold's scratch on another stream waits for them
            std::lock_guard<std::mutex> lk(pk->mu);
            OrderScope order_(pk->order, s);
            order_.done();
        }
        // one profile entry per kernel name, the stages' times summed (several stages run k_smexp / k_segprod)
        g_last_times.clear();
        for (const KernelTime& t : times) {
            auto it = std::find_if(g_last_times.begin(), g_last_times.end(), [&](const KernelTime& u) { return u.name == t.name; });
            if (it == g_last_times.end()) g_last_times.push_back(t);
            else it->ms += t.ms;
        }
    });
}
