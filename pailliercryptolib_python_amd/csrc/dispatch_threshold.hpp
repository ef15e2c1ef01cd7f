// Threshold decryption: pai_keyshare_create / _destroy, pai_partial_decrypt, pai_threshold_combine.
//   partial   c^E for a share's exponent E = 2 Delta s_i: k_pow_padic on the share's own sliding-window schedule (digit-engine keys, from
//             tpart_min rows on), else the routes of pai_ct_mul with E as the broadcast exponent — the same bits
//   combine   P+ and P- (the members with positive / negative Lagrange coefficients) by k_tcomb_padic (digit-engine keys, from tcomb_min
//             rows on, PAI_DISABLE=tcombine not set) or by pai_ct_mul per part and pai_ct_addn per side; then pai_ct_invert_flag on P-,
//             pai_ct_add, and k_tfinish: (x - 1) / n with the test x = 1 (mod n), times theta modulo n
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once

struct pai_keyshare {
    const pai_pubkey* pk = nullptr;
    int device = 0;
    Limbs e;                      // the exponent (secret)
    int ebits = 0, e_words = 0;
    uint32_t* d_e = nullptr;      // its e_words little-endian words: the broadcast exponent of the pai_ct_mul routes
    uint16_t* d_ops = nullptr;    // its sliding-window schedule (compile_sliding_schedule) for k_pow_padic; digit-engine keys only
    int nops = 0;
};

void pai_keyshare_destroy(pai_keyshare* sh) {
    if (!sh) return;
    int prev_ = -1;
    (void)hipGetDevice(&prev_);
    (void)hipSetDevice(sh->device);
    (void)hipDeviceSynchronize();                             // nothing in flight may still read the exponent
    if (sh->d_e) {
        (void)hipMemset(sh->d_e, 0, (size_t)sh->e_words * 4);
        (void)hipFree(sh->d_e);
    }
    if (sh->d_ops) {
        (void)hipMemset(sh->d_ops, 0, (size_t)sh->nops * 2);
        (void)hipFree(sh->d_ops);
    }
    volatile uint32_t* w = sh->e.data();                      // volatile: the stores are not optimised away before the vector is freed
    for (size_t i = 0; i < sh->e.size(); ++i) w[i] = 0;
    if (prev_ >= 0) (void)hipSetDevice(prev_);
    delete sh;
}

int pai_keyshare_create(const pai_pubkey* pk, const uint32_t* h_e, int e_words, pai_keyshare** out) {
    return guarded([&] {
        require(pk && h_e && out, "NULL argument");
        require(e_words >= 1 && e_words <= 1024, "pai_keyshare_create: 1 <= e_words <= 1024");
        DeviceScope scope_(pk->device);
        struct Del { void operator()(pai_keyshare* p) const { pai_keyshare_destroy(p); } };
        std::unique_ptr<pai_keyshare, Del> sh(new pai_keyshare());
        sh->pk = pk;
        sh->device = pk->device;
        sh->e = hbn::from_u32(h_e, (size_t)e_words);
        require(!hbn::is_zero(sh->e), "pai_keyshare_create: the exponent is zero");
        sh->ebits = hbn::bitlen(sh->e);
        sh->e_words = words_for_bits(sh->ebits);
        sh->d_e = upload_words(sh->e, sh->e_words);
        if (pk->penc_nl) {
            std::vector<uint16_t> ops = compile_sliding_schedule(sh->e);
            sh->nops = (int)ops.size();
            HIP_CHECK(hipMalloc((void**)&sh->d_ops, ops.size() * 2));
            HIP_CHECK(hipMemcpy(sh->d_ops, ops.data(), ops.size() * 2, hipMemcpyHostToDevice));
            volatile uint16_t* w = ops.data();
            for (size_t i = 0; i < ops.size(); ++i) w[i] = 0;
        }
        *out = sh.release();
    });
}

int pai_partial_decrypt(pai_keyshare* sh, const uint32_t* d_ct, size_t N, uint32_t* d_out, void* stream) {
    const int rc = guarded([&] {
        require(sh && d_ct && d_out, "NULL argument");
        g_last_times.clear();
        if (N == 0) return;
        require(N <= (size_t)0x7fffffff, "pai_partial_decrypt: batch too large");
        const pai_pubkey* pk = sh->pk;
        require_no_overlap(d_out, N * (size_t)pk->ct_words * 4, d_ct, N * (size_t)pk->ct_words * 4, false,
                           "pai_partial_decrypt: d_out overlaps d_ct");
    });
    if (rc != PAI_OK || N == 0) return rc;
    const pai_pubkey* pk = sh->pk;
    if (!(pk->penc_nl && sh->d_ops && N >= tpart_min((size_t)pk->dev.ncu, pk->key_bits, hbn::bitlen(pk->n))))
        return pai_ct_mul(pk, d_ct, sh->d_e, sh->e_words, sh->ebits, 1, N, d_out, stream);
    return guarded([&] {
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        std::lock_guard<std::mutex> lk(pk->mu);
        const size_t tiles = (N + BLOCK_THREADS - 1) / BLOCK_THREADS;
        int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
        long long cap = 0;
        if (knob_tune("tpart_grid", &cap) && cap >= 1) grid = (int)std::min<long long>(grid, cap);     // a small batch then walks the tile loop
        pk->table.ensure(padic_table_words(pk->penc_nl, (size_t)grid) * 4);
        PowPadicParams Q;
        Q.nctx = pk->nmod.d_ctx;
        Q.nm1 = pk->d_nm1;
        Q.nsq = pk->d_nsq29;
        Q.kdig = pk->d_ct_kdig;
        Q.ops = sh->d_ops;
        Q.nops = sh->nops;
        Q.tbl_entries = PADIC_TBL_ENTRIES;
        Q.mscratch = reinterpret_cast<uint4*>(pk->d_mscratch);
        Q.table = pk->table.as<uint4>();
        Q.in_words = pk->ct_words;
        Q.ct_words = pk->ct_words;
        OrderScope order_(pk->order, s);
        ScopedKernelTimer t("k_pow_padic", s, "padic");
        launcher(padic_enc_ops(pk->penc_nl), &PadicEncOps::pow, "no digit-engine power kernel for this limb count")(s, grid, Q, d_ct, d_out,
                                                                                                                 (int)N);
        t.stop();
        HIP_CHECK(hipGetLastError());
        order_.done();
    });
}

int pai_threshold_combine(const pai_pubkey* pk, const uint32_t* const* h_parts, int t, const uint32_t* h_mu, const int32_t* h_neg,
                          int mu_words, const uint32_t* h_theta, size_t N, uint32_t* d_m, int32_t* d_flag, int32_t* d_rowflag,
                          void* stream) {
    return guarded([&] {
        require(pk && h_parts && h_mu && h_neg && h_theta && d_flag, "NULL argument");
        require(t >= 1 && t <= TCOMB_MAX_PARTS, "pai_threshold_combine: 1 <= t <= 16");
        require(mu_words >= 1 && mu_words <= TCOMB_MU_WORDS, "pai_threshold_combine: 1 <= mu_words <= 4");
        require(N <= (size_t)0x7fffffff, "pai_threshold_combine: batch too large");
        const size_t W = (size_t)pk->ct_words, NW = (size_t)pk->n_words;
        require(NW <= 256, "pai_threshold_combine: key too wide");
        uint32_t mu[TCOMB_MAX_PARTS][TCOMB_MU_WORDS] = {};
        int mu_bits[TCOMB_MAX_PARTS] = {};
        unsigned neg_mask = 0;
        for (int j = 0; j < t; ++j) {
            for (int k = 0; k < mu_words; ++k) mu[j][k] = h_mu[(size_t)j * mu_words + k];
            mu_bits[j] = hbn::bitlen(hbn::from_u32(mu[j], TCOMB_MU_WORDS));
            require(mu_bits[j] > 0, "pai_threshold_combine: a zero coefficient");
            if (h_neg[j]) neg_mask |= 1u << j;
            require(N == 0 || h_parts[j] != nullptr, "NULL argument");
        }
        const Limbs theta = hbn::from_u32(h_theta, NW);
        require(hbn::cmp(theta, pk->n) < 0, "pai_threshold_combine: theta is not a residue modulo n");
        g_last_times.clear();
        if (N == 0) return;
        require(d_m != nullptr, "NULL argument");
        for (int j = 0; j < t; ++j)
            require_no_overlap(d_m, N * NW * 4, h_parts[j], N * W * 4, false, "pai_threshold_combine: d_m overlaps a part");
        if (d_rowflag) require_no_overlap(d_rowflag, N * 4, d_m, N * NW * 4, false, "pai_threshold_combine: d_rowflag overlaps d_m");
        std::lock_guard<std::mutex> open_lk(pk->open_mu);
        DeviceScope scope_(pk->device);
        hipStream_t s = (hipStream_t)stream;
        std::vector<KernelTime> times;
        auto keep = [&] {
            times.insert(times.end(), g_last_times.begin(), g_last_times.end());
            g_last_times.clear();
        };
        // theta 2^(32 n_words) mod n for k_tfinish's Montgomery product and the exponents of the composition route: read by the kernels
        // from one pinned staging slot (this call stages nothing else, and neither do the calls it is made of)
        std::vector<uint32_t> thR(NW, 0);
        {
            const Limbs v = hbn::mod(hbn::shl(theta, 32 * (int)NW), pk->n);
            std::copy(v.begin(), v.end(), thR.begin());
        }
        const uint32_t *d_thR = nullptr, *d_mu = nullptr;
        {
            const void* src[2] = {thR.data(), mu};
            const size_t len[2] = {NW * 4, sizeof(mu[0]) * (size_t)t};
            void* dp[2] = {nullptr, nullptr};
            host_stage_parts(pk->device, 2, src, len, stream, dp);
            d_thR = static_cast<const uint32_t*>(dp[0]);
            d_mu = static_cast<const uint32_t*>(dp[1]);
        }
        StageSeal seal_(pk->device);                              // theta and the coefficients: their last reader (k_tfinish) is queued when this scope ends
        const bool has_neg = neg_mask != 0, has_pos = (~neg_mask & ((1u << t) - 1u)) != 0;
        const bool fused = pk->penc_nl != 0 && !knob_disabled("tcombine") && N >= tcomb_min((size_t)pk->dev.ncu, pk->key_bits, hbn::bitlen(pk->n), t);
        uint32_t *Pp = nullptr, *Pn = nullptr;
        int* inv_flag = nullptr;
        {
            std::lock_guard<std::mutex> lk(pk->mu);
            pk->tcomb_sides.ensure(2 * N * W * 4 + 16);
            Pp = pk->tcomb_sides.as<uint32_t>();
            Pn = Pp + N * W;
            inv_flag = reinterpret_cast<int*>(Pn + N * W);
            if (fused) {
                const size_t tiles = (N + BLOCK_THREADS - 1) / BLOCK_THREADS;
                int grid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
                long long cap = 0;
                if (knob_tune("tcomb_grid", &cap) && cap >= 1) grid = (int)std::min<long long>(grid, cap);
                pk->tcomb_table.ensure(ctmul_padic_table_words(pk->penc_nl, 4, (size_t)grid) * 4);       // 16 entries per slot
                TcombPadicParams Q{};
                Q.nctx = pk->nmod.d_ctx;
                Q.nm1 = pk->d_nm1;
                Q.nsq = pk->d_nsq29;
                Q.kdig = pk->d_ct_kdig;
                Q.mscratch = reinterpret_cast<uint4*>(pk->d_mscratch);
                Q.table = pk->tcomb_table.as<uint4>();
                Q.nd = pk->ct_nd;
                Q.ct_words = pk->ct_words;
                Q.t = t;
                Q.neg_mask = neg_mask;
                for (int j = 0; j < t; ++j) {
                    Q.parts[j] = h_parts[j];
                    for (int k = 0; k < TCOMB_MU_WORDS; ++k) Q.mu[j][k] = mu[j][k];
                }
                OrderScope order_(pk->order, s);
                ScopedKernelTimer tm("k_tcomb_padic", s, "padic");
                launcher(padic_enc_ops(pk->penc_nl), &PadicEncOps::tcomb, "no digit-engine combine kernel for this limb count")(s, grid, Q, Pp, Pn,
                                                                                                                              (int)N);
                tm.stop();
                HIP_CHECK(hipGetLastError());
                order_.done();
            } else {
                pk->tcomb_pow.ensure((size_t)t * N * W * 4);
            }
        }
        keep();
        if (!fused) {
            // composition: every part to its exponent (pai_ct_mul, broadcast), then the n-ary product of each side (pai_ct_addn)
            uint32_t* pw = pk->tcomb_pow.as<uint32_t>();
            for (int side = 0; side < 2; ++side) {
                std::vector<const uint32_t*> ops;
                uint32_t* dst = side ? Pn : Pp;
                int members = 0;
                for (int j = 0; j < t; ++j) members += (((neg_mask >> j) & 1u) == (unsigned)side);
                for (int j = 0; j < t; ++j) {
                    if (((neg_mask >> j) & 1u) != (unsigned)side) continue;
                    uint32_t* o = members == 1 ? dst : pw + (size_t)j * N * W;
                    open_sub(pai_ct_mul(pk, h_parts[j], d_mu + (size_t)j * TCOMB_MU_WORDS, TCOMB_MU_WORDS, mu_bits[j], 1, N, o, s));
                    keep();
                    ops.push_back(o);
                }
                if (members >= 2) {
                    open_sub(pai_ct_addn(pk, ops.data(), nullptr, members, 0, 0, 0, N, dst, s));
                    keep();
                }
            }
        }
        const uint32_t* x = Pp;
        if (has_neg) {
            HIP_CHECK(hipMemsetAsync(inv_flag, 0, 4, s));
            open_sub(pai_ct_invert_flag(pk, Pn, N, Pn, inv_flag, s));
            keep();
            hipLaunchKernelGGL(k_status_or, dim3(1), dim3(1), 0, s, d_flag, inv_flag, 2);
            HIP_CHECK(hipGetLastError());
            if (has_pos) {
                open_sub(pai_ct_add(pk, Pp, Pn, 0, N, Pp, s));
                keep();
            } else {
                x = Pn;
            }
        }
        {
            ScopedKernelTimer tm("k_tfinish", s);
            const int nw = (int)NW;
            auto go = [&](auto kernel) {                          // one instantiation per bound on the words of n (the lane's private arrays)
                hipLaunchKernelGGL(kernel, dim3((unsigned)((N + BLOCK_THREADS - 1) / BLOCK_THREADS)), dim3(BLOCK_THREADS), 0, s,
                                   (const uint32_t*)pk->d_nexp, d_thR, nw, x, d_m, d_flag, d_rowflag, (int)N);
            };
            if (nw <= 32) go(k_tfinish<32>);
            else if (nw <= 64) go(k_tfinish<64>);
            else if (nw <= 96) go(k_tfinish<96>);
            else if (nw <= 128) go(k_tfinish<128>);
            else go(k_tfinish<256>);
            tm.stop();
            HIP_CHECK(hipGetLastError());
        }
        keep();
        {   // the last stages ran outside the handle's scratch order: the next user of the sides on another stream waits for them
            std::lock_guard<std::mutex> lk(pk->mu);
            OrderScope order_(pk->order, s);
            order_.done();
        }
        g_last_times.clear();
        for (const KernelTime& kt : times) {                     // one profile entry per kernel name, the stages' times summed
            auto it = std::find_if(g_last_times.begin(), g_last_times.end(), [&](const KernelTime& u) { return u.name == kt.name; });
            if (it == g_last_times.end()) g_last_times.push_back(kt);
            else it->ms += kt.ms;
        }
    });
}
