// pai_recover_r: the randomness of a ciphertext's opening, by the holder of p and q (kernels_recover.hpp).  One route: stage A and
// stage B on the lane-group geometry of the primes (sk->pr[w]), for every key pai_privkey_create accepts and every batch size.
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once

// Recovery context.  d_s = n^-1 mod (s - 1) = (the other prime)^-1 mod (s - 1), since n = p q and s == 1 (mod s - 1); s - 1 is even,
// hence hbn::inv_mod, and each inverse is multiplied back.  A key with gcd(n, (p - 1)(q - 1)) != 1 (p | q - 1) has no such exponent:
// PAI_E_INVALID, every time, before anything is launched.
static void ensure_rec(pai_privkey* sk) {
    pai_privkey::Rec& R = sk->rec;
    static const char* const no_inverse = "pai_recover_r: n is not coprime to (p - 1)(q - 1): this key's ciphertexts have no unique opening";
    if (R.tried) {
        if (!R.ok) throw PaiError(PAI_E_INVALID, no_inverse);
        return;
    }
    const Limbs one{1u};
    const Limbs prime[2] = {sk->p, sk->q};
    Limbs d[2];
    for (int w = 0; w < 2; ++w) {
        const Limbs sm1 = hbn::sub(prime[w], one);
        const Limbs other = hbn::mod(prime[1 - w], sm1);
        if (!hbn::inv_mod(other, sm1, &d[w])) {
            R.tried = true;
            throw PaiError(PAI_E_INVALID, no_inverse);
        }
        if (hbn::cmp(hbn::mulmod(d[w], hbn::mod(sk->pk->n, sm1), sm1), one) != 0)
            throw PaiError(PAI_E_INTERNAL, "pai_recover_r: inverse check failed");
    }
    const GeoOps* g = sk->pr[0].geo;
    const int nl = g->nl;
    R.nd = (32 * sk->pk->ct_words + hbn::RB * nl - 1) / (hbn::RB * nl);
    R.r_words = std::max(sk->pr[0].w32, sk->pr[1].w32);
    for (int w = 0; w < 2; ++w) {
        R.ebits[w] = hbn::bitlen(d[w]);
        R.ewords[w] = words_for_bits(R.ebits[w]);
        R.d_expo[w] = upload_words(d[w], R.ewords[w]);
        // R^(i+2) mod s for the row's base-R digits, as stage A of decryption has them modulo s^2
        std::vector<uint32_t> kd;
        Limbs K = sk->pr[w].R2;
        for (int i = 0; i < R.nd; ++i) {
            const auto r = hbn::to_r29(K, nl);
            kd.insert(kd.end(), r.begin(), r.end());
            K = hbn::mulmod(K, sk->pr[w].R, prime[w]);
        }
        R.d_kdig[w] = upload_vec(kd);
    }
    R.tried = true;
    R.ok = true;
}

static void release_rec(pai_privkey* sk) {
    pai_privkey::Rec& R = sk->rec;
    for (int w = 0; w < 2; ++w) {
        if (R.d_expo[w]) (void)hipFree(R.d_expo[w]);
        if (R.d_kdig[w]) (void)hipFree(R.d_kdig[w]);
        R.d_expo[w] = R.d_kdig[w] = nullptr;
    }
    R.table.release();
    R.rs.release();
}

int pai_recover_r(pai_privkey* sk, const uint32_t* d_ct, size_t N, uint32_t* d_r, void* stream) {
    return guarded([&] {
        require(sk && d_ct && d_r, "NULL argument");
        if (N == 0) return;
        require(N <= (size_t)0x7fffffff, "pai_recover_r: batch too large");
        std::lock_guard<std::mutex> lk(sk->mu);
        const pai_pubkey* pk = sk->pk;
        DeviceScope scope_(pk->device);
        DeviceInfo dev = scope_.info;
        hipStream_t s = (hipStream_t)stream;
        g_last_times.clear();
        ensure_rec(sk);
        pai_privkey::Rec& R = sk->rec;
        const GeoOps* g = sk->pr[0].geo;
        int gridx = grid_for(g, N, dev.ncu, 1);           // x 2 primes => 2 workgroups per CU
        long long cap = 0;
        if (knob_tune("rrec_grid", &cap) && cap >= 1) gridx = (int)std::min<long long>(gridx, cap);
        R.table.ensure(g->table_words((size_t)gridx * 2) * 4);
        R.rs.ensure(2 * N * (size_t)R.r_words * 4);
        OrderScope order(sk->order, s);
        RrecAParams A;
        RrecBParams B;
        for (int w = 0; w < 2; ++w) {
            A.pr[w] = sk->pr[w].d_ctx;
            A.kdig[w] = R.d_kdig[w];
            A.expo[w] = R.d_expo[w];
            A.ewords[w] = R.ewords[w];
            A.ebits[w] = R.ebits[w];
            B.pr[w] = sk->pr[w].d_ctx;
        }
        A.nd = R.nd;
        A.ct_words = pk->ct_words;
        A.r_words = R.r_words;
        B.pinvqR = sk->d_pinvqR;
        B.r_words = R.r_words;
        B.out_words = pk->n_words;
        {
            ScopedKernelTimer t("k_rrec_a", s, "lane_group");
            launcher(g, &GeoOps::rrec_a, "no recovery kernel for this geometry")(s, gridx, A, d_ct, R.rs.as<uint32_t>(), (int)N,
                                                                                 R.table.as<uint32_t>());
            t.stop();
        }
        HIP_CHECK(hipGetLastError());
        {
            ScopedKernelTimer t("k_rrec_b", s);
            launcher(g, &GeoOps::rrec_b, "no recovery kernel for this geometry")(s, grid_for(g, N, dev.ncu), B, R.rs.as<uint32_t>(), d_r,
                                                                                 (int)N);
            t.stop();
        }
        HIP_CHECK(hipGetLastError());
        order.done();                          // table / residue scratch are reused by the next call: ordered by stream or event
    });
}
