// pai_encrypt_crt / pai_obfuscate_crt: DJN encryption by the party that holds p and q.  hs^r mod n^2 is two fixed-base
// exponentiations on the encryption digit engine with base s = p, q (k_encrypt_padic with the context of s in place of n: half the
// limbs, a quarter of the limb products each), the Garner lift of the two residues (k_crt_lift) and one pass of k_encrypt on the
// n^2 geometry that multiplies 1 + m n [or the ciphertext] in.  Same bits as pai_encrypt / pai_obfuscate for the same r; every
// call the route does not serve IS the public call.  (Ranges: path_ranges.hpp, section owner-side CRT encryption.)
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once

}  // extern "C"
namespace {

std::vector<uint32_t> crt_pair_of(const Limbs& v, const Limbs& s, int nl) {
    Limbs rem;
    Limbs quo = hbn::divq(v, s, &rem);
    std::vector<uint32_t> h(2 * (size_t)nl, 0);
    auto ra = hbn::to_r29(rem, nl), rb = hbn::to_r29(quo, nl);
    std::memcpy(h.data(), ra.data(), (size_t)nl * 4);
    std::memcpy(h.data() + nl, rb.data(), (size_t)nl * 4);
    return h;
}

// which keys the route serves: DJN keys whose two primes one instantiation of the encryption digit engine accepts (the rule that
// chooses penc_nl, applied to the primes), with a lift kernel for the geometry of q^2
int crt_enc_nl(const pai_privkey* sk) {
    const pai_pubkey* pk = sk->pk;
    if (!pk->djn || knob_disabled("crtenc") || knob_disabled("padic")) return 0;
    const int a = padic_enc_nl_for_n_bits(hbn::bitlen(sk->p)), b = padic_enc_nl_for_n_bits(hbn::bitlen(sk->q));
    return a == b ? a : 0;
}

// constants of the route, built by the first served call (caller holds sk->mu)
bool ensure_crt(pai_privkey* sk) {
    pai_privkey::Crt& C = sk->crt;
    if (C.tried) return C.ok;
    C.tried = true;
    const pai_pubkey* pk = sk->pk;
    const int nl = crt_enc_nl(sk);
    if (!nl) return false;
    const Limbs one{1u};
    const Limbs prime[2] = {sk->p, sk->q};
    const Limbs p2 = hbn::mul(sk->p, sk->p), q2 = hbn::mul(sk->q, sk->q);
    const GeoOps* gq = geo_for_bits(hbn::bitlen(q2));
    if (!gq || !crt_lift_ops(gq->nl)) return false;
    C.nl = nl;
    C.sw = words_for_bits(hbn::bitlen(q2));
    C.nd = (32 * C.sw + hbn::RB * nl - 1) / (hbn::RB * nl);
    C.s_words = words_for_bits(hbn::bitlen(sk->q));
    for (int w = 0; w < 2; ++w) {
        const Limbs& s = prime[w];
        const Limbs s2 = w ? q2 : p2;
        C.hs_s[w] = hbn::mod(pk->hs, s2);
        C.sdig[w].init(s, nl);
        C.d_sm1[w] = upload_r29(hbn::sub(s, one), nl);
        C.d_s2[w] = upload_r29(s2, 2 * nl);
        const Limbs Rm = hbn::mod(hbn::shl(one, hbn::RB * nl), s2);
        C.d_one[w] = upload_vec(crt_pair_of(Rm, s, nl));
        C.d_hs[w] = upload_vec(crt_pair_of(hbn::mulmod(C.hs_s[w], Rm, s2), s, nl));
        std::vector<uint32_t> kd;
        Limbs K = hbn::mulmod(Rm, Rm, s2);
        for (int i = 0; i < C.nd; ++i) {
            const auto h = crt_pair_of(K, s, nl);
            kd.insert(kd.end(), h.begin(), h.end());
            K = hbn::mulmod(K, Rm, s2);
        }
        C.d_kdig[w] = upload_vec(kd);
        C.d_swords[w] = upload_words(s, C.s_words);
    }
    // p^-2 mod q^2 from p^-1 mod q by one Hensel step: x <- x (2 - p x) mod q^2
    const Limbs x0 = sk->pinvq_host;
    const Limbs px = hbn::mulmod(sk->p, x0, q2);
    const Limbs two_minus = hbn::mod(hbn::sub(hbn::add(q2, Limbs{2u}), px), q2);
    const Limbs pinv = hbn::mulmod(x0, two_minus, q2);
    require(hbn::cmp(hbn::mulmod(pinv, hbn::mod(sk->p, q2), q2), one) == 0, "p^-1 mod q^2: inverse check failed");
    const Limbs pinv2 = hbn::mulmod(pinv, pinv, q2);
    require(hbn::cmp(hbn::mulmod(pinv2, hbn::mod(p2, q2), q2), one) == 0, "p^-2 mod q^2: inverse check failed");
    C.q2.init(q2, 0, gq);
    C.d_p2 = upload_r29(p2, gq->nl);
    C.d_pinv2R = upload_r29(hbn::mulmod(pinv2, C.q2.R, q2), gq->nl);
    HIP_CHECK(hipMalloc((void**)&C.d_mscratch, 2 * (size_t)pk->dev.ncu * BLOCK_THREADS * (size_t)nl * 4));
    C.ok = true;
    return true;
}

void release_crt(pai_privkey* sk) {
    pai_privkey::Crt& C = sk->crt;
    for (int w = 0; w < 2; ++w) {
        C.sdig[w].release();
        if (C.d_sm1[w]) (void)hipFree(C.d_sm1[w]);
        if (C.d_s2[w]) (void)hipFree(C.d_s2[w]);
        if (C.d_one[w]) (void)hipFree(C.d_one[w]);
        if (C.d_hs[w]) (void)hipFree(C.d_hs[w]);
        if (C.d_kdig[w]) (void)hipFree(C.d_kdig[w]);
        if (C.d_swords[w]) (void)hipFree(C.d_swords[w]);
    }
    C.q2.release();
    if (C.d_p2) (void)hipFree(C.d_p2);
    if (C.d_pinv2R) (void)hipFree(C.d_pinv2R);
    if (C.d_mscratch) (void)hipFree(C.d_mscratch);
    C.zeros.release();
    C.cs.release();
    C.lifted.release();
}

// The base-s digit-form tables T_s[j][d] = pair_s( hs_s^(d 2^(wb j)) R_s mod s^2 ), s = p, q: the public table's builders
// (k_fb_table_padic, k_fb_expand_padic, the g-factoring passes) with the context of s in place of n.  The window bases
// hs_s^(2^(h j)) are squared on the host (a chain of randbits squarings modulo s^2: milliseconds) and enter digit form on the
// device the way ciphertexts do.  The window width follows the public digit table's rule applied to the half-size entry;
// PAI_TUNE fb_digit_wbits pins it.  The tables belong to the public handle's table set: same LRU entry, same byte budget,
// evicted, trimmed and freed together (capi_pubkey_tables.hpp).  Caller holds sk->mu and pk->mu.
void build_crt_tables_body(pai_privkey* sk, pai_pubkey* pk, int dwb) {
    pai_privkey::Crt& C = sk->crt;
    const int nl = C.nl, randbits = pk->randbits;
    const auto fb_table = launcher(padic_enc_ops(nl), &PadicEncOps::fb_table, "no digit-engine table kernel for this limb count");
    const auto fb_expand = launcher(padic_enc_ops(nl), &PadicEncOps::fb_expand, "no digit-engine table kernel for this limb count");
    const size_t ent_bytes = 2 * (size_t)nl * 4;
    const int DJ = (randbits + dwb - 1) / dwb;
    const int h1 = dwb <= 12 ? dwb : dwb / 2, J1 = dwb <= 12 ? DJ : 2 * DJ;
    const Limbs prime[2] = {sk->p, sk->q};
    bool gform[2] = {false, false};
    for (int w = 0; w < 2; ++w) {
        const Limbs s2 = hbn::mul(prime[w], prime[w]);
        std::vector<uint32_t> bases((size_t)J1 * C.sw, 0);
        {
            hbn::Mont32 mt(s2);
            Limbs b = mt.to_mont(C.hs_s[w]);
            for (int j = 0; j < J1; ++j) {
                const Limbs plain = mt.from_mont(b);
                std::memcpy(&bases[(size_t)j * C.sw], plain.data(), plain.size() * 4);
                if (j + 1 < J1) for (int k = 0; k < h1; ++k) b = mt.mmul(b, b);
            }
        }
        ScopedDevBuf d_bases, d_half;
        d_bases.ensure(bases.size() * 4);
        HIP_CHECK(hipMemcpy(d_bases.p, bases.data(), bases.size() * 4, hipMemcpyHostToDevice));
        FbBases fbb;
        fbb.bases_plain = d_bases.as<uint32_t>();
        fbb.base_words = C.sw;
        fbb.kdig = C.d_kdig[w];
        fbb.nd = C.nd;
        const size_t bytes = ((size_t)DJ << dwb) * ent_bytes;
        HIP_CHECK(hipMalloc((void**)&pk->d_crt_fb[w], bytes));
        pk->crt_fb_bytes += bytes;
        if (dwb <= 12) {
            fb_table(nullptr, C.sdig[w].d_ctx, C.d_sm1[w], C.d_hs[w], C.d_one[w], pk->d_crt_fb[w], DJ, dwb, fbb);
        } else {
            const int h = dwb / 2;
            d_half.ensure(((size_t)(2 * DJ) << h) * ent_bytes);
            fb_table(nullptr, C.sdig[w].d_ctx, C.d_sm1[w], C.d_hs[w], C.d_one[w], d_half.as<uint32_t>(), 2 * DJ, h, fbb);
            fb_expand(nullptr, pk->dev.ncu, C.sdig[w].d_ctx, C.d_sm1[w], d_half.as<uint32_t>(), pk->d_crt_fb[w], DJ, h, C.d_mscratch);
        }
        const hipError_t e1 = hipGetLastError(), e2 = hipDeviceSynchronize();
        HIP_CHECK(e1);
        HIP_CHECK(e2);
        gform[w] = gfactor_digit_rows(nl, C.sdig[w].d_ctx, pk->d_crt_fb[w], (size_t)DJ << dwb, dwb, C.s_words, C.d_swords[w], C.d_mscratch,
                                      pk->dev.ncu);
    }
    // one table format for both halves (the knobs and the scratch decide alike for both; a difference would be a failed allocation)
    if (gform[0] != gform[1]) throw PaiError(PAI_E_HIP, "g-factoring served one prime's table only");
    pk->crt_gform = gform[0];
    pk->crt_wbits = dwb;
    pk->crt_windows = DJ;
    pk->crt_fb_ready = true;
}

void build_crt_tables(pai_privkey* sk) {
    pai_pubkey* pk = const_cast<pai_pubkey*>(sk->pk);
    if (pk->crt_fb_ready) { fb_touch(pk); return; }
    const int nl = sk->crt.nl, randbits = pk->randbits;
    const size_t ent_bytes = 2 * (size_t)nl * 4;
    auto table_bytes = [&](int w) { return (double)((randbits + w - 1) / w) * (double)((size_t)1 << w) * (double)ent_bytes; };
    size_t mem_free = 0, mem_total = 0;
    HIP_CHECK(hipMemGetInfo(&mem_free, &mem_total));
    // the public digit table's sizing rule (build_fb_tables_body) applied to the half-size entry, per table
    double budget = std::min((double)mem_total / 32.0, (double)mem_free / 4.0);
    bool pinned = false;
    if (const char* env = std::getenv("PAI_FB_TABLE_MB")) { double v = std::atof(env); if (v >= 1.0) { budget = v * 1048576.0; pinned = true; } }
    if (!pinned) {
        size_t used = 0; int resident = 0;
        {
            std::lock_guard<std::mutex> g(g_fb.mu);
            for (pai_pubkey* o : g_fb.lru) if (o->device == pk->device && o != pk) { used += o->fb_registered; ++resident; }
        }
        if (resident >= fb_big_keys() || used + pk->fb_bytes + 2 * (size_t)budget > fb_cache_budget(mem_total))
            budget = std::min(budget, (double)fb_small_table_bytes() / 2.0);     // the small operating point, shared by the two tables
    }
    int dwb = 12;
    for (int cand = 20; cand > 12; cand -= 2)
        if (table_bytes(cand) <= budget) { dwb = cand; break; }
    if (long long v; knob_tune("fb_digit_wbits", &v)) {
        if ((v >= 4 && v <= 12) || (v > 12 && v <= 20 && v % 2 == 0)) dwb = (int)v;
    }
    fb_make_room(pk, (size_t)(2.0 * table_bytes(dwb)), mem_total);
    auto drop = [&] {
        fb_free_crt_tables(pk);
        (void)hipGetLastError();
    };
    for (int attempt = 0;; ++attempt) {
        try {
            build_crt_tables_body(sk, pk, dwb);
            pk->fb_bytes += pk->crt_fb_bytes;
            fb_register(pk);
            return;
        } catch (const PaiError& e) {
            drop();
            if (attempt == 0 && e.code == PAI_E_HIP && fb_make_room(pk, (size_t)-1 / 2, mem_total) > 0) continue;
            throw;
        } catch (...) {
            drop();
            throw;
        }
    }
}

// returns false when the call is not served (the caller then takes the public route)
bool encrypt_crt(pai_privkey* sk, const uint32_t* d_m, const uint32_t* d_r, uint32_t* d_ct, size_t N, void* stream, bool from_plain) {
    const pai_pubkey* pk = sk->pk;
    if (N < crtenc_min((size_t)pk->dev.ncu, pk->key_bits) || N >= ((size_t)1 << 30)) return false;
    if (!crt_enc_nl(sk)) return false;
    std::lock_guard<std::mutex> lk(sk->mu);
    DeviceScope scope_(pk->device);
    if (!ensure_crt(sk)) return false;
    pai_privkey::Crt& C = sk->crt;
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lkp(pk->mu);
    g_last_times.clear();
    build_crt_tables(sk);
    const bool grow_zeros = C.zeros_rows < N;
    if (grow_zeros) C.zeros.ensure(N * 4);                  // (a grown buffer is a fresh one: DevBuf::ensure frees the old one, which waits for the device)
    C.cs.ensure(2 * N * (size_t)C.sw * 4);
    C.lifted.ensure(N * (size_t)pk->ct_words * 4);
    OrderScope order_sk(sk->order, s);
    OrderScope order_pk(pk->order, s);
    if (grow_zeros) {
        // filled on the call's own stream, inside the scratch order: this call's kernels follow it on `s`, and a later call on
        // another stream waits for the event this scope records.  (A memset on the null stream is ordered before nothing that
        // runs on a non-blocking stream, and hipMemset does not promise to have completed when it returns.)
        HIP_CHECK(hipMemsetAsync(C.zeros.p, 0, N * 4, s));
        C.zeros_rows = N;
    }
    const size_t tiles = (N + BLOCK_THREADS - 1) / BLOCK_THREADS;
    const int pgrid = (int)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)pk->dev.ncu));
    const auto enc = launcher(padic_enc_ops(C.nl), &PadicEncOps::encrypt, "no digit-engine encrypt kernel for this limb count");
    for (int w = 0; w < 2; ++w) {
        // o_s = hs_s^r mod s^2: mode 1 with an all-zero message (rows of one word), out as the plain residue a + b s mod s^2
        EncPadicParams Q;
        Q.nctx = C.sdig[w].d_ctx;
        Q.nm1 = C.d_sm1[w];
        Q.nsq = C.d_s2[w];
        Q.fb_table = reinterpret_cast<const uint4*>(pk->d_crt_fb[w]);
        Q.mscratch = reinterpret_cast<uint4*>(C.d_mscratch);
        Q.kdig = nullptr;
        Q.nd = 0;
        Q.fb_windows = pk->crt_windows;
        Q.fb_wbits = pk->crt_wbits;
        Q.fb_gform = pk->crt_gform ? 1 : 0;
        Q.pt_words = 1;
        Q.ct_words = C.sw;
        Q.r_words = pk->r_words;
        ScopedKernelTimer t(w ? "k_encrypt_padic(crt q)" : "k_encrypt_padic(crt p)", s, "crt");
        enc(s, pgrid, Q, C.zeros.as<uint32_t>(), d_r, nullptr, C.cs.as<uint32_t>() + (size_t)w * N * C.sw, (int)N, 1);
        t.stop();
        HIP_CHECK(hipGetLastError());
    }
    {
        const CrtLiftOps* L = crt_lift_ops(C.q2.geo->nl);
        CrtLiftParams P;
        P.q2 = C.q2.d_ctx;
        P.p2 = C.d_p2;
        P.pinv2R = C.d_pinv2R;
        P.in_words = C.sw;
        P.ct_words = pk->ct_words;
        const size_t lt = (N + L->epb - 1) / L->epb;
        const int lgrid = (int)std::max<size_t>(1, std::min<size_t>(lt, (size_t)pk->dev.ncu * 4));
        ScopedKernelTimer t("k_crt_lift", s, "crt");
        L->lift(s, lgrid, P, C.cs.as<uint32_t>(), C.lifted.as<uint32_t>(), (int)N);
        t.stop();
        HIP_CHECK(hipGetLastError());
    }
    {
        // ct = (1 + m n) hs^r [or ct hs^r]: the obfuscator-given modes of k_encrypt on the n^2 geometry, as the standard scheme's
        const GeoOps* g = pk->msq.geo;
        ScopedKernelTimer t(from_plain ? "k_encrypt(crt mul)" : "k_encrypt(crt obfuscate)", s, "crt");
        g->encrypt(s, grid_for(g, N, pk->dev.ncu), pk->enc_params(), d_m, C.lifted.as<uint32_t>(), d_ct, d_ct, (int)N, from_plain ? 3 : 4);
        t.stop();
        HIP_CHECK(hipGetLastError());
    }
    order_pk.done();
    order_sk.done();
    return true;
}

}  // namespace
extern "C" {

int pai_encrypt_crt(pai_privkey* sk, const uint32_t* d_m, const uint32_t* d_r, size_t N, uint32_t* d_ct, void* stream) {
    bool served = false;
    const int rc = guarded([&] {
        require(sk && sk->pk && d_m && d_ct, "NULL argument");
        if (N == 0) { served = true; return; }
        if (d_r) served = encrypt_crt(sk, d_m, d_r, d_ct, N, stream, true);
    });
    if (rc != PAI_OK || served) return rc;
    return pai_encrypt(sk->pk, d_m, d_r, N, d_ct, stream);
}

int pai_obfuscate_crt(pai_privkey* sk, uint32_t* d_ct, const uint32_t* d_r, size_t N, void* stream) {
    bool served = false;
    const int rc = guarded([&] {
        require(sk && sk->pk && d_ct && d_r, "NULL argument");
        if (N == 0) { served = true; return; }
        served = encrypt_crt(sk, nullptr, d_r, d_ct, N, stream, false);
    });
    if (rc != PAI_OK || served) return rc;
    return pai_obfuscate(sk->pk, d_ct, d_r, N, stream);
}

int pai_privkey_crt_table_info(const pai_privkey* sk, size_t* table_bytes, int* window_bits, int* windows) {
    return guarded([&] {
        require(sk && sk->pk, "sk is NULL");
        const pai_pubkey* pk = sk->pk;
        std::lock_guard<std::mutex> lk(pk->mu);
        if (table_bytes) *table_bytes = pk->crt_fb_ready ? pk->crt_fb_bytes : 0;
        if (window_bits) *window_bits = pk->crt_fb_ready ? pk->crt_wbits : 0;
        if (windows) *windows = pk->crt_fb_ready ? pk->crt_windows : 0;
    });
}
