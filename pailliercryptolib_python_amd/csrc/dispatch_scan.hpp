// pai_ct_scan: the prefix products behind PaillierEncryptedNumber.cumsum (extension; kernel: k_segscan).
// (Part of the C-API translation unit: included by paillier_capi.hip inside extern "C"; not a stand-alone header.)
#pragma once
// With enough runs to fill the device a run is one chain and the call is one launch.  Otherwise a level cuts every run into
// chunks of C scan positions (scan_chunk, path_ranges.hpp) and takes three phases, separate launches on the stream — no
// workgroup ever waits for another one:
//   1. totals:  one chain per chunk, unseeded, only its last value (tag 1) and the sum of its steps;
//   2. the inclusive scan of the totals per run, their step sums as steps — the same problem with seg_len = chunks per run,
//      so the next level, until one fits a chain per run; chunk c's carry is the scanned total of chunk c - 1;
//   3. prefixes: one chain per chunk again, seeded with its carry (the first chunk of a run unseeded), every prefix stored.
// A level holds T = runs * ceil(L / C) totals; totals, scanned totals and step sums of all levels lie behind one another in the
// handle's scratch (seg_partial / seg_plan: at most 2 N rows each way, N / C in practice).  Nothing is read back: uniform runs
// make every size known on the host.  The caller holds pk->mu and has selected the device.
static void ct_scan_locked(const pai_pubkey* pk, hipStream_t s, const uint32_t* d_ct, size_t N, int tag, int dom_out, size_t seg_len,
                           int reverse, const int32_t* d_raise, const int32_t* d_step, uint32_t* d_out) {
    const uint32_t* rpow = rpow_table(pk);
    const GeoOps* g = pk->msq.geo;
    const size_t W = (size_t)pk->ct_words;
    struct Level { size_t n, len, chunk, cpr, chains; };
    std::vector<Level> lv;                               // the chunked levels, then the one that runs a chain per run
    size_t rows_total = 0;
    for (size_t n = N, len = seg_len;;) {
        size_t c = scan_chunk((size_t)pk->dev.ncu, g->epb, n, len);
        if (!lv.empty()) c = std::max<size_t>(c, 2);
        if (c >= len) {
            lv.push_back({n, len, len, 1, n / len});
            break;
        }
        const size_t cpr = (len + c - 1) / c, chains = (n / len) * cpr;
        lv.push_back({n, len, c, cpr, chains});
        rows_total += chains;
        n = chains;
        len = cpr;
    }
    const size_t K = lv.size() - 1;                      // chunked levels
    OrderScope order_(pk->order, s);
    uint32_t *totals = nullptr, *scanned = nullptr;
    int32_t* ssum = nullptr;
    if (K) {
        pk->seg_partial.ensure(2 * rows_total * W * 4);
        pk->seg_plan.ensure(rows_total * 4);
        totals = pk->seg_partial.as<uint32_t>();
        scanned = totals + rows_total * W;
        ssum = pk->seg_plan.as<int32_t>();
    }
    std::vector<size_t> at(K + 1, 0);                    // level l's totals / scanned totals / step sums start at row at[l]
    for (size_t l = 0; l < K; ++l) at[l + 1] = at[l] + lv[l].chains;
    int* status = status_word(pk, s);
    // level l reads: the caller's rows (l == 0), or the totals of level l - 1 (tag 1, forward, their step sums as steps)
    auto launch = [&](size_t l, const uint32_t* seed, uint32_t* out, int32_t* step_sum, bool totals_only, int dom) {
        const Level& L = lv[l];
        ScanArgs A;
        A.ct = l ? totals + at[l - 1] * W : d_ct;
        A.raise = l ? nullptr : d_raise;
        A.step = l ? ssum + at[l - 1] : d_step;
        A.seed = seed; A.out = out; A.step_sum = step_sum; A.status = status;
        A.n = (int)L.n; A.tag = l ? 1 : tag; A.dom_out = dom; A.seg_len = (int)L.len; A.chunk = (int)L.chunk; A.cpr = (int)L.cpr;
        A.chains = (int)L.chains; A.reverse = l ? 0 : reverse; A.totals = totals_only ? 1 : 0;
        ScopedKernelTimer t("k_segscan", s);
        g->segscan(s, grid_for(g, L.chains, pk->dev.ncu), pk->msq.d_ctx, A, pk->ct_words, rpow);
        t.stop();
        HIP_CHECK(hipGetLastError());
    };
    for (size_t l = 0; l < K; ++l) launch(l, nullptr, totals + at[l] * W, ssum + at[l], true, 1);
    for (size_t l = K + 1; l-- > 0;) {
        uint32_t* out = l ? scanned + at[l - 1] * W : d_out;
        launch(l, l < K ? scanned + at[l] * W : nullptr, out, nullptr, false, l ? 1 : dom_out);
    }
    order_.done();
}

int pai_ct_scan(const pai_pubkey* pk, const uint32_t* d_ct, size_t N, int tag, int dom_out, size_t seg_len, int reverse,
                const int32_t* d_raise, const int32_t* d_step, uint32_t* d_out, void* stream) {
    return guarded([&] {
        require(pk != nullptr, "NULL argument");
        require(std::abs(tag) <= RPOW_SPAN - 2 && std::abs(dom_out) <= RPOW_SPAN - 2, "pai_ct_scan: domain tag out of range");
        require(N < ((size_t)1 << 31), "pai_ct_scan: too many rows for one call");
        if (N == 0) return;
        require(seg_len > 0 && N % seg_len == 0, "pai_ct_scan: seg_len must divide N");
        require(d_ct && d_out, "NULL argument");
        require_no_overlap(d_out, N * (size_t)pk->ct_words * 4, d_ct, N * (size_t)pk->ct_words * 4, false, "pai_ct_scan: d_out must not alias d_ct");
        std::lock_guard<std::mutex> lk(pk->mu);
        DeviceScope scope_(pk->device);
        g_last_times.clear();
        ct_scan_locked(pk, (hipStream_t)stream, d_ct, N, tag, dom_out, seg_len, reverse != 0, d_raise, d_step, d_out);
    });
}
