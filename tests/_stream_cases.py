"""The case table of the stream-contract tests: one row per entry point of include/paillier_hip.h that takes `void* stream`
(tests/test_stream_contract_cpu.py parses the header and asserts, by name, that every one of them is here or in EXCLUDED).

A row says how to call its entry point at a small shape through a placement of tests/_streams.py (Resident or Late), what the
outputs must be — CPython integers, hashlib for the SHA calls, the models the suite already has for the codec — and two flags read
off the dispatcher:

    syncs    the header says that the call synchronises `stream` (the call may return with the stream idle);
    chained  the call runs under its handle's OrderScope at the routes the row forces: it is ordered against the other scratch users
             of that handle on OTHER streams (test B).  A set of variant names where only some routes are.

Rows with `family` run test A through the runner of tests/_fuzz_ext_run.py on the case tests/_fuzz_ext.case(family, key, SEED, rnd)
builds; every row that is chained carries a single-call `build(h, st, N) -> (call, [(device array, expected host array), ...])`,
which test A uses where there is no family and test B (one call against a partner on another stream) always.

Variants are environments (the suite's knobs, read by the library at every call): "lat" — the defaults, which at N = 65 are the
small-batch routes; "thr" — PAI_LATENCY_MAX=0 and PAI_LAT_ADD_MAX=0, the throughput kernels (the digit engine up to 2048 bits, lane
groups and digit pairs above).  Shapes: N = 65, one full and one ragged tile of the 64-element kernels; 257 where a route walks
256-row tiles.  Value operands (ciphertext rows, messages, randomness, exponents, SHA parts, codec inputs) are late; whatever a
kernel indexes with (shifts, offsets, rows, targets) is resident."""
from __future__ import annotations

import contextlib
import ctypes as C
import hashlib
import random
import struct
from collections import namedtuple

import numpy as np

N_TILE = 65
N_LANES = 257
BASE_TUNE = {"fb_digit_wbits": 6}                    # small fixed-base tables (as tests/_fuzz_ext.FB_WBITS): built in milliseconds
VARIANTS = {
    "lat": {},
    "thr": {"PAI_LATENCY_MAX": "0", "PAI_LAT_ADD_MAX": "0"},
    "pow2digit": {"PAI_LATENCY_MAX": "0", "PAI_LAT_ADD_MAX": "0", "PAI_POW2_DIGIT_MIN": "1"},
}
ALL_BITS = (1024, 2048, 3072, 4096)                  # one key per class of tests/_fuzz_ext.KEY_CLASSES
Row = namedtuple("Row", "name syncs chained build family variants bits N tune rnd", defaults=(None, None, ("lat",), (2048,), N_TILE, None, 1))

# entry points with a stream argument that have no row, and why
EXCLUDED = {
    "pai_memcpy_h2d": "the harness itself: the tests place operands with it (and it synchronises by definition)",
    "pai_memcpy_d2h": "the harness itself: every output of every row is read back with it on the stream under test",
    "pai_stream_sync": "the harness itself: hipStreamSynchronize behind the device scope",
}


_MEMO = {}
_SALT = [""]


@contextlib.contextmanager
def salted(text):
    """operands built inside are drawn from other seeds: inputs of its own for every thread of the thread test"""
    _SALT.append(text)
    try:
        yield
    finally:
        _SALT.pop()


def memo(fn):
    """operands and expectations are computed once per (key, shape) and shared by the tests that need them"""
    def wrapped(h, *args):
        k = (fn.__name__, h.key.bits, _SALT[-1]) + args
        if k not in _MEMO:
            _MEMO[k] = fn(h, *args)
        return _MEMO[k]
    return wrapped


def L(vals, words):
    from tests._util import ints_to_limbs

    return ints_to_limbs(vals, words)


def plain(h, N, seed):
    rng = random.Random(f"stream-plain/{h.key.bits}/{seed}/{_SALT[-1]}")
    m = [rng.randrange(h.key.n) for _ in range(N)]
    m[:3] = [0, 1, h.key.n - 1][:N]
    return m


def ciph(h, N, seed):
    """N units modulo n^2 with known plaintexts: (1 + m n) hs^(seed + i)"""
    key = h.key
    m = plain(h, N, seed)
    g, out = pow(key.hs, seed + 3, key.nsq), []
    for x in m:
        out.append((1 + x * key.n) % key.nsq * g % key.nsq)
        g = g * key.hs % key.nsq
    return m, out


def expos(N, bits, seed):
    rng = random.Random(f"stream-expo/{bits}/{seed}/{_SALT[-1]}")
    e = [rng.getrandbits(bits) | 1 << (bits - 1) for _ in range(N)]
    e[:2] = [1, (1 << bits) - 1][:N]
    return e


def rand_r(h, N, seed):
    from oracle import paillier_oracle as orc

    r = orc.synth_r_limbs(seed, N, h.key.randbits)
    r[0] = 0
    return r


def deltas(N, seed):
    d = np.random.default_rng(seed).integers(-3, 9, N).astype(np.int32)
    d[:6] = [0, 1, -3, 8, -1, 7][:N]
    return d


def aligned(a, b, d, M):
    return [x * pow(y, 1 << int(k), M) % M if k > 0 else pow(x, 1 << int(-k), M) * y % M for x, y, k in zip(a, b, d)]


def host_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the hot path ----------------------------------------------------------------------------------------------------------------
def b_raw_encrypt(h, st, N):
    nk, key = h.nk, h.key
    m = plain(h, N, 1)
    dm, out = st.value(L(m, nk.nw)), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_raw_encrypt(nk.pk, dm.ptr, N, out.ptr, st.stream)), [(out, L([(1 + x * key.n) % key.nsq for x in m], nk.cw))]


def b_ct_add_plain(h, st, N):
    nk, key = h.nk, h.key
    _, ct = ciph(h, N, 2)
    m = plain(h, N, 3)
    dc, dm, out = st.value(L(ct, nk.cw)), st.value(L(m, nk.nw)), st.out((N, nk.cw))
    want = [c * (1 + x * key.n) % key.nsq for c, x in zip(ct, m)]
    return (lambda: nk.lib.pai_ct_add_plain(nk.pk, dc.ptr, dm.ptr, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


@memo
def _enc_operands(h, N, seed):
    from tests._util import djn_encrypt_many, limbs_to_ints

    m, r = plain(h, N, seed), rand_r(h, N, seed + 100)
    return m, r, djn_encrypt_many(h.key, m, limbs_to_ints(r))


def b_encrypt(h, st, N):
    nk = h.nk
    m, r, want = _enc_operands(h, N, 4)
    dm, dr, out = st.value(L(m, nk.nw)), st.value(r), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_obfuscate(h, st, N):
    from tests._util import djn_obfuscate_many, limbs_to_ints

    nk = h.nk
    _, ct = ciph(h, N, 5)
    r = rand_r(h, N, 105)
    dc, dr = st.value(L(ct, nk.cw)), st.value(r)
    return (lambda: nk.lib.pai_obfuscate(nk.pk, dc.ptr, dr.ptr, N, st.stream)), [(dc, L(djn_obfuscate_many(h.key, ct, limbs_to_ints(r)), nk.cw))]


def b_encrypt_crt(h, st, N):
    nk = h.nk
    m, r, want = _enc_operands(h, N, 6)
    dm, dr, out = st.value(L(m, nk.nw)), st.value(r), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_encrypt_crt(nk.sk, dm.ptr, dr.ptr, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_decrypt(h, st, N):
    nk = h.nk
    m, ct = ciph(h, N, 7)
    dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.nw))
    return (lambda: nk.lib.pai_decrypt(nk.sk, dc.ptr, N, out.ptr, st.stream)), [(out, L(m, nk.nw))]


def b_recover_r(h, st, N):
    from tests._util import pow_many

    nk, key = h.nk, h.key
    rng = random.Random(f"stream-recover/{key.bits}")
    rs = [1, key.n - 1] + [rng.randrange(2, key.n) for _ in range(N - 2)]        # (a random residue is a unit but for a negligible chance)
    ms = plain(h, N, 8)
    ct = [(1 + m * key.n) % key.nsq * o % key.nsq for m, o in zip(ms, pow_many(rs, key.n, key.nsq))]
    dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.nw))
    return (lambda: nk.lib.pai_recover_r(nk.sk, dc.ptr, N, out.ptr, st.stream)), [(out, L(rs, nk.nw))]


# ---- ciphertext arithmetic ---------------------------------------------------------------------------------------------------------
def _binary(fn_name, want_of, extra=None):
    def build(h, st, N):
        nk, M = h.nk, h.key.nsq
        _, a = ciph(h, N, 10)
        _, b = ciph(h, N, 11)
        da, db, out = st.value(L(a, nk.cw)), st.value(L(b, nk.cw)), st.out((N, nk.cw))
        ex, want = want_of(h, st, N, a, b)
        fn = getattr(nk.lib, fn_name)
        return (lambda: fn(nk.pk, da.ptr, db.ptr, 0, *ex(N, out))), [(out, L(want, nk.cw))]
    return build


def _w_add(h, st, N, a, b):
    M = h.key.nsq
    return (lambda N, out: (N, out.ptr, st.stream)), [x * y % M for x, y in zip(a, b)]


def _w_mont(h, st, N, a, b):
    M = h.key.nsq
    Ri = pow(h.R, -1, M)
    return (lambda N, out: (N, out.ptr, st.stream)), [x * y * Ri % M for x, y in zip(a, b)]


def _w_aligned(h, st, N, a, b):
    d = deltas(N, 12)
    dd = st.resident(d)
    return (lambda N, out: (dd.ptr, N, out.ptr, st.stream)), aligned(a, b, d, h.key.nsq)


def _w_aligned_host(h, st, N, a, b):
    d = deltas(N, 13)
    return (lambda N, out: (host_ptr(d), N, out.ptr, st.stream)), aligned(a, b, d, h.key.nsq)


def b_add_aligned_dom(h, st, N):
    nk, M = h.nk, h.key.nsq
    _, a = ciph(h, N, 14)
    _, b = ciph(h, N, 15)
    d = deltas(N, 16)
    t1 = lambda v: [x * h.R % M for x in v]
    da, db, dd, de, out = st.value(L(t1(a), nk.cw)), st.value(L(t1(b), nk.cw)), st.resident(d), st.resident(L([h.R], nk.cw)), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_ct_add_aligned_dom(nk.pk, da.ptr, db.ptr, 0, dd.ptr, N, out.ptr, de.ptr, st.stream)), \
        [(out, L(t1(aligned(a, b, d, M)), nk.cw))]


def b_addn(h, st, N):
    nk, M = h.nk, h.key.nsq
    ops = [ciph(h, N, 20 + j)[1] for j in range(3)]
    dops = [st.value(L(o, nk.cw)) for o in ops]
    out = st.out((N, nk.cw))
    ptrs = (C.c_void_p * 3)(*[d.ptr.value for d in dops])
    want = [x * y % M * z % M for x, y, z in zip(*ops)]
    return (lambda: nk.lib.pai_ct_addn(nk.pk, ptrs, None, 3, 0, 0, 0, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


@memo
def _mul_operands(h, N):
    from tests._util import pow_many

    _, ct = ciph(h, N, 30)
    e = expos(N, 53, 31)
    return ct, e, pow_many(ct, e, h.key.nsq)


def b_ct_mul(h, st, N):
    nk = h.nk
    ct, e, want = _mul_operands(h, N)
    dc, de, out = st.value(L(ct, nk.cw)), st.value(L(e, 2)), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_ct_mul(nk.pk, dc.ptr, de.ptr, 2, 53, 0, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_ct_mul_host(h, st, N):
    nk = h.nk
    ct, e, want = _mul_operands(h, N)
    eh = L(e, 2)
    dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_ct_mul_host(nk.pk, dc.ptr, host_ptr(eh), 2, 53, 0, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_host_stage(h, st, N):
    """pai_host_stage, then its consumer on the same stream: pai_ct_mul reads the exponents through the returned pointer"""
    nk = h.nk
    ct, e, want = _mul_operands(h, N)
    eh = L(e, 2)
    dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.cw))

    def call():
        srcs, sizes, ptrs = (C.c_void_p * 1)(eh.ctypes.data), (C.c_size_t * 1)(eh.nbytes), (C.c_void_p * 1)()
        rc = nk.lib.pai_host_stage(0, 1, srcs, sizes, st.stream, ptrs)
        rc = rc or nk.lib.pai_ct_mul(nk.pk, dc.ptr, C.c_void_p(ptrs[0]), 2, 53, 0, N, out.ptr, st.stream)
        # the next staging of this thread marks the point behind the reader on st.stream: made here, on the null stream, because the
        # test destroys st.stream when it ends (include/paillier_hip.h, pai_host_stage)
        return rc or nk.lib.pai_host_stage(0, 1, srcs, sizes, None, (C.c_void_p * 1)())
    return call, [(out, L(want, nk.cw))]


def b_ct_prod(h, st, N):
    nk, M = h.nk, h.key.nsq
    groups = 5
    _, ct = ciph(h, N, 32)                               # N = 65: 13 members in each of 5 groups
    want = []
    for g in range(groups):
        acc = 1
        for l in range(N // groups):
            acc = acc * ct[l * groups + g] % M
        want.append(acc)
    dc, out = st.value(L(ct, nk.cw)), st.out((groups, nk.cw))
    return (lambda: nk.lib.pai_ct_prod(nk.pk, dc.ptr, N, groups, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def _invert(form):
    def build(h, st, N):
        nk, M = h.nk, h.key.nsq
        _, ct = ciph(h, N, 33)
        dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.cw))
        exp = [(out, L([pow(c, -1, M) for c in ct], nk.cw))]
        if form == "flag":
            fl = st.resident(np.zeros(1, np.int32))
            return (lambda: nk.lib.pai_ct_invert_flag(nk.pk, dc.ptr, N, out.ptr, fl.ptr, st.stream)), exp + [(fl, np.zeros(1, np.int32))]
        fn = nk.lib.pai_ct_invert if form == "sync" else nk.lib.pai_ct_invert_async
        return (lambda: fn(nk.pk, dc.ptr, N, out.ptr, st.stream)), exp
    return build


def _pow2(hint):
    def build(h, st, N):
        nk, M = h.nk, h.key.nsq
        _, ct = ciph(h, N, 34)
        d = deltas(N, 35)
        dc, dd = st.value(L(ct, nk.cw)), st.resident(d)
        want = [pow(c, 1 << int(k), M) if k > 0 else c for c, k in zip(ct, d)]
        if hint:
            return (lambda: nk.lib.pai_ct_pow2_hint(nk.pk, dc.ptr, dd.ptr, 0, N, 8, st.stream)), [(dc, L(want, nk.cw))]
        return (lambda: nk.lib.pai_ct_pow2(nk.pk, dc.ptr, dd.ptr, 0, N, st.stream)), [(dc, L(want, nk.cw))]
    return build


def b_status(h, st, N):
    """the status word after an asynchronous inversion of units queued on the same stream: 0, read behind it"""
    nk, M = h.nk, h.key.nsq
    _, ct = ciph(h, N, 36)
    dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.cw))
    word = C.c_int(-1)

    def call():
        rc = nk.lib.pai_ct_invert_async(nk.pk, dc.ptr, N, out.ptr, st.stream)
        rc = rc or nk.lib.pai_pubkey_status(nk.pk, C.byref(word), 1, st.stream)
        assert word.value == 0, f"status word {word.value}"
        return rc
    return call, [(out, L([pow(c, -1, M) for c in ct], nk.cw))]


def b_multiexp(h, st, N):
    nk, M = h.nk, h.key.nsq
    R_, K_, Mc, ew = 2, 5, 3, 2
    _, base = ciph(h, R_ * K_, 37)
    rng = random.Random(38)
    e = [[[rng.getrandbits(53) for _ in range(Mc)] for _ in range(K_)] for _ in range(R_)]
    e[0][0][0], e[0][1][0], e[1][0][1] = 0, 1, (1 << 53) - 1
    e_l = np.array([[[[e[r][l][j] & 0xFFFFFFFF, e[r][l][j] >> 32] for j in range(Mc)] for l in range(K_)] for r in range(R_)], dtype=np.uint32)
    want = []
    for r in range(R_):
        for j in range(Mc):
            acc = 1
            for l in range(K_):
                acc = acc * pow(base[r * K_ + l], e[r][l][j], M) % M
            want.append(acc)
    dc, de, out = st.value(L(base, nk.cw)), st.value(e_l.reshape(-1, ew)), st.out((R_ * Mc, nk.cw))
    return (lambda: nk.lib.pai_ct_multiexp(nk.pk, dc.ptr, None, R_, K_, Mc, de.ptr, ew, 53, None, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_scan(h, st, N):
    from tests._fuzz_ext import model_scan

    nk, M = h.nk, h.key.nsq
    _, ct = ciph(h, N, 39)
    rng = np.random.default_rng(40)
    raise_, step = rng.integers(0, 3, N).astype(np.int32), rng.integers(0, 3, N).astype(np.int32)
    want = model_scan(ct, [int(v) for v in raise_], [int(v) for v in step], N, 0, M)
    dc, dr, ds, out = st.value(L(ct, nk.cw)), st.resident(raise_), st.resident(step), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_ct_scan(nk.pk, dc.ptr, N, 0, 0, N, 0, dr.ptr, ds.ptr, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_obfuscate_crt(h, st, N):
    from tests._util import djn_obfuscate_many, limbs_to_ints

    nk = h.nk
    _, ct = ciph(h, N, 44)
    r = rand_r(h, N, 144)
    dc, dr = st.value(L(ct, nk.cw)), st.value(r)
    return (lambda: nk.lib.pai_obfuscate_crt(nk.sk, dc.ptr, dr.ptr, N, st.stream)), [(dc, L(djn_obfuscate_many(h.key, ct, limbs_to_ints(r)), nk.cw))]


def b_segment_prod(h, st, N):
    """65 gathered rows in 5 segments (an empty one, one member, 2, 17, 45) with shifts; segprod_chunk = 3: several levels"""
    from tests._fuzz_ext import model_segprod

    nk, M = h.nk, h.key.nsq
    _, ct = ciph(h, N, 45)
    rng = np.random.default_rng(46)
    offs = np.array([0, 0, 1, 3, 20, N], dtype=np.int64)
    rows = rng.permutation(N).astype(np.uint32)
    shift = rng.integers(0, 3, N).astype(np.int32)
    want = model_segprod(ct, N, rows, shift, offs, M)
    dc, dr, ds, do, out = st.value(L(ct, nk.cw)), st.resident(rows), st.resident(shift), st.resident(offs), st.out((5, nk.cw))
    return (lambda: nk.lib.pai_ct_segment_prod(nk.pk, dc.ptr, N, 0, dr.ptr, ds.ptr, do.ptr, 5, out.ptr, st.stream)), [(out, L(want, nk.cw))]


def b_sparse_multiexp(h, st, N):
    """12 bases, 30 terms in 5 segments (the second empty, the third of one term); smexp_chunk = 4: chunks and a combine"""
    from tests._fuzz_ext import model_smexp

    nk, M = h.nk, h.key.nsq
    NB, T = 12, 30
    _, base = ciph(h, NB, 47)
    rng = np.random.default_rng(48)
    bidx = rng.integers(0, NB, T).astype(np.int32)
    e = expos(T, 53, 49)
    offs = np.array([0, 4, 4, 5, 17, T], dtype=np.int64)
    want = model_smexp(base, None, NB, bidx, e, None, offs, T, M)
    dc, db, de, do, out = st.value(L(base, nk.cw)), st.resident(bidx), st.value(L(e, 2)), st.resident(offs), st.out((5, nk.cw))
    return (lambda: nk.lib.pai_ct_sparse_multiexp(nk.pk, dc.ptr, None, NB, db.ptr, de.ptr, 2, 53, None, T, do.ptr, 5, out.ptr, st.stream)), \
        [(out, L(want, nk.cw))]


def _pack(step_form):
    def build(h, st, N):
        from tests._fuzz_ext import model_pack_step

        nk, M = h.nk, h.key.nsq
        _, ct = ciph(h, N, 50)
        step, count = (48, 4) if step_form else (16, 3)      # 65 rows: a ragged last chain either way
        want = model_pack_step(ct, step, count, M)
        dc, out = st.value(L(ct, nk.cw)), st.out((len(want), nk.cw))
        fn = nk.lib.pai_ct_pack_step if step_form else nk.lib.pai_ct_pack
        return (lambda: fn(nk.pk, dc.ptr, N, 0, step, count, out.ptr, st.stream)), [(out, L(want, nk.cw))]
    return build


def b_opening_fold(h, st, N):
    """65 openings in segments of 7 (a ragged last one), 40-bit coefficients; open_chunk = 2"""
    from tests._fuzz_ext import model_fold
    from tests._util import pow_many

    nk, key = h.nk, h.key
    rng = random.Random(f"stream-fold/{key.bits}")
    rs = [1, key.n - 1] + [rng.randrange(2, key.n) for _ in range(N - 2)]
    ms = plain(h, N, 51)
    ct = [(1 + m * key.n) % key.nsq * o % key.nsq for m, o in zip(ms, pow_many(rs, key.n, key.nsq))]
    es = expos(N, 40, 52)
    lhs, rhs, flag = model_fold(key, ct, ms, rs, es, 7)
    assert lhs == rhs and flag == 0
    S = len(lhs)
    dc, dm, dr, de = st.value(L(ct, nk.cw)), st.value(L(ms, nk.nw)), st.value(L(rs, nk.nw)), st.value(L(es, 2))
    dl, dh, fl = st.out((S, nk.cw)), st.out((S, nk.cw)), st.resident(np.zeros(1, np.int32))
    return (lambda: nk.lib.pai_opening_fold(nk.pk, dc.ptr, dm.ptr, dr.ptr, N, de.ptr, 2, 40, 7, dl.ptr, dh.ptr, fl.ptr, st.stream)), \
        [(dl, L(lhs, nk.cw)), (dh, L(rhs, nk.cw)), (fl, np.zeros(1, np.int32))]


# ---- threshold decryption and its transcript ------------------------------------------------------------------------------------------
@memo
def _shares(h, t=3, parties=5):
    """a dealt t-of-l sharing of d (d = 0 mod lambda', 1 mod n) as in threshold.py, on Python integers"""
    import math

    key = h.key
    lam = (key.p - 1) * (key.q - 1) // math.gcd(key.p - 1, key.q - 1)
    d = lam * pow(lam, -1, key.n) % (key.n * lam)
    rng = random.Random(f"stream-shares/{key.bits}")
    coef = [d] + [rng.randrange(key.n * lam) for _ in range(t - 1)]
    fact = math.factorial(parties)
    share = {i: sum(c * i ** k for k, c in enumerate(coef)) % (key.n * lam) for i in range(1, parties + 1)}
    return fact, share


def same_r(h, N, seed):
    """N ciphertexts (1 + m_i n) g that share one obfuscator g = hs^(seed + 3): their E-th powers are (1 + (m_i E mod n) n) g^E — one
    long exponentiation on the host for the whole batch instead of one per row (two rows are held to pow())"""
    key = h.key
    m = plain(h, N, seed)
    g = pow(key.hs, seed + 3, key.nsq)
    return m, g, [(1 + x * key.n) % key.nsq * g % key.nsq for x in m]


def same_r_power(h, m, g, ct, E):
    key = h.key
    G = pow(g, E, key.nsq)
    out = [(1 + x * E % key.n * key.n) * G % key.nsq for x in m]
    for i in (0, len(ct) - 1):
        assert out[i] == pow(ct[i], E, key.nsq)
    return out


@memo
def _tpart_operands(h, N):
    fact, share = _shares(h)
    E = 2 * fact * share[2]
    m, g, ct = same_r(h, N, 41)
    return E, ct, same_r_power(h, m, g, ct, E)


def keyshare(h, E, ew):
    """one pai_keyshare per (key, exponent); kept on the handle object and destroyed before it (release_keyshares)"""
    from pailliercryptolib_python_amd import _native

    shares = h.__dict__.setdefault("stream_shares", {})
    if E not in shares:
        sh = C.c_void_p()
        _native.check(h.nk.lib.pai_keyshare_create(h.nk.pk, host_ptr(L([E], ew)), ew, C.byref(sh)))
        shares[E] = sh
    return shares[E]


def release_keyshares(handles):
    for h in handles:
        for sh in h.__dict__.pop("stream_shares", {}).values():
            h.nk.lib.pai_keyshare_destroy(sh)


def b_partial_decrypt(h, st, N):
    nk = h.nk
    E, ct, want = _tpart_operands(h, N)
    ew = (E.bit_length() + 31) // 32
    sh = keyshare(h, E, ew)
    dc, out = st.value(L(ct, nk.cw)), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_partial_decrypt(sh, dc.ptr, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


@memo
def combine_operands(h, N, subset=(1, 2, 4), seed=42):
    """t partial decryptions of N ciphertexts by the parties of `subset`, the Lagrange magnitudes, signs, theta and the plaintexts"""
    import math
    from fractions import Fraction

    key = h.key
    parties = 5
    fact, share = _shares(h)
    m, g, ct = same_r(h, N, seed)
    parts = [same_r_power(h, m, g, ct, 2 * fact * share[i]) for i in subset]
    mu, neg = [], []
    for j in subset:
        v = Fraction(fact)
        for k in subset:
            if k != j:
                v *= Fraction(k, k - j)
        assert v.denominator == 1
        mu.append(abs(2 * int(v)))
        neg.append(1 if v < 0 else 0)
    theta = pow(4 * fact * fact, -1, key.n)
    return m, parts, mu, neg, theta


def b_threshold_combine(h, st, N, subset=(1, 2, 4), seed=42):
    nk = h.nk
    m, parts, mu, neg, theta = combine_operands(h, N, subset, seed)
    t = len(parts)
    dparts = [st.value(L(p, nk.cw)) for p in parts]
    out, fl, rf = st.out((N, nk.nw)), st.resident(np.zeros(1, np.int32)), st.resident(np.zeros(N, np.int32))
    mu_h, neg_h, th_h = L(mu, 1), np.asarray(neg, dtype=np.int32), L([theta], nk.nw)
    ptrs = (C.c_void_p * t)(*[p.ptr.value for p in dparts])
    return (lambda: nk.lib.pai_threshold_combine(nk.pk, ptrs, t, host_ptr(mu_h), host_ptr(neg_h), 1, host_ptr(th_h), N, out.ptr, fl.ptr, rf.ptr,
                                                 st.stream)), [(out, L(m, nk.nw)), (fl, np.zeros(1, np.int32)), (rf, np.zeros(N, np.int32))]


def sha_mats(N, widths, seed):
    rng = np.random.default_rng([seed, len(_SALT[-1]), sum(_SALT[-1].encode())])
    return [rng.integers(0, 1 << 32, size=(N, w), dtype=np.uint64).astype(np.uint32) for w in widths]


def sha_digests(mats):
    n = mats[0].shape[0]
    out = b"".join(hashlib.sha256(b"".join(m[j].tobytes() for m in mats)).digest() for j in range(n))
    return np.frombuffer(out, dtype=np.uint32).reshape(n, 8).copy()


def b_sha256_rows(h, st, N, seed=43):
    nk = h.nk
    widths = (128, 7, 37)
    mats = sha_mats(N, widths, seed)
    dm = [st.value(m) for m in mats]
    out = st.out((N, 8))
    ptrs = (C.c_void_p * 3)(*[d.ptr.value for d in dm])
    words = np.asarray(widths, dtype=np.int32)
    return (lambda: nk.lib.pai_sha256_rows(nk.pk, ptrs, host_ptr(words), 3, N, out.ptr, st.stream)), [(out, sha_digests(mats))]


def b_sha256_expand(h, st, N):
    nk = h.nk
    seed, tag, first, bits = hashlib.sha256(b"stream contract").digest(), b"pai-rho", (1 << 32) - 3, 100
    ew = (bits + 31) // 32
    rows = []
    for j in range(N):
        d = hashlib.sha256(seed + tag + struct.pack("<Q", (first + j) % (1 << 64))).digest()
        rows.append(int.from_bytes(d[:4 * ew], "little") & ((1 << bits) - 1))
    out = st.out((N, ew))
    return (lambda: nk.lib.pai_sha256_expand(nk.pk, seed, tag, len(tag), first, N, bits, out.ptr, ew, st.stream)), [(out, L(rows, ew))]


# ---- codec, randomness, buffers, generic arithmetic -----------------------------------------------------------------------------------
def _codec_x(N, kind):
    rng = np.random.default_rng(50)
    if kind == "f":
        x = rng.uniform(-1e6, 1e6, N)
        x[:3] = [-0.75, 0.0, 1e-200]
        return x
    x = rng.integers(-(1 << 62), 1 << 62, N).astype(np.int64)
    x[:3] = [-1, 0, 2**53]
    return x


def _encode(kind):
    def build(h, st, N):
        from oracle import paillier_oracle as orc

        nk, n = h.nk, h.key.n
        x = _codec_x(N, kind)
        enc = [orc.fp_encode(float(v) if kind == "f" else int(v), n, n // 3 - 1) for v in x]
        dx, dm, de = st.value(x), st.out((N, nk.nw)), st.out((N,), np.int32)
        fn = nk.lib.pai_fp_encode_f64 if kind == "f" else nk.lib.pai_fp_encode_i64
        return (lambda: fn(nk.pk, dx.ptr, N, dm.ptr, de.ptr, st.stream)), \
            [(dm, L([e[0] for e in enc], nk.nw)), (de, np.array([e[1] for e in enc], dtype=np.int32))]
    return build


def b_encode_at(h, st, N):
    nk, n = h.nk, h.key.n
    x = _codec_x(N, "i")
    tg = np.random.default_rng(51).integers(0, 41, N).astype(np.int32)
    dx, dt, dm, de = st.value(x), st.resident(tg), st.out((N, nk.nw)), st.out((N,), np.int32)
    want = [(int(v) << int(t)) % n for v, t in zip(x, tg)]
    return (lambda: nk.lib.pai_fp_encode_at(nk.pk, dx.ptr, 0, N, dt.ptr, 0, dm.ptr, de.ptr, st.stream)), [(dm, L(want, nk.nw)), (de, tg)]


def b_decode(h, st, N):
    nk, n = h.nk, h.key.n
    mant = [int(v) for v in _codec_x(N, "i")]
    dm, do, df = st.value(L([v % n for v in mant], nk.nw)), st.out((N,), np.int64), st.out((N,), np.int32)
    return (lambda: nk.lib.pai_fp_decode_i64(nk.pk, dm.ptr, N, do.ptr, df.ptr, st.stream)), \
        [(do, np.array(mant, dtype=np.int64)), (df, np.zeros(N, np.int32))]


def _pack_vals(N):
    return [int(v) for v in np.random.default_rng(52).integers(-(1 << 14) + 1, 1 << 14, N)]


def b_fp_pack(h, st, N):
    from tests._util import model_pack

    nk, n = h.nk, h.key.n
    ms = _pack_vals(N)
    rows = model_pack(ms, 16, 3, n)
    dx, dm, fl = st.value(np.array(ms, dtype=np.int64)), st.out((len(rows), nk.nw)), st.resident(np.zeros(1, np.int32))
    return (lambda: nk.lib.pai_fp_pack(nk.pk, dx.ptr, 0, N, 0, 14, 16, 3, dm.ptr, fl.ptr, st.stream)), \
        [(dm, L(rows, nk.nw)), (fl, np.zeros(1, np.int32))]


def b_fp_unpack(h, st, N):
    from tests._util import model_pack

    nk, n = h.nk, h.key.n
    ms = _pack_vals(N)
    rows = model_pack(ms, 16, 3, n)
    G = len(rows)
    dm, do, df = st.value(L(rows, nk.nw)), st.out((G * 3,), np.int64), st.out((G,), np.int32)
    want = np.array(ms + [0] * (G * 3 - N), dtype=np.int64)
    return (lambda: nk.lib.pai_fp_unpack(nk.pk, dm.ptr, G, 16, 3, do.ptr, df.ptr, st.stream)), [(do, want), (df, np.zeros(G, np.int32))]


def b_quantize(h, st, N):
    from tests.test_packed_linear_cpu import quantize_model

    nk = h.nk
    K_, M_, ew, wb = N, 4, 2, 40                         # K = 65 rows of 4 weights: 260 values, more than one 256-lane tile
    x = np.random.default_rng(53).integers(-(1 << wb) + 1, 1 << wb, (K_, M_)).astype(np.int64)
    x[:, 2] = 0
    words, sign, sums = quantize_model(x, 0, ew)
    want_sum = np.array([[s & ((1 << 64) - 1), s >> 64] for s in sums], dtype=np.uint64)
    dx, de, ds = st.value(x), st.out((K_ * M_, ew)), st.out((K_ * M_,), np.uint8)
    du, fl = st.out((M_, 2), np.uint64), st.resident(np.zeros(1, np.int32))
    return (lambda: nk.lib.pai_fp_quantize(nk.pk, dx.ptr, 0, K_, M_, M_, 1, 0, wb, None, 0, de.ptr, ew, ds.ptr, du.ptr, fl.ptr, st.stream)), \
        [(de, words.reshape(K_ * M_, ew)), (ds, sign.reshape(-1)), (du, want_sum), (fl, np.zeros(1, np.int32))]


def b_draw_r(h, st, N):
    from oracle import chacha20 as cc

    nk = h.nk
    key, nonce = bytes(range(100, 132)), bytes([0xF0, 0xFF, 0xFF, 0xFF, 1, 2, 3, 4, 5, 6, 7, 8])
    k, nn = np.frombuffer(key, dtype="<u4").copy(), np.frombuffer(nonce, dtype="<u4").copy()
    out = st.out((N, nk.rw))
    want = cc.draw_r_words(key, nonce, 7, N, nk.rw, h.key.randbits)
    return (lambda: nk.lib.pai_draw_r(nk.pk, host_ptr(k), host_ptr(nn), 7, N, out.ptr, st.stream)), [(out, np.asarray(want, dtype=np.uint32))]


def b_buf_slice(h, st, N):
    nk = h.nk
    src = L(ciph(h, N, 60)[1], nk.cw)
    ds, out = st.value(src), st.out((21, nk.cw))
    return (lambda: nk.lib.pai_buf_slice(0, ds.ptr, nk.cw, 3, 21, 3, out.ptr, st.stream)), [(out, src[3:3 + 21 * 3:3])]


def b_buf_rotate(h, st, N):
    nk = h.nk
    src = L(ciph(h, N, 61)[1], nk.cw)
    ds, out = st.value(src), st.out((N, nk.cw))
    return (lambda: nk.lib.pai_buf_rotate(0, ds.ptr, nk.cw, N, -3, out.ptr, st.stream)), [(out, np.roll(src, 3, axis=0))]


_MODULI = {}


def modulus(h):
    """a pai_modulus handle for n^2 of the key (kept for the life of the process: a few kilobytes)"""
    from pailliercryptolib_python_amd import _native

    if h.key.bits not in _MODULI:
        m = C.c_void_p()
        _native.check(h.nk.lib.pai_modulus_create(host_ptr(L([h.key.nsq], h.nk.cw)), h.nk.cw, 0, C.byref(m)))
        _MODULI[h.key.bits] = m
    return _MODULI[h.key.bits]


def b_modmul(h, st, N):
    nk, M = h.nk, h.key.nsq
    a, b = ciph(h, N, 62)[1], ciph(h, N, 63)[1]
    da, db, out = st.value(L(a, nk.cw)), st.value(L(b, nk.cw)), st.out((N, nk.cw))
    m = modulus(h)
    return (lambda: nk.lib.pai_modmul(m, da.ptr, db.ptr, 0, N, out.ptr, st.stream)), [(out, L([x * y % M for x, y in zip(a, b)], nk.cw))]


def b_modexp_fixed(h, st, N, e=(1 << 52) + 0xABCDEF12345):
    nk, M = h.nk, h.key.nsq
    a = ciph(h, N, 64)[1]
    eh = L([e], 2)
    da, out = st.value(L(a, nk.cw)), st.out((N, nk.cw))
    m = modulus(h)
    return (lambda: nk.lib.pai_modexp_fixed(m, da.ptr, host_ptr(eh), 2, N, out.ptr, st.stream)), [(out, L([pow(x, e, M) for x in a], nk.cw))]


def b_modexp_var(h, st, N):
    nk = h.nk
    ct, e, want = _mul_operands(h, N)
    dc, de, out = st.value(L(ct, nk.cw)), st.value(L(e, 2)), st.out((N, nk.cw))
    m = modulus(h)
    return (lambda: nk.lib.pai_modexp_var(m, dc.ptr, 0, de.ptr, 2, 53, 0, N, out.ptr, st.stream)), [(out, L(want, nk.cw))]


BOTH = ("lat", "thr")
TABLE = [
    Row("pai_raw_encrypt", False, {"thr"}, b_raw_encrypt, variants=BOTH),
    Row("pai_ct_add_plain", False, False, b_ct_add_plain, variants=BOTH),
    Row("pai_encrypt", False, True, b_encrypt, variants=BOTH, bits=ALL_BITS),
    Row("pai_obfuscate", False, True, b_obfuscate, variants=BOTH),
    Row("pai_decrypt", False, True, b_decrypt, variants=BOTH, bits=ALL_BITS),
    Row("pai_recover_r", False, True, b_recover_r),
    Row("pai_encrypt_crt", False, True, b_encrypt_crt, bits=ALL_BITS, tune={"crtenc_min": 0}),
    Row("pai_obfuscate_crt", False, True, b_obfuscate_crt, family="crtenc", tune={"crtenc_min": 0}),
    Row("pai_ct_add", False, False, _binary("pai_ct_add", _w_add), variants=BOTH),
    Row("pai_ct_mont_mul", False, False, _binary("pai_ct_mont_mul", _w_mont), variants=BOTH),
    Row("pai_ct_add_aligned", False, False, _binary("pai_ct_add_aligned", _w_aligned), variants=BOTH),
    Row("pai_ct_add_aligned_host", False, False, _binary("pai_ct_add_aligned_host", _w_aligned_host), variants=BOTH),
    Row("pai_ct_add_aligned_dom", False, False, b_add_aligned_dom, variants=BOTH),
    Row("pai_ct_addn", False, False, b_addn),
    Row("pai_ct_mul", False, True, b_ct_mul, variants=BOTH, bits=ALL_BITS),
    Row("pai_ct_mul_host", False, True, b_ct_mul_host, variants=BOTH),
    Row("pai_host_stage", False, False, b_host_stage),
    Row("pai_ct_prod", False, True, b_ct_prod),
    Row("pai_ct_invert", True, True, _invert("sync"), tune={"invert_chunk": 8}),
    Row("pai_ct_invert_async", False, True, _invert("async"), tune={"invert_chunk": 8}),
    Row("pai_ct_invert_flag", False, True, _invert("flag"), tune={"invert_chunk": 8}),
    Row("pai_ct_pow2", True, {"pow2digit"}, _pow2(False), variants=("lat", "thr", "pow2digit")),
    Row("pai_ct_pow2_hint", False, {"pow2digit"}, _pow2(True), variants=("lat", "thr", "pow2digit")),
    Row("pai_pubkey_status", True, False, b_status),
    Row("pai_ct_multiexp", False, True, b_multiexp),
    Row("pai_ct_segment_prod", True, True, b_segment_prod, family="segprod", bits=ALL_BITS, tune={"segprod_chunk": 3}),
    Row("pai_ct_scan", False, True, b_scan, bits=ALL_BITS, tune={"scan_chunk": 5}),
    Row("pai_ct_sparse_multiexp", True, True, b_sparse_multiexp, family="smexp", bits=ALL_BITS, tune={"smexp_chunk": 4}),
    Row("pai_ct_pack", True, True, _pack(False), family="pack"),
    Row("pai_ct_pack_step", True, True, _pack(True), family="pack"),
    Row("pai_opening_fold", True, True, b_opening_fold, family="open", bits=ALL_BITS, tune={"open_chunk": 2}),
    Row("pai_partial_decrypt", False, True, b_partial_decrypt, variants=BOTH, bits=ALL_BITS, N=N_LANES, tune={"tpart_min": 0}),
    Row("pai_threshold_combine", False, True, b_threshold_combine, bits=ALL_BITS, N=N_LANES, tune={"tcomb_min": 0}),
    Row("pai_sha256_rows", False, True, b_sha256_rows, N=N_LANES, tune={"sha_grid": 1}),
    Row("pai_sha256_expand", False, True, b_sha256_expand, N=N_LANES, tune={"sha_grid": 1}),
    Row("pai_fp_encode_f64", False, False, _encode("f"), N=N_LANES),
    Row("pai_fp_encode_i64", False, False, _encode("i"), N=N_LANES),
    Row("pai_fp_encode_at", False, False, b_encode_at, N=N_LANES),
    Row("pai_fp_decode_i64", False, False, b_decode, N=N_LANES),
    Row("pai_fp_pack", False, False, b_fp_pack, N=N_LANES),
    Row("pai_fp_unpack", False, False, b_fp_unpack, N=N_LANES),
    Row("pai_fp_quantize", False, True, b_quantize),
    Row("pai_draw_r", False, False, b_draw_r),
    Row("pai_buf_slice", False, False, b_buf_slice),
    Row("pai_buf_rotate", False, False, b_buf_rotate),
    Row("pai_modmul", False, False, b_modmul),
    Row("pai_modexp_fixed", False, True, b_modexp_fixed),
    Row("pai_modexp_var", False, True, b_modexp_var),
]
BY_NAME = {r.name: r for r in TABLE}


def chained_in(row, variant):
    return variant in row.chained if isinstance(row.chained, (set, frozenset)) else bool(row.chained)


def env_of(row, variant):
    """the environment of one (row, variant): the variant's switches and PAI_TUNE with the row's knobs"""
    env = dict(VARIANTS[variant])
    tune = dict(BASE_TUNE)
    tune.update(row.tune or {})
    env["PAI_TUNE"] = ",".join(f"{k}={v}" for k, v in tune.items())
    return env
