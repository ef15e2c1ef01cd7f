"""GPU: threshold decryption — pai_partial_decrypt, pai_threshold_combine (csrc/dispatch_threshold.hpp, kernels_threshold.hpp:
k_tcomb_padic, k_tfinish) and PaillierPrivateKey.share / PaillierKeyShare.partial_decrypt / PaillierPublicKey.combine*.

Every expectation is a CPython integer, bit-equal or wrong.  Partial decryptions are held, every row, to pow_many(cts, 2 Delta s_i,
n^2).  The combine is fed partials made by the oracle, never by the kernel under test: its rows are c_k = g^(a_k) mod n^2 for one
DJN encryption g of a known m0 and random 64-bit a_k, so that c_k decrypts to m0 a_k mod n and its partial under exponent E is
(g^E)^(a_k) — one wide CPython pow per share instead of one per row (three rows per case are checked against the direct pow).
The profile is on: every case asserts which route ran."""
import ctypes as C
import math
import pickle

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import (PaillierKeyShare, PaillierPartialDecryption, PaillierPrivateKey, PaillierPublicKey, _native,
                                          engine)
from pailliercryptolib_python_amd import threshold as th
from pailliercryptolib_python_amd.bindings import ipclPublicKey
from tests._arena import ALIGNS, FILLERS, Arena
from tests._util import DevArray, disable, djn_encrypt_many, host_ptr, ints_to_limbs, limbs_to_ints, pow_many, tune
from tests.test_gpu_crt_encrypt import keys
from tests.test_gpu_paillier_abi import NativeKey
from tests.test_recover_cpu import all_keys

pytestmark = pytest.mark.gpu

POW, TCOMB, TFIN = "k_pow_padic", "k_tcomb_padic", "k_tfinish"
PAI_E_INVALID = -1


@pytest.fixture(autouse=True)
def profiled():
    engine.profile_enable(True)
    yield
    engine.profile_enable(False)


def dev(h, ints, words):
    return engine.to_device_words(engine.ints_to_words(ints, words), h.device)


def ints(t):
    return engine.words_to_ints(engine.to_host_words(t))


_SHARES = {}


def dealt(bits, parties, threshold):
    """[s_1 .. s_l] of keys(bits), dealt once per shape from a fixed seed"""
    k = (bits, parties, threshold)
    if k not in _SHARES:
        key = keys(bits)[0]
        _SHARES[k] = th.deal(key.p, key.q, parties, threshold, th.SeededRng(bits + 31 * parties + threshold))[1]
    return _SHARES[k]


def exponent(bits, parties, threshold, index):
    return 2 * math.factorial(parties) * dealt(bits, parties, threshold)[index - 1]


# ---- partial decryptions against pow_many, every row ------------------------------------------------------------------------------------
def partial(pk, E, cts):
    h = pk.pubkey.handle
    sh = engine.KeyShareHandle(h, E)
    got = ints(sh.partial_decrypt(dev(h, cts, h.ct_words)))
    return got, engine.profile_last()


@pytest.mark.parametrize("bits", (1024, 2048, 3072, 4096))
def test_partials_key_sizes(bits):
    key, pk, sk = keys(bits)
    N = 37 if bits <= 2048 else 9
    vals = [float(v) for v in np.random.default_rng(bits).uniform(-1000, 1000, N)]
    en = pk.encrypt(vals, r=orc.synth_r_limbs(bits + 5, N, key.randbits))
    cts = [int(c) for c in en.ciphertextBN()]
    shares = sk.share(3, 2, seed=bits)
    assert [s.index for s in shares] == [1, 2, 3]
    for sh in (shares[0], shares[2]):
        E = sh.exponent()
        assert E.bit_length() <= 2 * bits + 46
        part = sh.partial_decrypt(en)
        prof = engine.profile_last()
        assert "k_ctmul" in prof and POW not in prof, prof                 # a small batch: the routes of pai_ct_mul
        print(f"ROUTE partial {bits} bits, N = {N}: {sorted(prof)}")
        assert isinstance(part, PaillierPartialDecryption) and (part.index, part.parties, part.threshold) == (sh.index, 3, 2)
        assert len(part) == N and part.rows == N and part._expo.tolist() == en.exponent()
        assert ints(part.words(pk.pubkey.handle.device)) == pow_many(cts, E, key.nsq)


_POOL = {}


def pool(bits, count):
    """`count` random residues modulo n^2 and their powers under share 2 of (3, 2), once per key size"""
    if bits not in _POOL:
        key = keys(bits)[0]
        rng = np.random.default_rng(bits + 19)
        cts = [int.from_bytes(rng.bytes(bits // 4 + 8), "little") % key.nsq for _ in range(count)]
        E = exponent(bits, 3, 2, 2)
        _POOL[bits] = (cts, E, pow_many(cts, E, key.nsq))
    assert len(_POOL[bits][0]) == count
    return _POOL[bits]


@pytest.mark.parametrize("shape", ("1", "255", "256", "257", "513:grid1"))
def test_partials_digit_route_1024(shape, monkeypatch):
    key, pk, _ = keys(1024)
    cts, E, want = pool(1024, 513)
    N = int(shape.split(":")[0])
    tune(monkeypatch, "tpart_min", 0)
    if shape.endswith("grid1"):
        tune(monkeypatch, "tpart_grid", 1)                    # one workgroup walks three tiles, the last one ragged
    off = len(cts) - N                                        # (every shape ends on the pool's last row)
    got, prof = partial(pk, E, cts[off:])
    assert POW in prof and "k_ctmul" not in prof, prof
    assert got == want[off:], shape


@pytest.mark.parametrize("N", (37, 257))
def test_partials_digit_route_2048(N, monkeypatch):
    key, pk, _ = keys(2048)
    cts, E, want = pool(2048, 257)
    tune(monkeypatch, "tpart_min", 0)
    got, prof = partial(pk, E, cts[-N:])
    assert POW in prof, prof
    assert got == want[-N:]
    tune(monkeypatch, "tpart_min", None)
    got2, prof2 = partial(pk, E, cts[-37:])                    # the routes give the same bits
    assert POW not in prof2 and "k_ctmul" in prof2, prof2
    assert got2 == want[-37:]


@pytest.mark.parametrize("bits", (1024, 2048, 3072))
def test_partials_corner_rows(bits, monkeypatch):
    key, pk, _ = keys(bits)
    n, nsq = key.n, key.nsq
    full = int.from_bytes(np.random.default_rng(bits).bytes(bits // 4), "little") % nsq | 1 << (nsq.bit_length() - 2)
    cts = [1, nsq - 1, n + 1, full]
    E = exponent(bits, 3, 2, 1)
    want = [pow(c, E, nsq) for c in cts]
    assert want[0] == 1 and want[1] == 1 and want[2] == (1 + E % n * n) % nsq
    for force in (False, True):
        tune(monkeypatch, "tpart_min", 0 if force else None)
        got, prof = partial(pk, E, cts)
        assert (POW in prof) == (force and bits <= 2048), (bits, force, prof)
        assert got == want, (bits, force)


# ---- the combine, on partials made by the oracle -------------------------------------------------------------------------------------------
CASES = {"5,3:123": (5, 3, (1, 2, 3)), "5,3:135": (5, 3, (1, 3, 5)), "5,3:245": (5, 3, (2, 4, 5)), "4,1:3": (4, 1, (3,)),
         "16,16": (16, 16, tuple(range(1, 17)))}
_ROWS = {}


def rows(bits):
    """(g, a_k, c_k = g^(a_k), m_k = m0 a_k mod n), once per key size: 513 rows at 1024 bits (three tiles), 257 above"""
    if bits not in _ROWS:
        count = 513 if bits == 1024 else 257
        key = keys(bits)[0]
        rng = np.random.default_rng(bits + 23)
        m0 = int.from_bytes(rng.bytes(bits // 8 + 8), "little") % key.n
        g = orc.encrypt(key, m0, int.from_bytes(rng.bytes(key.randbits // 8), "little"))
        a = [1] + [int.from_bytes(rng.bytes(8), "little") | 1 << 63 for _ in range(count - 1)]
        c = [pow(g, ak, key.nsq) for ak in a]
        m = [m0 * ak % key.n for ak in a]
        assert orc.decrypt_crt(key, c[-1]) == m[-1] and orc.decrypt_crt(key, c[0]) == m0
        _ROWS[bits] = (g, a, c, m)
    return _ROWS[bits]


_PARTS = {}


def oracle_partials(bits, parties, threshold, index):
    """the partial decryptions of rows(bits) under share `index`: (g^E)^(a_k), three rows checked against c_k^E"""
    k = (bits, parties, threshold, index)
    if k not in _PARTS:
        key = keys(bits)[0]
        g, a, c, _ = rows(bits)
        E = exponent(bits, parties, threshold, index)
        gE = pow(g, E, key.nsq)
        out = [pow(gE, ak, key.nsq) for ak in a]
        for i in (0, len(a) // 2, len(a) - 1):
            assert out[i] == pow(c[i], E, key.nsq)
        _PARTS[k] = out
    return _PARTS[k]


def run_combine(pk, parties, subset, parts_ints):
    h = pk.pubkey.handle
    mags, negs = th.lagrange(list(subset), parties)
    m, flag, rowflag = h.threshold_combine([dev(h, p, h.ct_words) for p in parts_ints], [2 * v for v in mags], negs, th.theta(pk.n, parties))
    prof = engine.profile_last()
    return ints(m), int(flag.item()), rowflag.cpu().numpy(), prof


COMBINE_CASES = [(bits, case) for bits in (1024, 2048, 3072) for case in CASES if case != "16,16" or bits == 1024]      # (16, 16) at 1024 bits only


@pytest.mark.parametrize("bits,case", COMBINE_CASES)
def test_combine_on_oracle_partials(bits, case, monkeypatch):
    key, pk, _ = keys(bits)
    parties, threshold, subset = CASES[case]
    _, _, _, want = rows(bits)
    parts = [oracle_partials(bits, parties, threshold, i) for i in subset]
    mags, negs = th.lagrange(list(subset), parties)
    assert (case == "4,1:3") == (not any(negs))               # (4, 1) has no negative side
    fusable = bits <= 2048
    shapes = [(1, None), (256, None), (257, None)] + ([(513, 1)] if bits == 1024 else [])
    for N, grid in shapes:
        res = {}
        for route in ("fused", "composition"):
            disable(monkeypatch, "tcombine", route == "composition")
            tune(monkeypatch, "tcomb_min", 0)
            tune(monkeypatch, "tcomb_grid", grid)
            got, flag, rowflag, prof = run_combine(pk, parties, subset, [p[-N:] for p in parts])
            assert TFIN in prof, prof
            assert (TCOMB in prof) == (route == "fused" and fusable), (bits, case, N, route, prof)
            if (route == "composition" or not fusable) and (fusable or max(2 * v for v in mags).bit_length() > 8):
                assert "k_ctmul" in prof, prof                # (beyond the digit engine pai_ct_mul times exponents above 8 bits only)
            assert flag == 0 and not rowflag.any()
            assert got == want[-N:], (bits, case, N, route)
            res[route] = got
        assert res["fused"] == res["composition"]


# ---- flags and refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("fused", "composition"))
def test_flags(route, monkeypatch):
    bits, N = 1024, 37
    key, pk, _ = keys(bits)
    disable(monkeypatch, "tcombine", route == "composition")
    tune(monkeypatch, "tcomb_min", 0)
    parties, subset = 5, (1, 3, 5)
    mags, negs = th.lagrange(list(subset), parties)
    assert negs == [False, True, False]                       # share 3 is the negative side of {1, 3, 5}
    _, _, _, want = rows(bits)
    parts = [list(oracle_partials(bits, 5, 3, i)[-N:]) for i in subset]
    bad = [list(p) for p in parts]
    bad[0][11] = parts[0][12]                                 # one row of one partial replaced by another unit
    got, flag, rowflag, _ = run_combine(pk, parties, subset, bad)
    assert flag == 1 and np.flatnonzero(rowflag).tolist() == [11]
    assert [g for i, g in enumerate(got) if i != 11] == [w for i, w in enumerate(want[-N:]) if i != 11]
    expo = np.zeros(N, dtype=np.int32)
    h = pk.pubkey.handle
    objs = [PaillierPartialDecryption(pk, dev(h, p, h.ct_words), i, 5, 3, expo, N) for p, i in zip(bad, subset)]
    with pytest.raises(ValueError, match="1 of 37 rows .*row 11"):
        pk.combine_raw(objs)
    good = [PaillierPartialDecryption(pk, dev(h, p, h.ct_words), i, 5, 3, expo, N) for p, i in zip(parts, subset)]
    assert pk.combine_raw(good) == want[-N:]
    bad = [list(p) for p in parts]
    bad[1][5] = key.p * 987654321                             # a row of the negative side that is no unit
    got, flag, rowflag, _ = run_combine(pk, parties, subset, bad)
    assert flag & 2
    objs = [PaillierPartialDecryption(pk, dev(h, p, h.ct_words), i, 5, 3, expo, N) for p, i in zip(bad, subset)]
    with pytest.raises(ValueError, match="not invertible"):
        pk.combine_raw(objs)
    # the Python refusals: t - 1 parts, a duplicate, mixed shapes
    other = PaillierPartialDecryption(pk, dev(h, parts[0][:5], h.ct_words), 2, 5, 3, expo[:5], 5)
    for unusable in (good[:2], [good[0], good[1], good[1]], [good[0], good[1], other]):
        with pytest.raises(ValueError):
            pk.combine_raw(unusable)


def test_native_refusals():
    key, pk, _ = keys(1024)
    h = pk.pubkey.handle
    lib = h.lib
    part = dev(h, [1, 1], h.ct_words)
    m, flag = h.empty_pt(2), h.new_flag()
    ptrs = (C.c_void_p * 17)(*([part.data_ptr()] * 17))
    mu = np.ones((17, 4), dtype=np.uint32)
    neg = np.zeros(17, dtype=np.int32)
    theta = engine.int_to_words(1, h.n_words)

    def call(t, mu_words=4, mu_=mu, out=m, theta_=theta):
        return lib.pai_threshold_combine(h.h, ptrs, t, host_ptr(mu_), host_ptr(neg), mu_words, host_ptr(theta_), 2, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(flag.data_ptr()), None, None)

    zero = mu.copy()
    zero[1] = 0
    for rc in (call(0), call(17), call(2, mu_words=0), call(2, mu_words=5), call(2, mu_=zero), call(2, out=part),
               call(2, theta_=engine.int_to_words(key.n, h.n_words))):
        assert rc == PAI_E_INVALID
    assert call(2) == 0 and int(flag.item()) == 0 and ints(m) == [0, 0]          # 1^2 = 1: L = 0
    sh = engine.KeyShareHandle(h, 12345)
    ct = dev(h, [5, 7, 9], h.ct_words)
    with pytest.raises(_native.NativeError) as ei:
        sh.partial_decrypt(ct, out=ct)
    assert ei.value.code == PAI_E_INVALID and "overlaps" in str(ei.value)
    with pytest.raises(_native.NativeError):
        sh.partial_decrypt(ct, out=ct[1:])
    assert ints(ct) == [5, 7, 9]
    with pytest.raises(_native.NativeError):
        engine.KeyShareHandle(h, 0)


# ---- through the API ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("djn", "standard"))
@pytest.mark.parametrize("route", ("default", "fused"))
def test_through_the_api(scheme, route, monkeypatch):
    key, pk, sk = keys(2048)
    if scheme == "standard":
        pk = PaillierPublicKey(ipclPublicKey(key.n, 2048, False))
        sk = PaillierPrivateKey(pk, key.p, key.q)
    if route == "fused":
        tune(monkeypatch, "tcomb_min", 0)
    shares = sk.share(5, 3, seed=2048)
    assert all(isinstance(s, PaillierKeyShare) for s in shares) and shares == sk.share(5, 3, seed=2048)
    shares = pickle.loads(pickle.dumps(shares))
    rng = np.random.default_rng(11)
    x = pk.encrypt([0.5, -3.0, 7.25, 1e6, 3.0, -1e-3, 12345.0, 2.0 ** -20])          # mixed exponents
    y = pk.encrypt([float(v) for v in rng.uniform(-10, 10, 8)])
    ids = np.array([0, 0, 1, 1, 1, 2, 2, 3])
    containers = [x, x + y, x * -2.5, pk.encrypt([1, 2, 3, 4, 5, 6, 7, 8]).segment_sum(ids, 4).cumsum()]
    for subset in ((1, 2, 3), (5, 2, 4)):
        for c in containers:
            parts = [shares[i - 1].partial_decrypt(c) for i in subset]
            parts = pickle.loads(pickle.dumps(parts))
            assert all(isinstance(p._t, np.ndarray) for p in parts)                  # wire-form words
            raw = pk.combine_raw(parts)
            prof = engine.profile_last()
            assert TFIN in prof and (TCOMB in prof) == (route == "fused"), prof
            assert raw == sk.raw_decrypt(c)
            assert pk.combine(parts) == sk.decrypt(c)
            assert np.array_equal(pk.combine_to_numpy(parts), sk.decrypt_to_numpy(c))
        packed = containers[3].pack(slot_bits=32, value_bits=16)
        parts = [shares[i - 1].partial_decrypt(packed) for i in subset]
        assert parts[0].packing == (packed.slot_bits, packed.slots, packed.exponent, packed.value_bits) and parts[0]._expo is None
        assert np.array_equal(pk.combine_packed(pickle.loads(pickle.dumps(parts))), sk.decrypt_packed(packed))
        with pytest.raises(ValueError):
            pk.combine(parts)
    one = pk.encrypt(4.5)
    assert pk.combine([s.partial_decrypt(one) for s in shares]) == sk.decrypt(one) == 4.5          # more than threshold parts; a scalar
    with pytest.raises(ValueError):
        pk.combine([shares[0].partial_decrypt(x), shares[1].partial_decrypt(x)])
    with pytest.raises(ValueError):
        pk.combine([shares[0].partial_decrypt(x), shares[1].partial_decrypt(x), shares[2].partial_decrypt(y[:4])])
    with pytest.raises(ValueError):
        keys(1024)[1].combine([s.partial_decrypt(x) for s in shares[:3]])


# ---- structured and limit keys -------------------------------------------------------------------------------------------------------------
ALL_KEYS = all_keys()
SERVED, REFUSED = set(), {}


@pytest.mark.parametrize("ident,p,q", ALL_KEYS, ids=[e[0] for e in ALL_KEYS])
def test_structured_and_limit_keys(ident, p, q):
    """(3, 2), five DJN ciphertexts, shares 1 and 3 through pai_partial_decrypt, then pai_threshold_combine: raw_decrypt's residues.
    gcd(n, lcm(p - 1, q - 1)) = 1 holds for all 42 keys (tests/test_recover_cpu.py): none is refused."""
    bits = 2 * max(p.bit_length(), q.bit_length())
    try:
        _, shares = th.deal(p, q, 3, 2, th.SeededRng(p % (1 << 32)))
    except ValueError as e:
        REFUSED[ident] = str(e)
        return
    djn = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=bits)
    nk = NativeKey(orc.make_key(p, q, djn_x=None, bits=bits))
    lib = nk.lib
    rng = np.random.default_rng(p % (1 << 32))
    ms = [0, djn.n - 1] + [int.from_bytes(rng.bytes(bits // 8 + 8), "little") % djn.n for _ in range(3)]
    rs = [1, (1 << djn.randbits) - 1] + orc.limbs_to_ints(orc.synth_r_limbs(bits, 3, djn.randbits))
    cts = djn_encrypt_many(djn, ms, rs)                        # (the C oracle: CPython's pow costs seconds per key at these widths)
    assert cts[0] == orc.encrypt(djn, ms[0], rs[0]) and orc.decrypt_crt(djn, cts[4]) == ms[4]
    ct = DevArray(ints_to_limbs(cts, nk.cw))
    outs = []
    for i in (1, 3):
        E = 2 * 6 * shares[i - 1]
        ew = (E.bit_length() + 31) // 32
        sh = C.c_void_p()
        _native.check(lib.pai_keyshare_create(nk.pk, host_ptr(ints_to_limbs([E], ew)), ew, C.byref(sh)))
        out = DevArray(shape=(5, nk.cw))
        _native.check(lib.pai_partial_decrypt(sh, ct.ptr, 5, out.ptr, None))
        lib.pai_keyshare_destroy(sh)
        outs.append(out)
    assert limbs_to_ints(outs[1].get()) == pow_many(cts, 12 * shares[2], djn.nsq, check=1), ident
    mags, negs = th.lagrange([1, 3], 3)
    ptrs = (C.c_void_p * 2)(outs[0].ptr, outs[1].ptr)
    m, flag = DevArray(shape=(5, nk.nw)), DevArray(np.zeros(1, dtype=np.int32))
    _native.check(lib.pai_threshold_combine(nk.pk, ptrs, 2, host_ptr(ints_to_limbs([2 * v for v in mags], 4)),
                                            host_ptr(np.asarray(negs, dtype=np.int32)), 4, host_ptr(ints_to_limbs([th.theta(djn.n, 3)], nk.nw)),
                                            5, m.ptr, flag.ptr, None, None))
    assert TFIN in engine.profile_last()
    assert int(flag.get()[0]) == 0, ident
    assert limbs_to_ints(m.get()) == ms, ident
    SERVED.add(ident)
    del nk


def test_structured_key_coverage():
    """runs behind test_structured_and_limit_keys (the module's order)"""
    print(f"COVERAGE threshold decryption on structured and limit keys: {len(SERVED)} of {len(ALL_KEYS)} keys, refused: {sorted(REFUSED)}")
    assert len(ALL_KEYS) == 42 and len(SERVED) >= 40 and len(SERVED) + len(REFUSED) == 42, (sorted(REFUSED), len(SERVED))
    assert len(SERVED) == 42                                  # checked on the CPU: every one of the 42 keys can be shared


# ---- the memory contract ---------------------------------------------------------------------------------------------------------------------
def arena_sweep(build):
    """build(place) -> (call, expected); both alignment classes, both fillers; the whole arena is compared after the call"""
    lib = _native.load()
    for al in ALIGNS:
        for fill in FILLERS:
            ar = Arena(fill)
            try:
                call, expected = build(lambda name, host=None, **kw: ar.place(name, host, align=al, **kw))
                ar.commit()
                rc = call()
                _native.check(lib.pai_stream_sync(0, None))
                if expected is None:
                    assert rc == PAI_E_INVALID, rc
                    ar.check({})                              # refused: nothing written
                else:
                    _native.check(rc)
                    ar.check(expected)
            finally:
                ar.free()


@pytest.mark.parametrize("bits,N,force", ((1024, 257, True), (1024, 5, False), (3072, 5, False)))
def test_memory_contract_partial_decrypt(bits, N, force, monkeypatch):
    key, pk, _ = keys(bits)
    h = pk.pubkey.handle
    tune(monkeypatch, "tpart_min", 0 if force else None)
    if bits == 1024:
        cts, E, want = pool(1024, 513)
        cts, want = cts[-N:], want[-N:]
    else:
        cts = rows(bits)[2][-N:]
        E = exponent(bits, 5, 3, 1)
        want = oracle_partials(bits, 5, 3, 1)[-N:]
    sh = engine.KeyShareHandle(h, E)

    def served(P):
        ct = P("ct", ints_to_limbs(cts, h.ct_words))
        out = P("out", shape=(N, h.ct_words))
        return (lambda: h.lib.pai_partial_decrypt(sh.h, ct.ptr, N, out.ptr, None)), {"out": ints_to_limbs(want, h.ct_words)}

    arena_sweep(served)
    assert (POW in engine.profile_last()) == force

    def overlapping(P):
        ct = P("ct", ints_to_limbs(cts + cts[:1], h.ct_words))
        return (lambda: h.lib.pai_partial_decrypt(sh.h, ct.ptr, N, ct.at(1), None)), None

    def in_place(P):
        ct = P("ct", ints_to_limbs(cts, h.ct_words))
        return (lambda: h.lib.pai_partial_decrypt(sh.h, ct.ptr, N, ct.ptr, None)), None

    arena_sweep(overlapping)
    arena_sweep(in_place)


@pytest.mark.parametrize("bits,N,route", ((1024, 257, "fused"), (1024, 257, "composition"), (1024, 1, "fused"), (3072, 5, "composition")))
def test_memory_contract_combine(bits, N, route, monkeypatch):
    key, pk, _ = keys(bits)
    h = pk.pubkey.handle
    disable(monkeypatch, "tcombine", route == "composition")
    tune(monkeypatch, "tcomb_min", 0)
    parties, subset = 5, (1, 3, 5)
    mags, negs = th.lagrange(list(subset), parties)
    parts = [oracle_partials(bits, 5, 3, i)[-N:] for i in subset]
    want = rows(bits)[3][-N:]
    mu = ints_to_limbs([2 * v for v in mags], 4)
    ng = np.asarray(negs, dtype=np.int32)
    theta = ints_to_limbs([th.theta(key.n, parties)], h.n_words)

    def call_with(regs, m, flag, rowflag):
        def call():                                           # (pointers exist once the arena is committed)
            ptrs = (C.c_void_p * 3)(*[r.address for r in regs])
            return h.lib.pai_threshold_combine(h.h, ptrs, 3, host_ptr(mu), host_ptr(ng), 4, host_ptr(theta), N, m.ptr, flag.ptr,
                                               rowflag.ptr if rowflag is not None else None, None)
        return call

    def served(P):
        regs = [P(f"part{i}", ints_to_limbs(p, h.ct_words)) for i, p in zip(subset, parts)]
        m = P("m", shape=(N, h.n_words))
        flag = P("flag", np.zeros(1, dtype=np.int32))
        rowflag = P("rowflag", np.zeros(N, dtype=np.int32))
        return call_with(regs, m, flag, rowflag), {"m": ints_to_limbs(want, h.n_words)}

    arena_sweep(served)
    prof = engine.profile_last()
    assert TFIN in prof and (TCOMB in prof) == (route == "fused" and bits <= 2048), prof

    def overlapping(P):
        regs = [P(f"part{i}", ints_to_limbs(p, h.ct_words)) for i, p in zip(subset, parts)]
        flag = P("flag", np.zeros(1, dtype=np.int32))
        return call_with(regs, regs[2], flag, None), None

    arena_sweep(overlapping)
