"""GPU: every kernel family against CPython integers on the structured keys of tests/golden/extreme_keys.json (families and
their purpose: tests/golden/make_extreme_keys.py; their structure is held by tests/test_extreme_keys_cpu.py).  Every other key
of the suite is random, while the kernels' carry, borrow and lazy-bound arguments depend on the modulus: limbs of 2^29 - 1 or 0
in p, q, n and n^2, quotient digits with n0inv = 2^29 - 1 or 1, Karatsuba halves of the prime at opposite extremes, and primes
at the widest size a digit geometry admits (676 / 1604 / 2068 bits = 29 NL - 20 on 24 / 56 / 72 limbs, n of 3208 / 4136 bits on
the 112- / 144-limb pair geometries, limits 3228 / 4156: the values of padic_nl_for_prime_bits, pair_nl_for_prime_bits and
pair_nl_for_n_bits in the tree).

One module-scoped pair of handles per key (DJN, fixed x); creating them and the lazily built tables (fixed-base, digit-engine,
pair, latency, mid-size) is part of the test: any status but PAI_OK fails it.  Every comparison is bit-exact; bulk powers go
through tests/_util.pow_many (the C oracle, spot-checked against CPython's pow at every call).  Batches are one full and one
ragged workgroup tile (70 at 64 elements per tile, 37 at 32; 257 for the 256-element tile of k_dec_a_padic).  The ciphertext
operands of a test are the 10 corner values, the 49 cells of the CRT grid and a pattern tail (runs of ones, single bits, values
next to 0 and M): 70 of them, which is one batch at the 64-element tiles and, with four more pattern values, two batches of 37
at the 32-element tiles — every forced family sees every corner and the tail at every width.  Paths are forced with the suite's knobs, and what ran is read back (pai_profile_last / pai_profile_last_path):
a throughput, mid-size or window path that was asked for must be the one that ran; the four-wave and wave-pair paths depend on
per-key constants (csrc/dispatch_decrypt.hpp: build_pp_consts; capi_pubkey_tables.hpp: ensure_lat_ctx), so there the test accepts
the documented hand-down (pp -> rl -> window), records what ran, and the last test requires every family to have run on some key.
Ciphertext corners that are no units modulo n (0, n, M - n, (n - 1) n) have no decryption under the oracle (its L function
asserts): they go through the products, powers and sums, not through pai_decrypt or pai_ct_invert."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from tests._util import DevArray, djn_encrypt_many, djn_obfuscate_many, ints_to_limbs, limbs_to_ints, pow_many, tune
from tests._util import disable as knob_disable
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_padic_kara_mul import MODES, crt
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels

pytestmark = pytest.mark.gpu

ENTRIES = load_extreme_keys()
DJN_X = (1 << 70) + 12345
SEEN = {}            # (op, prime_bits) -> set of "kernel:path" that ran
VISITED = set()


class Key:
    def __init__(self, ident, family, b, p, q):
        self.ident, self.family, self.b = ident, family, b
        self.key = orc.make_key(p, q, djn_x=DJN_X, bits=2 * b)
        self.nk = NativeKey(self.key)
        self.N = 70 if 2 * b < 4000 else 37               # a full and a ragged tile at 64 / 32 elements per workgroup
        self.T = 70 if self.N == 70 else 74               # operands of a test: one batch of 70 or two of 37 (corners, CRT grid, pattern tail)
        self.offs = range(0, self.T, self.N)
        self.consts = orc.crt_constants(self.key)


@pytest.fixture(scope="module", params=ENTRIES, ids=[e[0] for e in ENTRIES])
def xk(request):
    _native.check(_native.load().pai_profile_enable(1))
    k = Key(*request.param)
    VISITED.add(k.ident)
    yield k
    _native.check(k.nk.lib.pai_profile_enable(0))


def ran(k, op):
    """the kernels of the calling thread's last library call as "name:path", recorded per (operation, prime width)"""
    lib = k.nk.lib
    names = _last_kernels(lib)
    buf = C.create_string_buffer(64)
    out = []
    for i, nm in enumerate(names):
        _native.check(lib.pai_profile_last_path(i, buf, 64))
        out.append(f"{nm}:{buf.value.decode()}")
    SEEN.setdefault((op, k.b), set()).update(out)
    return out


def pattern(M, n, seed):
    """tools/fuzz_gpu.py::pattern, seeded: values next to 0 and M, runs of ones from the bottom and from the top, single bits, random"""
    rng = random.Random(seed)
    bits = M.bit_length()
    out = []
    for i in range(n):
        kind = i % 8
        if kind == 0: v = rng.randrange(3)
        elif kind == 1: v = M - 1 - rng.randrange(3)
        elif kind == 2: v = (1 << rng.randrange(1, bits)) - 1
        elif kind == 3: v = ((1 << bits) - 1) ^ ((1 << rng.randrange(1, bits)) - 1)
        elif kind == 4: v = 1 << rng.randrange(bits)
        else: v = rng.getrandbits(bits + 64)
        out.append(v % M)
    return out


def ciphertexts(k, n, seed, units=False):
    key = k.key
    nn, M, p2, q2 = key.n, key.nsq, key.p * key.p, key.q * key.q
    front = [0, 1, 2, nn - 1, nn, nn + 1, M - 1, M - 2, M - nn, (nn - 1) * nn]
    sp = [1, p2 - 1, 2, p2 - 2, key.p + 1, p2 - key.p - 1, (p2 - 1) // 2]
    sq = [1, q2 - 1, q2 - 2, 2, key.q + 1, q2 - key.q - 1, (q2 - 1) // 2]
    grid = [crt(a, b, p2, q2) for a in sp for b in sq]          # test_gpu_padic_kara_mul.py::corner_cts with this key's primes
    out = front + grid + pattern(M, max(0, n - len(front) - len(grid)), seed)
    if units:
        out = [c for c in out if math.gcd(c, nn) == 1]
        out += [c | 1 if math.gcd(c | 1, nn) == 1 else 1 for c in pattern(M, n, seed + 1)]
    return out[:n]


def plain(k, n, seed):
    key = k.key
    return ([0, 1, key.n - 1, key.p, key.q, key.n - key.p, key.n - key.q] + pattern(key.n, n, seed))[:n]


def rand_r(k, n, seed):
    rb = k.key.randbits
    return ([0, (1 << rb) - 1, 1 << (rb - 1)] + pattern(1 << rb, n, seed))[:n]


def decrypt_many(k, cts):
    """[orc.decrypt_crt(key, c)] with the two half-size powers of each ciphertext through pow_many"""
    key, kc = k.key, k.consts
    p, q = key.p, key.q
    up = pow_many([c % (p * p) for c in cts], p - 1, p * p)
    uq = pow_many([c % (q * q) for c in cts], q - 1, q * q)
    out = []
    for a, b in zip(up, uq):
        mp = orc._lfun(a, p) * kc["hp"] % p
        mq = orc._lfun(b, q) * kc["hq"] % q
        out.append(mp + p * ((mq - mp) * kc["pinv_q"] % q))
    return out


def gpu_decrypt(k, dct, n):
    out = DevArray(shape=(n, k.nk.nw))
    _native.check(k.nk.lib.pai_decrypt(k.nk.sk, getattr(dct, "ptr", dct), n, out.ptr, None))
    return limbs_to_ints(out.get())


def test_encrypt_and_obfuscate(xk, monkeypatch):
    """pai_raw_encrypt, pai_encrypt (DJN) and pai_obfuscate on the throughput engine of the key size (base-n digit engine, lane-group
    digit pairs, or lane groups), the small-batch chains (wave-shared on the minus-one context, wave-shared, one chain per integer)
    and, where n fits the 4-lane geometries, the mid-size digit-pair kernel: orc.encrypt / apply_obfuscator.  The first call builds
    the fixed-base (g-factored where the key takes them), digit-engine and pair tables."""
    k, nk, key, N = xk, xk.nk, xk.key, xk.N
    m, r = plain(k, N, 1), rand_r(k, N, 2)
    want = djn_encrypt_many(key, m, r)
    assert want[:4] == [orc.encrypt(key, x, rr) for x, rr in zip(m[:4], r[:4])]
    want2 = djn_obfuscate_many(key, want, r)
    assert want2[3] == orc.apply_obfuscator(key, want[3], r[3])
    raw = [orc.raw_encrypt(x, key.n) for x in m]
    dm, dr = DevArray(ints_to_limbs(m, nk.nw)), DevArray(ints_to_limbs(r, nk.rw))
    ct = DevArray(shape=(N, nk.cw))
    thr = "padic" if 2 * xk.b <= 1024 or 1400 <= 2 * xk.b <= 2068 else ("pair" if 2 * xk.b > 2048 else "lane_group")
    mid = 2 * xk.b in (1024, 2048)
    cfgs = [("0", None, None, False, {thr}), ("100000", "100000", False, False, {"lat_tree_m1", "lat_tree"}),
            ("100000", "100000", True, False, {"lat_tree"}), ("100000", "0", False, False, {"lat_chain"})]
    if mid:
        cfgs.append(("100000", None, None, True, {"pair4"}))
    for switch, tree, no_m1, use_mid, allowed in cfgs:
        monkeypatch.setenv("PAI_LATENCY_MAX", switch)
        tune(monkeypatch, "lat_enc_tree", tree)
        knob_disable(monkeypatch, "lat_enc_m1", bool(no_m1))
        tune(monkeypatch, "enc_mid_min", 0 if use_mid else None)
        tune(monkeypatch, "enc_mid_max", 1 << 30 if use_mid else None)
        _native.check(nk.lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, N, ct.ptr, None))
        got = ran(k, "encrypt")
        assert limbs_to_ints(ct.get()) == want, (xk.ident, switch, tree, no_m1, use_mid, got)
        assert len(got) == 1 and got[0].split(":")[1] in allowed, (xk.ident, switch, tree, no_m1, use_mid, got)
        _native.check(nk.lib.pai_obfuscate(nk.pk, ct.ptr, dr.ptr, N, None))
        got = ran(k, "encrypt")
        assert limbs_to_ints(ct.get()) == want2, (xk.ident, switch, tree, no_m1, use_mid, got)
        assert len(got) == 1 and got[0].split(":")[1] in allowed, (xk.ident, got)
    for lat_add, allowed in (("0", {"padic" if thr == "padic" else "lane_group"}), ("4096", {"lat"})):
        monkeypatch.setenv("PAI_LAT_ADD_MAX", lat_add)
        _native.check(nk.lib.pai_raw_encrypt(nk.pk, dm.ptr, N, ct.ptr, None))
        got = ran(k, "encrypt")
        assert limbs_to_ints(ct.get()) == raw, (xk.ident, lat_add, got)
        assert got[0].split(":")[1] in allowed, (xk.ident, lat_add, got)


def test_decrypt(xk, monkeypatch):
    """pai_decrypt -> orc.decrypt_crt on the digit-pair engine of the prime width (256-element tiles: a batch of 257; at 36 limbs
    all three MODES of test_gpu_padic_kara_mul.py), the four-wave, wave-pair and window kernels of small batches, and the 4-lane
    digit-pair stage A of mid-size batches."""
    k, nk = xk, xk.nk
    cts = ciphertexts(k, 257, 3, units=True)
    want = decrypt_many(k, cts)
    assert want[:3] == [orc.decrypt_crt(k.key, c) for c in cts[:3]]
    dct = DevArray(ints_to_limbs(cts, nk.cw))
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")
    tune(monkeypatch, "dec_mid_max", 0)
    kara = 676 < xk.b <= 1024
    for mode in (MODES if kara else ["padic"]):
        for name in ("padic_kara_mul", "padic_kara"):
            knob_disable(monkeypatch, name, kara and name in MODES[mode])
        got = gpu_decrypt(k, dct, 257)
        path = ran(k, "decrypt")
        assert got == want, (xk.ident, mode, path)
        assert path[0] == "k_dec_a:" + ({"kara_mul": "padic_kara_mul", "kara_sqr": "padic_kara", "rowwise": "padic_rowwise"}[mode] if kara else "padic"), path
    tune(monkeypatch, "dec_mid_max", None)
    N = k.N
    row = 4 * nk.cw
    monkeypatch.setenv("PAI_LATENCY_MAX", "100000")
    for pp, rl, allowed in (("100000", "100000", {"pp", "rl", "window"}), ("0", "100000", {"rl"}), ("0", "0", {"window"})):
        tune(monkeypatch, "lat_pp", pp)
        tune(monkeypatch, "lat_rl", rl)
        for off in k.offs:                                   # the 6 unit corners, the 49 grid cells and 15 / 19 pattern units
            got = gpu_decrypt(k, C.c_void_p(dct.ptr.value + off * row), N)
            path = ran(k, "decrypt")
            assert got == want[off:off + N], (xk.ident, pp, rl, off, path)
            assert path[0].split(":")[1] in allowed, (xk.ident, pp, rl, path)
    tune(monkeypatch, "dec_mid_min", 0)
    tune(monkeypatch, "dec_mid_max", 1 << 30)
    for off in k.offs:
        got = gpu_decrypt(k, C.c_void_p(dct.ptr.value + off * row), N)
        path = ran(k, "decrypt")
        assert got == want[off:off + N], (xk.ident, "mid", off, path)
        assert path[0] == "k_dec_a:pair4", (xk.ident, path)


def test_ct_mul(xk, monkeypatch):
    """pai_ct_mul -> pow(c, e, n^2): exponents 0, 1, 2^ebits - 1, 2^(ebits - 1) in front of every batch per element, and each of
    the four as the broadcast exponent, on the throughput engine (digit engine / lane-group digit pairs / windowed lane groups with pair_ctmul off), the small-batch kernels
    and the mid-size 4-lane kernel."""
    k, nk, key, N, T = xk, xk.nk, xk.key, xk.N, xk.T
    M = key.nsq
    c = ciphertexts(k, T, 5)
    dc = DevArray(ints_to_limbs(c, nk.cw))
    row = 4 * nk.cw
    nb = 2 * xk.b
    thr = "padic" if nb <= 1024 or 1400 <= nb <= 2068 else ("pair" if nb > 2048 else "lane_group")
    for ebits in (12, 53, 130):
        rng = random.Random(ebits)
        ecorn = [0, 1, (1 << ebits) - 1, 1 << (ebits - 1)]
        e = [rng.getrandbits(ebits) for _ in range(T)]
        for off in k.offs:
            e[off:off + 4] = ecorn
        ew = (ebits + 31) // 32
        de = DevArray(ints_to_limbs(e, ew))
        want = pow_many(c, e, M)
        want_b = [[1] * T, list(c), pow_many(c, ecorn[2], M), pow_many(c, ecorn[3], M)]
        cfgs = [("0", None, None, False, False, {thr})]
        if nb > 2048:
            cfgs.append(("0", None, None, True, False, {"lane_group"}))
        cfgs += [("100000", "100000", "100000", False, False, {"pp", "rl", "window"}), ("100000", "0", "100000", False, False, {"rl", "window"}),
                 ("100000", "0", "0", False, False, {"window"})]
        if nb <= 2068:
            cfgs.append(("100000", None, None, False, True, {"pair4"}))
        for switch, pp, rl, no_pair, mid, allowed in cfgs:
            monkeypatch.setenv("PAI_LATENCY_MAX", switch)
            tune(monkeypatch, "lat_mul_pp", pp)
            tune(monkeypatch, "lat_mul_rl", rl)
            knob_disable(monkeypatch, "pair_ctmul", no_pair)
            tune(monkeypatch, "ctmul_mid_min", 0 if mid else None)
            tune(monkeypatch, "ctmul_mid_max", 1 << 30 if mid else None)
            out = DevArray(shape=(N, nk.cw))
            for off in k.offs:
                dco = C.c_void_p(dc.ptr.value + off * row)
                _native.check(nk.lib.pai_ct_mul(nk.pk, dco, C.c_void_p(de.ptr.value + 4 * ew * off), ew, ebits, 0, N, out.ptr, None))
                path = ran(k, "ct_mul")
                assert limbs_to_ints(out.get()) == want[off:off + N], (xk.ident, ebits, switch, pp, rl, no_pair, mid, off, path)
                assert len(path) == 1 and path[0].split(":")[1] in allowed, (xk.ident, ebits, switch, pp, rl, no_pair, mid, path)
                for j in range(4):                               # broadcast: 0 (result 1), 1 (result c), all ones, the single top bit
                    _native.check(nk.lib.pai_ct_mul(nk.pk, dco, C.c_void_p(de.ptr.value + 4 * ew * j), ew, ebits, 1, N, out.ptr, None))
                    path = ran(k, "ct_mul")
                    assert limbs_to_ints(out.get()) == want_b[j][off:off + N], (xk.ident, ebits, switch, pp, rl, no_pair, mid, off, "bcast", j, path)
                    assert path[0].split(":")[1] in allowed, (xk.ident, path)


def test_ct_add_family(xk, monkeypatch):
    """pai_ct_add on the most-significant-limb-first product (where the key has the context: reported, not required) and on the
    Montgomery products, each on one integer per wavefront and on wave tiles; pai_ct_mont_mul, pai_ct_add_aligned and pai_ct_pow2
    with shifts in -3 .. 8 on both geometries: products and powers modulo n^2."""
    k, nk, key, N, T = xk, xk.nk, xk.key, xk.N, xk.T
    M, W = key.nsq, nk.cw
    a, b = ciphertexts(k, T, 7), list(reversed(ciphertexts(k, T, 8)))
    assert (a[1], a[3], a[6]) == (1, key.n - 1, M - 1)
    b[1], b[3], b[6] = M - 1, key.n + 1, M - 1              # products M - 1, M - 1 (the longest borrow of the final subtraction) and 1
    da, db = DevArray(ints_to_limbs(a, W)), DevArray(ints_to_limbs(b, W))
    row = 4 * W
    out = DevArray(shape=(N, W))
    rb = C.c_int(0)
    _native.check(nk.lib.pai_pubkey_mont_bits(nk.pk, C.byref(rb)))
    Ri = pow(pow(2, rb.value, M), -1, M)
    rng = np.random.default_rng(xk.b)
    delta = rng.integers(-3, 9, T).astype(np.int32)
    for off in k.offs:
        delta[off:off + 6] = [0, 1, -3, 8, -1, 7]
    dd = DevArray(delta)
    prod = [x * y % M for x, y in zip(a, b)]
    want_al = [x * pow(y, 1 << int(d), M) % M if d > 0 else pow(x, 1 << int(-d), M) * y % M for x, y, d in zip(a, b, delta)]
    want_p2 = [pow(x, 1 << int(d), M) if d > 0 else x for x, d in zip(a, delta)]
    has_msb = None
    for lat_add, geo in (("0", "lane_group"), ("4096", "lat")):
        monkeypatch.setenv("PAI_LAT_ADD_MAX", lat_add)
        for off in k.offs:
            pa, pb, pd = C.c_void_p(da.ptr.value + off * row), C.c_void_p(db.ptr.value + off * row), C.c_void_p(dd.ptr.value + 4 * off)
            sl = slice(off, off + N)
            for no_msb in (False, True):
                knob_disable(monkeypatch, "add_msb", no_msb)
                _native.check(nk.lib.pai_ct_add(nk.pk, pa, pb, 0, N, out.ptr, None))
                path = ran(k, "ct_add")
                if lat_add == "0" and not no_msb:
                    has_msb = path == ["k_modmul_msb:lane_group"]
                assert limbs_to_ints(out.get()) == prod[sl], (xk.ident, lat_add, no_msb, off, path, "msb context:", has_msb)
                if geo == "lat":
                    assert path[0] in ("k_modmul:lat", "k_modmul:lat_m1"), (xk.ident, path)
                else:
                    assert path == (["k_modmul:lane_group"] if no_msb or not has_msb else ["k_modmul_msb:lane_group"]), (xk.ident, path, has_msb)
                _native.check(nk.lib.pai_ct_add(nk.pk, pa, pb, 1, N, out.ptr, None))
                assert limbs_to_ints(out.get()) == [x * b[off] % M for x in a[sl]], (xk.ident, lat_add, no_msb, off, "bcast")
            knob_disable(monkeypatch, "add_msb", False)
            _native.check(nk.lib.pai_ct_mont_mul(nk.pk, pa, pb, 0, N, out.ptr, None))
            path = ran(k, "ct_add")
            assert limbs_to_ints(out.get()) == [x * Ri % M for x in prod[sl]], (xk.ident, lat_add, off, path)
            assert path == [f"k_modmul:{geo}"], (xk.ident, path)
            _native.check(nk.lib.pai_ct_add_aligned(nk.pk, pa, pb, 0, pd, N, out.ptr, None))
            path = ran(k, "ct_add")
            assert limbs_to_ints(out.get()) == want_al[sl], (xk.ident, lat_add, off, path)
            assert path[0].split(":")[1].startswith(geo), (xk.ident, path)
            dc = DevArray(ints_to_limbs(a[sl], W))
            _native.check(nk.lib.pai_ct_pow2(nk.pk, dc.ptr, pd, 0, N, None))
            path = ran(k, "ct_add")
            assert limbs_to_ints(dc.get()) == want_p2[sl], (xk.ident, lat_add, off, path)
            assert path == [f"k_pow2:{geo}"], (xk.ident, path)
    SEEN.setdefault(("msb_context", xk.b), set()).add(f"{xk.family}={has_msb}")


def test_invert_prod_multiexp(xk):
    """pai_ct_invert on units -> pow(x, -1, n^2); pai_ct_prod with 70 members in 1 and 7 groups -> plain products;
    pai_ct_multiexp on R=2, K=5, M=3 with 53-bit exponents and mixed signs -> product of powers."""
    k, nk, key = xk, xk.nk, xk.key
    M, W = key.nsq, nk.cw
    u = ciphertexts(k, 70, 9, units=True)
    du = DevArray(ints_to_limbs(u, W))
    out = DevArray(shape=(70, W))
    _native.check(nk.lib.pai_ct_invert(nk.pk, du.ptr, 70, out.ptr, None))
    assert limbs_to_ints(out.get()) == [pow(x, -1, M) for x in u], xk.ident
    a = ciphertexts(k, 70, 10, units=True)
    a[3] = key.n                                            # one multiple of n: its group's product stays one, not zero
    da = DevArray(ints_to_limbs(a, W))
    for groups in (1, 7):
        og = DevArray(shape=(groups, W))
        _native.check(nk.lib.pai_ct_prod(nk.pk, da.ptr, 70, groups, og.ptr, None))
        want = []
        for g in range(groups):
            acc = 1
            for l in range(70 // groups):
                acc = acc * a[l * groups + g] % M
            want.append(acc)
        assert limbs_to_ints(og.get()) == want, (xk.ident, groups)
    R, K, Mc, ew = 2, 5, 3, 2
    base = u[3:3 + R * K]
    inv = [pow(x, -1, M) for x in base]
    rng = random.Random(xk.b)
    e = [[[rng.getrandbits(53) for _ in range(Mc)] for _ in range(K)] for _ in range(R)]
    e[0][0][0], e[0][1][0], e[1][0][1], e[1][1][1] = 0, 1, (1 << 53) - 1, 1 << 52
    sign = np.array([[(l + j) % 2 for j in range(Mc)] for l in range(K)], dtype=np.uint8)
    e_l = np.zeros((R, K, Mc, ew), dtype=np.uint32)
    for r in range(R):
        for l in range(K):
            for j in range(Mc):
                e_l[r, l, j] = [e[r][l][j] & 0xFFFFFFFF, e[r][l][j] >> 32]
    want = []
    for r in range(R):
        for j in range(Mc):
            acc = 1
            for l in range(K):
                acc = acc * pow(inv[r * K + l] if sign[l, j] else base[r * K + l], e[r][l][j], M) % M
            want.append(acc)
    dc, di, de, dsg = DevArray(ints_to_limbs(base, W)), DevArray(ints_to_limbs(inv, W)), DevArray(e_l), DevArray(sign)
    om = DevArray(shape=(R * Mc, W))
    _native.check(nk.lib.pai_ct_multiexp(nk.pk, dc.ptr, di.ptr, R, K, Mc, de.ptr, ew, 53, dsg.ptr, om.ptr, None))
    assert limbs_to_ints(om.get()) == want, xk.ident


def test_fallback_engines(xk, monkeypatch):
    """Handles created with the digit engines left out (PAI_DISABLE=padic,pair, then wide as well): DJN encryption, ct * pt and
    decryption of the same key on the wide / lane-group kernels that serve every size."""
    k, key, N = xk, xk.key, xk.N
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")
    m, r = plain(k, N, 11), rand_r(k, N, 12)
    want = djn_encrypt_many(key, m, r)
    e = [0, 1, (1 << 53) - 1, 1 << 52] + [random.Random(5).getrandbits(53) for _ in range(N - 4)]
    want_mul = pow_many(want, e, key.nsq)
    for off in ("padic,pair", "padic,pair,wide"):
        monkeypatch.setenv("PAI_DISABLE", off)
        nk = NativeKey(key)
        dm, dr, de = DevArray(ints_to_limbs(m, nk.nw)), DevArray(ints_to_limbs(r, nk.rw)), DevArray(ints_to_limbs(e, 2))
        ct, out, pr = DevArray(shape=(N, nk.cw)), DevArray(shape=(N, nk.nw)), DevArray(shape=(N, nk.cw))
        _native.check(nk.lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, N, ct.ptr, None))
        path = ran(k, "encrypt")
        assert limbs_to_ints(ct.get()) == want, (xk.ident, off, path)
        assert path == ["k_encrypt(djn):lane_group"], (xk.ident, off, path)
        _native.check(nk.lib.pai_ct_mul(nk.pk, ct.ptr, de.ptr, 2, 53, 0, N, pr.ptr, None))
        path = ran(k, "ct_mul")
        assert limbs_to_ints(pr.get()) == want_mul, (xk.ident, off, path)
        assert path == ["k_ctmul:lane_group"], (xk.ident, off, path)
        _native.check(nk.lib.pai_decrypt(nk.sk, ct.ptr, N, out.ptr, None))
        path = ran(k, "decrypt")
        assert limbs_to_ints(out.get()) == m, (xk.ident, off, path)
        assert path[0] in (["k_dec_a:wide", "k_dec_a:lane_group"] if off == "padic,pair" else ["k_dec_a:lane_group"]), (xk.ident, off, path)
        del nk


def test_standard_scheme_2048_ones(monkeypatch):
    """One pass of the standard scheme (obfuscator r^n) at the 2048-bit `ones` key."""
    _, _, b, p, q = next(e for e in ENTRIES if e[0] == "ones-1024")
    key = orc.make_key(p, q, djn_x=None, bits=2 * b)
    nk = NativeKey(key)
    N = 70
    m = ([0, 1, key.n - 1, key.p, key.q, key.n - key.p, key.n - key.q] + pattern(key.n, N, 21))[:N]
    r = [x or 1 for x in ([1, key.n - 1, 2] + pattern(key.n, N, 22))[:N]]
    obf = pow_many(r, key.n, key.nsq)
    want = [(1 + x * key.n) % key.nsq * o % key.nsq for x, o in zip(m, obf)]
    assert want[1] == orc.encrypt(key, m[1], r[1])
    dm, dr = DevArray(ints_to_limbs(m, nk.nw)), DevArray(ints_to_limbs(r, nk.nw))
    ct = DevArray(shape=(N, nk.cw))
    _native.check(nk.lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, N, ct.ptr, None))
    assert limbs_to_ints(ct.get()) == want
    out = DevArray(shape=(N, nk.nw))
    _native.check(nk.lib.pai_decrypt(nk.sk, ct.ptr, N, out.ptr, None))
    assert limbs_to_ints(out.get()) == m


def test_every_kernel_family_ran_on_some_key():
    """What ran, per operation and prime width (printed: the record of the coverage), and every family on at least one key — a knob
    that fell through everywhere fails here.  Holds when the whole file ran; a selection of keys only prints."""
    for (op, b), names in sorted(SEEN.items()):
        print(f"COVERAGE {op} prime_bits={b}: {' '.join(sorted(names))}")
    if VISITED != {e[0] for e in ENTRIES}:
        print(f"COVERAGE not asserted: {len(VISITED)} of {len(ENTRIES)} keys ran")
        return
    allseen = {op: set().union(*(v for (o, _), v in SEEN.items() if o == op)) for op in ("encrypt", "decrypt", "ct_mul", "ct_add")}
    assert {f"k_dec_a:{x}" for x in ("pp", "rl", "window", "pair4", "padic", "padic_kara_mul", "padic_kara", "padic_rowwise", "wide", "lane_group")} <= allseen["decrypt"]
    assert {f"k_ctmul:{x}" for x in ("pp", "rl", "window", "pair4", "padic", "pair", "lane_group")} <= allseen["ct_mul"]
    assert {f"k_encrypt(djn):{x}" for x in ("padic", "pair", "lane_group", "pair4", "lat_tree_m1", "lat_tree", "lat_chain")} <= allseen["encrypt"]
    assert {"k_modmul_msb:lane_group", "k_modmul:lane_group", "k_modmul:lat", "k_add_aligned:lane_group", "k_pow2:lane_group", "k_pow2:lat"} <= allseen["ct_add"]
