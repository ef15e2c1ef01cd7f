"""GPU: CRT decryption on the 36-limb digit-pair kernel with the quotient products of its Montgomery reductions by
Karatsuba columns (csrc/mont_padic.hpp: kara_pass<FORM, true>, kernel mode PADIC_LDS_KMR, the default), against the
same kernel with schoolbook quotient products (PAI_DISABLE=padic_kara_red: mode PADIC_LDS_KM), against the row-wise
products (PAI_DISABLE=padic_kara_mul) and against the Python-int oracle, through pai_decrypt.

Keys: the 2048-bit bench key, a 1536-bit key (768-bit primes still sit on 36 limbs) and the structured 2048-bit keys of
tests/golden/extreme_keys.json (primes of all-ones limbs, all-zero limbs, halves at opposite extremes, n0inv = 1 / 2^29 - 1:
the modulus differences p[18 + l] - p[l] of the new columns at both extremes and at zero).
Ciphertexts: real encryptions, 0, 1, n^2 - 1, and values = 0 and = -1 modulo p^2 resp. q^2.
Batches: 1, 255 / 256 / 257 (one 256-element tile and its edges) and one batch of more tiles than workgroups.
All three modes must give the same words for every ciphertext; where the oracle defines a decryption (c a unit modulo n:
L((c^(s-1) mod s^2) needs c^(s-1) == 1 mod s, orc._lfun asserts it) the words are the oracle's.  For 0 and the multiples of
p^2 / q^2 the oracle has no value, there the three modes are held to each other."""
import ctypes as C
import math
import random

import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from tests._util import DevArray, disable, djn_encrypt_many, ints_to_limbs, limbs_to_ints, pow_many, tune
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels, bench_key

pytestmark = pytest.mark.gpu

MODES = {"kara_red": (), "kara_mul": ("padic_kara_red",), "kara_sqr": ("padic_kara_mul",)}
POOL = 257


def crt(a, b, p2, q2):
    return (a + p2 * ((b - a) * pow(p2, -1, q2) % q2)) % (p2 * q2)


def key_1536():
    p = orc.seeded_prime(768, 7000 + 1536)
    q = orc.seeded_prime(768, 9000 + 1536)
    while q == p or (p * q).bit_length() != 1536:
        q = orc.seeded_prime(768, q % 100003)
    return orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=1536)


KEYS = {"bench-2048": bench_key, "seeded-1536": key_1536}
for _ident, _family, _b, _p, _q in load_extreme_keys():
    if _b == 1024:
        KEYS[_ident] = (lambda p=_p, q=_q: orc.make_key(p, q, djn_x=(1 << 70) + 12345, bits=2048))


def ciphertext_pool(key, n, seed):
    """The special residues first (position 0 is a real encryption, so that the batch of one is one), then real encryptions
    and random residues."""
    rng = random.Random(seed)
    p2, q2, M = key.p * key.p, key.q * key.q, key.nsq
    ra, rb = rng.randrange(1, p2), rng.randrange(1, q2)
    special = [0, 1, M - 1,
               crt(0, rb, p2, q2), crt(ra, 0, p2, q2), crt(0, 1, p2, q2), crt(1, 0, p2, q2),    # = 0 modulo p^2 resp. q^2
               crt(p2 - 1, rb, p2, q2), crt(ra, q2 - 1, p2, q2), crt(p2 - 1, 1, p2, q2), crt(1, q2 - 1, p2, q2),    # = -1
               crt(0, q2 - 1, p2, q2), crt(p2 - 1, 0, p2, q2)]
    n_enc = max(1, (n - len(special)) // 2)
    ms = [0, 1, key.n - 1] + [rng.randrange(key.n) for _ in range(n_enc)]
    rs = [rng.getrandbits(key.randbits) for _ in ms]
    enc = djn_encrypt_many(key, ms[:n_enc], rs[:n_enc])
    assert enc[0] == orc.encrypt(key, ms[0], rs[0])
    out = enc[:1] + special + enc[1:]
    while len(out) < n:
        out.append(rng.randrange(1, M))
    return out[:n]


def oracle_decrypt(key, cts):
    """[orc.decrypt_crt(key, c)] where it is defined (c a unit), None elsewhere; the half-size powers through pow_many."""
    kc = orc.crt_constants(key)
    p, q = key.p, key.q
    idx = [i for i, c in enumerate(cts) if math.gcd(c, key.n) == 1]
    up = pow_many([cts[i] % (p * p) for i in idx], p - 1, p * p)
    uq = pow_many([cts[i] % (q * q) for i in idx], q - 1, q * q)
    out = [None] * len(cts)
    for i, a, b in zip(idx, up, uq):
        mp = orc._lfun(a, p) * kc["hp"] % p
        mq = orc._lfun(b, q) * kc["hq"] % q
        out[i] = mp + p * ((mq - mp) * kc["pinv_q"] % q)
    for i in idx[:2]:
        assert out[i] == orc.decrypt_crt(key, cts[i])
    return out


class Case:
    def __init__(self, ident):
        self.key = KEYS[ident]()
        self.nk = NativeKey(self.key)
        self.cts = ciphertext_pool(self.key, POOL, seed=len(ident))
        self.want = oracle_decrypt(self.key, self.cts)
        assert sum(w is None for w in self.want) >= 7 and self.want[0] is not None
        self.dct = DevArray(ints_to_limbs(self.cts, self.nk.cw))


_CASES = {}


@pytest.fixture(params=list(KEYS))
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = Case(request.param)
    return _CASES[request.param]


def decrypt_modes(nk, dct, n, monkeypatch):
    """{mode: plaintext integers} of the first n ciphertexts at dct, every batch on k_dec_a_padic"""
    monkeypatch.setenv("PAI_LATENCY_MAX", "0")            # no small-batch kernels
    tune(monkeypatch, "dec_mid_max", 0)                   # no lane-group stage A
    _native.check(nk.lib.pai_profile_enable(1))
    got = {}
    try:
        for mode, off in MODES.items():
            for name in ("padic_kara_red", "padic_kara_mul", "padic_kara"):
                disable(monkeypatch, name, name in off)
            out = DevArray(shape=(n, nk.nw))
            _native.check(nk.lib.pai_decrypt(nk.sk, dct.ptr, n, out.ptr, None))
            buf = C.create_string_buffer(64)
            assert _last_kernels(nk.lib)[0] == "k_dec_a"
            _native.check(nk.lib.pai_profile_last_path(0, buf, 64))
            assert buf.value.decode() == ("padic_kara" if mode == "kara_sqr" else "padic_kara_mul")
            got[mode] = limbs_to_ints(out.get())
    finally:
        _native.check(nk.lib.pai_profile_enable(0))
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_padic_kred_decrypt(case, monkeypatch, n):
    got = decrypt_modes(case.nk, case.dct, n, monkeypatch)
    assert got["kara_red"] == got["kara_mul"]
    assert got["kara_red"] == got["kara_sqr"]
    for i in range(n):
        if case.want[i] is not None:
            assert got["kara_red"][i] == case.want[i], i


def test_padic_kred_more_tiles_than_workgroups(monkeypatch):
    """More 256-element tiles than the launch has workgroups per prime (at most 128 on a 256-CU device: 257 tiles and a
    tail), so that every workgroup walks its tile loop more than once.  The three modes agree on the whole batch; the
    oracle holds the special residues at the front and samples from every pass of the loop and the tail."""
    key = bench_key()
    nk = NativeKey(key)
    n = 2 * 128 * 256 + 77
    rng = random.Random(9)
    cts = ciphertext_pool(key, 64, seed=9) + [rng.randrange(1, key.nsq) for _ in range(n - 64)]
    dct = DevArray(ints_to_limbs(cts, nk.cw))
    got = decrypt_modes(nk, dct, n, monkeypatch)
    assert got["kara_red"] == got["kara_mul"]
    assert got["kara_red"] == got["kara_sqr"]
    sample = list(range(64)) + [255, 256, 32767, 32768, 40000, 65535, 65536, n - 77, n - 2, n - 1]
    want = oracle_decrypt(key, [cts[i] for i in sample])
    for i, w in zip(sample, want):
        if w is not None:
            assert got["kara_red"][i] == w, i
