"""CPU: the host side of ciphertext openings (pai_recover_r / PaillierPublicKey.verify_opening).

* pai_host_modinv (csrc/hostbn.hpp: inv_mod, extended Euclid on any modulus >= 2) against CPython's pow(a, -1, m).
* The expectation the GPU tests of tests/test_gpu_recover.py compare against — r from pow on the half-width primes plus Garner, and
  the full-width pow(c mod n, n^-1 mod lcm(p - 1, q - 1), n) — held to the definition of an opening, c = (1 + m n) r^n mod n^2, on
  the 1024-bit fixture key.
* Every structured and limit key of tests/golden has gcd(n, (p - 1)(q - 1)) = 1, so the GPU file may require all of them served."""
import json
import math
import random
from pathlib import Path

import pytest

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_limit_keys_cpu import load_limit_keys

ROOT = Path(__file__).resolve().parent.parent
DJN_X = 0xABCDEF1234567


# ---- the expectation (CPython ints only) ------------------------------------------------------------------------------------
def expect_r(p, q, c):
    """r of the opening of c by the route of the kernels: r_s = (c mod s)^(n^-1 mod (s - 1)) mod s, Garner-lifted modulo n."""
    p, q = (p, q) if p < q else (q, p)
    n = p * q
    rp = pow(c % p, pow(n % (p - 1), -1, p - 1), p)
    rq = pow(c % q, pow(n % (q - 1), -1, q - 1), q)
    return rp + p * ((rq - rp) * pow(p, -1, q) % q)


def expect_r_full(p, q, c):
    """The same r by one full-width power (units only)."""
    n = p * q
    lam = (p - 1) * (q - 1) // math.gcd(p - 1, q - 1)
    return pow(c % n, pow(n, -1, lam), n)


def expect_open(key, c):
    """(m, r) with c = (1 + m n) r^n mod n^2"""
    return orc.decrypt_crt(key, c), expect_r(key.p, key.q, c)


def reencrypt(n, m, r):
    return (1 + m * n) * pow(r, n, n * n) % (n * n)


def all_keys():
    """(id, p, q) of the 15 limit keys, then the 27 structured keys"""
    return [(e[0], e[5], e[6]) for e in load_limit_keys()] + [(e[0], e[3], e[4]) for e in load_extreme_keys()]


# ---- pai_host_modinv ----------------------------------------------------------------------------------------------------------
def _moduli():
    rng = random.Random(20)
    out = []
    for bits in (64, 65, 96, 512, 1023, 1024, 2048, 2100):
        m = rng.getrandbits(bits) | (1 << (bits - 1))
        out += [m | 1, m & ~1, (m & ~((1 << (bits // 2)) - 1))]          # odd, even, divisible by a large power of two
    return out


@pytest.mark.parametrize("m", _moduli(), ids=lambda m: f"{m.bit_length()}b-{'odd' if m & 1 else 'even' + str((m & -m).bit_length() - 1)}")
def test_host_modinv_against_pow(m):
    rng = random.Random(m & 0xFFFF)
    cands = [1, m - 1, m + 1, 3 * m - 1, rng.getrandbits(m.bit_length() + 70)]
    cands += [rng.randrange(1, m) for _ in range(6)]
    seen_unit = seen_non_unit = 0
    for a in cands:
        if math.gcd(a, m) == 1:
            got = _native.host_modinv(a, m)
            assert got == pow(a, -1, m), (a, m)
            assert 0 <= got < m and a * got % m == 1
            seen_unit += 1
        else:
            with pytest.raises(_native.NativeError) as ei:
                _native.host_modinv(a, m)
            assert ei.value.code == _native.PAI_E_INVALID
            seen_non_unit += 1
    assert seen_unit >= 3                                                # a = 1, m - 1, m + 1 are units of every m
    # a common factor on purpose: gcd(a, m) = g > 1
    g = 2 if m % 2 == 0 else next(d for d in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, m) if m % d == 0)
    for a in (g, g * rng.randrange(1, m), m, 0):
        with pytest.raises(_native.NativeError) as ei:
            _native.host_modinv(a, m)
        assert ei.value.code == _native.PAI_E_INVALID


def test_host_modinv_small_moduli():
    for m in (0, 1):
        for a in (0, 1, 5):
            with pytest.raises(_native.NativeError) as ei:
                _native.host_modinv(a, m)
            assert ei.value.code == _native.PAI_E_INVALID
    assert _native.host_modinv(1, 2) == 1 and _native.host_modinv(7, 2) == 1
    assert _native.host_modinv(3, 4) == 3 and _native.host_modinv(5, 6) == 5
    for m in range(2, 200):
        for a in range(0, 2 * m):
            if math.gcd(a, m) == 1:
                assert _native.host_modinv(a, m) == pow(a, -1, m)


def test_host_modinv_recovery_exponents_of_every_key():
    """the inverses pai_recover_r takes on its first call: (other prime)^-1 mod (s - 1), s - 1 even"""
    for ident, p, q in all_keys():
        for s, o in ((p, q), (q, p)):
            d = _native.host_modinv(o % (s - 1), s - 1)
            assert d == pow(p * q, -1, s - 1), ident


# ---- the expectation helper ---------------------------------------------------------------------------------------------------
def test_expectation_is_the_opening_on_the_fixture_key():
    fx = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())["1024"]
    p, q = int(fx["p"], 16), int(fx["q"], 16)
    key = orc.make_key(p, q, djn_x=DJN_X, bits=1024)
    n, nsq = key.n, key.nsq
    rng = random.Random(1024)
    h = expect_r(p, q, key.hs)                                           # hs = h^n mod n^2 (h = -x^2 mod n): hs^r' = (h^r')^n
    assert reencrypt(n, 0, h) == key.hs and h == (-DJN_X * DJN_X) % n
    m1, m2 = rng.randrange(n), rng.randrange(n)
    r1 = rng.getrandbits(key.randbits)
    djn = orc.encrypt(key, m1, r1)
    r_std = rng.randrange(1, n)
    std = (1 + m2 * n) * pow(r_std, n, nsq) % nsq
    unit = rng.randrange(1, nsq)
    assert math.gcd(unit, n) == 1
    for c in (djn, std, djn * std % nsq, unit, 1, nsq - 1, 1 + n, pow(2, n, nsq)):
        m, r = expect_open(key, c)
        assert 0 <= m < n and 0 < r < n
        assert reencrypt(n, m, r) == c
        assert r == expect_r_full(p, q, c)
    assert expect_open(key, djn) == (m1, pow(h, r1, n))
    assert expect_open(key, std) == (m2, r_std)
    assert expect_open(key, djn * std % nsq) == ((m1 + m2) % n, pow(h, r1, n) * r_std % n)
    assert expect_r(p, q, nsq - 1) == n - 1 and expect_r(p, q, pow(2, n, nsq)) == 2
    # a non-unit: the arithmetic gives r = 0 modulo the prime that divides the row
    c = key.p * rng.randrange(1, nsq // key.p)
    assert expect_r(p, q, c) % key.p == 0


def test_every_structured_and_limit_key_has_unique_openings():
    keys = all_keys()
    assert len(keys) == 42
    for ident, p, q in keys:
        assert math.gcd(p * q, (p - 1) * (q - 1)) == 1, ident
