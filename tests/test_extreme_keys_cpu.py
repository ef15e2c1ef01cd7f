"""CPU: the structured prime pairs of tests/golden/extreme_keys.json (tests/golden/make_extreme_keys.py) are what their family
names claim — primes, of the stated widths, with limbs of 2^29 - 1 / 0 at the stated positions and the stated residues modulo
2^58 — and are sound Paillier keys under the oracle.  The kernels meet them in tests/test_gpu_extreme_keys.py; the cell-bound
models meet their moduli in tests/test_host_logic_cpu.py (most-significant-limb-first product) and tests/test_padic_kara*_cpu.py.

Cost: about 50 s in CPython, not a few seconds — the oracle's 24-round Miller-Rabin over the 38 distinct primes takes 8 s, and a
round trip at the 2048-bit primes 2.5 s (key.hs, four decrypt_crt and one decrypt_lambda on 8192-bit moduli; the CRT constants
are derived once per key); the oracle has no cheaper form of either, and the checks are the ones the fixture needs."""
import json
import math
from pathlib import Path

import pytest

from oracle import paillier_oracle as orc

RB = 29
MASK = (1 << RB) - 1
NL = {512: 24, 676: 24, 1024: 36, 1536: 56, 1604: 56, 2048: 72, 2068: 72}     # digit-pair limbs serving a prime width
FAMILIES = ("ones", "zeros", "ones_zeros", "half", "n0", "n0_one")


def load_extreme_keys():
    """[(id, family, prime_bits, p, q)] in the fixture's order (by prime width, then family)."""
    fx = json.loads((Path(__file__).parent / "golden" / "extreme_keys.json").read_text())
    return [(f"{e['family']}-{e['prime_bits']}", e["family"], e["prime_bits"], int(e["p"], 16), int(e["q"], 16)) for e in fx]


ENTRIES = load_extreme_keys()


def n0inv(m):
    return (-pow(m, -1, 1 << RB)) % (1 << RB)


def is_ones(x, b):
    """every 29-bit and every 32-bit limb above the lowest is all ones"""
    return x.bit_length() == b and all((x >> w) == (1 << (b - w)) - 1 for w in (29, 32))


def is_zeros(x, b):
    """the top two bits, then zeros down to the lowest limb"""
    return x.bit_length() == b and 0 < x - (3 << (b - 2)) < 1 << 29


def test_fixture_covers_every_family_and_width():
    got = {(f, b) for _, f, b, _, _ in ENTRIES}
    assert got == {(f, b) for f in FAMILIES for b in (512, 1024, 1536, 2048)} | {("ones", b) for b in (676, 1604, 2068)}
    assert len(ENTRIES) == len(got)
    # the three limit widths are the widest primes the digit geometries admit: 29 NL - 20 bits, R / p >= 2^20 with nothing to spare
    # (csrc/padic_dec_kernels.hip: padic_nl_for_prime_bits, csrc/pair_kernels.hip: pair_nl_for_prime_bits), and n sits on the
    # 112- / 144-limb pair geometries (pair_nl_for_n_bits: n of at most 3228 / 4156 bits)
    assert [29 * NL[b] - 20 for b in (676, 1604, 2068)] == [676, 1604, 2068]
    assert 2 * 1604 <= 29 * 112 - 20 and 2 * 2068 <= 29 * 144 - 20


@pytest.mark.parametrize("ident,family,b,p,q", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_structure(ident, family, b, p, q):
    n = p * q
    assert p != q and p.bit_length() == b and q.bit_length() == b and n.bit_length() == 2 * b
    assert math.gcd(n, (p - 1) * (q - 1)) == 1
    if family == "ones":
        assert p < q and is_ones(p, b) and is_ones(q, b)
        assert (n >> (b + 32)) == (1 << (b - 32)) - 1                     # the top halves of n and n^2 are all ones
        assert ((n * n) >> (3 * b + 32)) == (1 << (b - 32)) - 1
    elif family == "zeros":
        assert p < q and is_zeros(p, b) and is_zeros(q, b)
    elif family == "ones_zeros":
        assert is_zeros(p, b) and is_ones(q, b) and (q - p).bit_length() == b - 2
    elif family == "half":
        h = RB * NL[b] // 2
        limbs = [(p >> (RB * i)) & MASK for i in range(NL[b])]
        assert all(v == MASK for v in limbs[1:NL[b] // 2]), "low Karatsuba half: all ones above the lowest limb"
        assert (p >> h) == 3 << (b - 2 - h), "high half: zero below the top two bits"
        assert is_ones(q, b)
    elif family == "n0":
        assert p % (1 << 58) == 1 and q % (1 << 58) == (1 << 58) - 1
        assert 0 <= p - (3 << (b - 2)) < 1 << 78 and 0 < (1 << b) - q < 1 << 78        # a few steps of 2^58 from the starting points
        assert (n0inv(p), n0inv(q)) == (MASK, 1)
        assert n & MASK == MASK and n0inv(n) == 1 and n0inv(n * n) == MASK
    elif family == "n0_one":
        assert p % (1 << 58) == 1 and q % (1 << 58) == 1
        assert 0 <= p - (3 << (b - 2)) < 1 << 78 and 0 < (1 << b) - q < 1 << 78
        assert (n0inv(p), n0inv(q), n0inv(n), n0inv(n * n)) == (MASK, MASK, MASK, MASK)
    else:
        raise AssertionError(family)


def test_primes_are_prime():
    for x in sorted({v for e in ENTRIES for v in e[3:]}):
        assert orc.is_probable_prime(x), hex(x)


@pytest.mark.parametrize("ident,family,b,p,q", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_oracle_roundtrip(ident, family, b, p, q, monkeypatch):
    key = orc.make_key(p, q, djn_x=0x1234567, bits=2 * b)
    n = key.n
    consts = orc.crt_constants(key)                       # (decrypt_crt derives them at every call: half of its time at the wide keys)
    monkeypatch.setattr(orc, "crt_constants", lambda k: consts)
    # (a short r: decryption does not care how a ciphertext was obfuscated, and CPython's pow with a b-bit r is most of the cost)
    cts = {m: orc.encrypt(key, m, 0xFEDCBA9876543211 + m % 7) for m in (0, 1, n - 1, n // 2)}
    for m, c in cts.items():
        assert orc.decrypt_crt(key, c) == m
    assert orc.decrypt_lambda(key, cts[n // 2]) == n // 2
