"""CPU: proofs of correct partial decryption (pailliercryptolib_python_amd/threshold.py) in CPython integers and
hashlib — the integer model that defines the transcript's byte layout and is the oracle of the device path — on the safe-prime keys
of tests/golden/safe_prime_keys.json.  No GPU."""
import hashlib
import json
import math
import pickle
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from pailliercryptolib_python_amd import (PaillierDecryptionProof, PaillierKeyShare, PaillierPartialDecryption, PaillierVerificationKey,
                                          _native)
from pailliercryptolib_python_amd import threshold as th
from tests.test_threshold_cpu import _Pub

ROOT = Path(__file__).resolve().parent.parent
KEYS = {k["name"]: k for k in json.loads((ROOT / "tests" / "golden" / "safe_prime_keys.json").read_text())}
SHAPES = ((1, 1), (3, 2), (16, 16))


class Setup:
    """a dealing of one fixture key with N ciphertexts of known plaintexts and every share's partial decryptions"""

    def __init__(self, name, parties, threshold, N=4):
        k = KEYS[name]
        self.p, self.q, self.key_bits = int(k["p"], 16), int(k["q"], 16), k["key_bits"]
        self.n = self.p * self.q
        self.nsq = self.n * self.n
        self.parties, self.threshold = parties, threshold
        rng = th.SeededRng(1000 * parties + threshold)
        self.d, self.shares, self.v, self.values = th.deal_verifiable(self.p, self.q, parties, threshold, rng)
        self.ms = [rng(self.n) for _ in range(N)]
        self.cts = [(1 + m * self.n) * pow(rng(self.n - 1) + 1, self.n, self.nsq) % self.nsq for m in self.ms]
        self.D = math.factorial(parties)

    def parts(self, index, cts=None):
        return [pow(c, 2 * self.D * self.shares[index - 1], self.nsq) for c in (self.cts if cts is None else cts)]

    def nonce(self, salt=0):
        return th.SeededRng(77 + salt)(1 << th.nonce_bits(self.n, self.parties))

    def prove(self, index, parts=None, cts=None, salt=0):
        return th.prove_int(self.n, self.key_bits, self.parties, self.threshold, index, self.shares[index - 1], self.v,
                            self.values[index - 1], self.cts if cts is None else cts, self.parts(index) if parts is None else parts,
                            self.nonce(salt))

    def verify(self, index, parts, proof, cts=None):
        return th.verify_int(self.n, self.key_bits, self.parties, self.threshold, index, self.v, self.values[index - 1],
                             self.cts if cts is None else cts, parts, proof)

    def combine(self, parts_by_index):
        """the plaintexts from `threshold` parts {index: rows}"""
        idx = sorted(parts_by_index)[:self.threshold]
        mags, negs = th.lagrange(idx, self.parties)
        out = []
        for j in range(len(self.cts)):
            x = 1
            for i, m, s in zip(idx, mags, negs):
                f = pow(parts_by_index[i][j], 2 * m, self.nsq)
                x = x * (pow(f, -1, self.nsq) if s else f) % self.nsq
            assert x % self.n == 1
            out.append((x - 1) // self.n * th.theta(self.n, self.parties) % self.n)
        return out


_SETUPS = {}


def setup(name, parties, threshold):
    key = (name, parties, threshold)
    if key not in _SETUPS:
        _SETUPS[key] = Setup(name, parties, threshold)
    return _SETUPS[key]


# ---- the byte layout, spelled out once more -----------------------------------------------------------------------------------------------
def test_transcript_layout():
    s = setup("toy", 3, 2)
    nw, W = th.key_words(s.key_bits)
    assert (nw, W) == (4, 8)
    parts = s.parts(2)
    leaves = th.transcript_leaves(s.cts, parts, s.key_bits)
    assert leaves == b"".join(hashlib.sha256(c.to_bytes(32, "little") + ci.to_bytes(32, "little")).digest() for c, ci in zip(s.cts, parts))
    root = th.transcript_root(s.n, s.key_bits, 3, 2, 2, s.v, s.values[1], leaves)
    want = hashlib.sha256(b"pai-tdec-v1" + struct.pack("<I", 128) + s.n.to_bytes(16, "little") + struct.pack("<III", 3, 2, 2)
                          + s.v.to_bytes(32, "little") + s.values[1].to_bytes(32, "little") + struct.pack("<Q", len(s.cts)) + leaves).digest()
    assert root == want
    r = th.rho(root, 3, first=5)
    assert r == [int.from_bytes(hashlib.sha256(root + b"pai-rho" + struct.pack("<Q", j)).digest()[:16], "little") for j in (5, 6, 7)]
    e = th.challenge(root, s.key_bits, 11, 12, 13, 14)
    assert e == int.from_bytes(hashlib.sha256(root + b"pai-chal" + b"".join(x.to_bytes(32, "little") for x in (11, 12, 13, 14))).digest()[:16],
                               "little")
    assert th.nonce_bits(s.n, 3) == 2 * 128 + 3 + 256
    assert th.verification_values(s.n, 3, s.shares, s.v) == [pow(s.v, 6 * x, s.nsq) for x in s.shares] == s.values


# ---- honest parts verify ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("toy", "k1024"))
@pytest.mark.parametrize("parties,threshold", SHAPES)
def test_honest_part_verifies(name, parties, threshold):
    s = setup(name, parties, threshold)
    for index in sorted({1, parties}):
        parts = s.parts(index)
        a, b, z = proof = s.prove(index)
        assert 1 <= a < s.nsq and 1 <= b < s.nsq and 0 <= z < 1 << (th.nonce_bits(s.n, parties) + 1)
        assert s.verify(index, parts, proof)
        assert s.verify(index, parts, PaillierDecryptionProof(*proof))
    if threshold <= 3:
        assert s.combine({i: s.parts(i) for i in range(1, threshold + 1)}) == s.ms


def test_empty_container_verifies():
    s = setup("toy", 3, 2)
    proof = s.prove(1, parts=[], cts=[])
    assert s.verify(1, [], proof, cts=[])
    assert not s.verify(2, [], proof, cts=[])


# ---- what is rejected ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("toy", "k1024"))
def test_rejections(name):
    s = setup(name, 3, 2)
    parts = s.parts(2)
    proof = s.prove(2)
    assert s.verify(2, parts, proof)
    # a part under another share's exponent: the prover of share 2 sends (and proves over) share 3's rows
    other = s.parts(3)
    assert not s.verify(2, other, s.prove(2, parts=other))
    assert not s.verify(2, other, proof)
    # the attack DESIGN 2.8d names: a row times (1 + n)^k passes combine's test and shifts the plaintext
    shifted = list(parts)
    shifted[1] = shifted[1] * pow(1 + s.n, 5, s.nsq) % s.nsq
    assert not s.verify(2, shifted, s.prove(2, parts=shifted))
    assert not s.verify(2, shifted, proof)
    # two rows swapped
    swapped = [parts[1], parts[0]] + parts[2:]
    assert not s.verify(2, swapped, s.prove(2, parts=swapped))
    assert not s.verify(2, swapped, proof)
    # a proof replayed on another container
    cts2 = [c * c % s.nsq for c in s.cts]
    assert not s.verify(2, s.parts(2, cts2), proof, cts=cts2)
    assert s.verify(2, s.parts(2, cts2), s.prove(2, parts=s.parts(2, cts2), cts=cts2), cts=cts2)
    # the proof under another index, ranges
    assert not s.verify(1, parts, proof)
    a, b, z = proof
    B = th.nonce_bits(s.n, 3)
    assert not s.verify(2, parts, (a, b, z + (1 << (B + 1))))
    assert not s.verify(2, parts, (a, b, 1 << (B + 1)))
    assert not s.verify(2, parts, (0, b, z))
    assert not s.verify(2, parts, (a, 0, z))
    assert not s.verify(2, parts, (a + s.nsq, b, z))
    assert not s.verify(2, parts, (a, b, z + 1))
    assert not s.verify(2, parts, None)
    # rows that are no residues: the part is rejected, the container is an error
    assert not s.verify(2, [parts[0] + s.nsq] + parts[1:], proof)
    assert not s.verify(2, parts[:-1], proof)
    with pytest.raises(ValueError, match="residue"):
        s.verify(2, parts, proof, cts=[s.cts[0] + s.nsq] + s.cts[1:])
    with pytest.raises(ValueError, match="residue"):
        s.prove(2, cts=[s.cts[0] + s.nsq] + s.cts[1:])
    with pytest.raises(ValueError, match="nonce"):
        th.prove_int(s.n, s.key_bits, 3, 2, 2, s.shares[1], s.v, s.values[1], s.cts, parts, 1 << B)


@pytest.mark.parametrize("name", ("toy", "k1024"))
def test_negated_row_is_accepted_and_combines_to_the_same_plaintext(name):
    s = setup(name, 3, 2)
    parts = s.parts(2)
    neg = list(parts)
    neg[0] = s.nsq - neg[0]
    neg[2] = s.nsq - neg[2]
    assert s.verify(2, neg, s.prove(2, parts=neg))                 # the squares are what is certified, and what combine uses
    assert s.combine({1: s.parts(1), 2: neg}) == s.combine({1: s.parts(1), 2: parts}) == s.ms


# ---- the dealer ---------------------------------------------------------------------------------------------------------------------------
def test_seeded_shares_with_and_without_verification_values_are_equal():
    k = KEYS["k1024"]
    p, q = int(k["p"], 16), int(k["q"], 16)
    for parties, threshold in SHAPES:
        plain = th.deal(p, q, parties, threshold, th.SeededRng(5))
        d, shares, v, values = th.deal_verifiable(p, q, parties, threshold, th.SeededRng(5))
        assert (d, shares) == plain
        n = p * q
        u2 = v
        assert 0 < v < n * n and math.gcd(v, n) == 1 and len(values) == parties
        assert pow(u2, (p - 1) * (q - 1) // 4 * n, n * n) == 1      # a square of a unit: its order divides n p' q'
    # the native host exponentiation gives the dealer the same values as pow
    d, shares, v, values = th.deal_verifiable(p, q, 3, 2, th.SeededRng(5))
    assert th.verification_values(p * q, 3, shares, v, _native.host_modexp) == values


def test_safe_primes_and_small_order_factor():
    for name in KEYS:
        p, q = int(KEYS[name]["p"], 16), int(KEYS[name]["q"], 16)
        assert th.safe_primes(p, q) and th.small_order_factor(p, q) == 0
    fx = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())["1024"]
    p, q = int(fx["p"], 16), int(fx["q"], 16)
    assert not th.safe_primes(p, q)                                 # the package's generator does not make safe primes
    want = next((f for f in range(3, 1 << 20, 2) if th.is_probable_prime(f) and (p - 1) * (q - 1) % f == 0), 0)
    assert th.small_order_factor(p, q) == want
    # a key with 3 | p - 1
    q3 = int(KEYS["toy"]["q"], 16)
    p3 = next(c for c in range(1 << 63, (1 << 63) + 100000) if c % 6 == 1 and th.is_probable_prime(c))
    assert (p3 - 1) % 3 == 0
    assert not th.safe_primes(p3, q3) and th.small_order_factor(p3, q3) == 3
    # Miller-Rabin against trial division, Carmichael numbers included
    for m in range(0, 3000):
        assert th.is_probable_prime(m) == (m >= 2 and all(m % f for f in range(2, math.isqrt(m) + 1))), m
    for m in (561, 1105, 1729, 2465, 2821, 6601, 8911, 41041, 825265, 321197185, (1 << 61) + 1, ((1 << 61) - 1) * ((1 << 31) - 1)):
        assert not th.is_probable_prime(m), m
    for m in ((1 << 31) - 1, (1 << 61) - 1, (1 << 127) - 1):
        assert th.is_probable_prime(m), m


# ---- objects ------------------------------------------------------------------------------------------------------------------------------
def test_pickles_with_both_tuple_lengths():
    s = setup("toy", 3, 2)
    pub = _Pub(s.n)
    vk = PaillierVerificationKey(s.n, 3, 2, s.v, s.values, True, 0)
    assert pickle.loads(pickle.dumps(vk)) == vk and "safe_primes=True" in repr(vk)
    assert (vk.n, vk.parties, vk.threshold, vk.v, list(vk.values), vk.safe_primes, vk.small_order_factor) == (s.n, 3, 2, s.v, s.values, True, 0)
    with pytest.raises(ValueError):
        PaillierVerificationKey(s.n, 3, 2, s.v, s.values[:2])
    plain, ver = PaillierKeyShare(pub, 2, 3, 2, s.shares[1]), PaillierKeyShare(pub, 2, 3, 2, s.shares[1], vk)
    assert plain.verification_key is None and ver.verification_key is vk
    assert len(plain.__getstate__()) == 5 and len(ver.__getstate__()) == 6
    for sh in (plain, ver):
        back = pickle.loads(pickle.dumps(sh))
        assert back == sh and back.verification_key == sh.verification_key and back.exponent() == sh.exponent()
    old = PaillierKeyShare.__new__(PaillierKeyShare)
    old.__setstate__(plain.__getstate__()[:5])                      # a pickle written before verification keys existed
    assert old == plain and old.verification_key is None
    with pytest.raises(ValueError, match="another dealing"):
        PaillierKeyShare(pub, 2, 3, 3, s.shares[1], vk)
    proof = PaillierDecryptionProof(*s.prove(2))
    assert pickle.loads(pickle.dumps(proof)) == proof and tuple(proof) == (proof.a, proof.b, proof.z)
    words = np.arange(8, dtype=np.uint32).reshape(1, 8)
    bare = PaillierPartialDecryption(pub, words, 2, 3, 2, [0], 1)
    with_proof = PaillierPartialDecryption(pub, words, 2, 3, 2, [0], 1, None, proof)
    assert bare.proof is None and len(bare.__getstate__()) == 8 and len(with_proof.__getstate__()) == 9
    for part in (bare, with_proof):
        back = pickle.loads(pickle.dumps(part))
        assert back.proof == part.proof and np.array_equal(back.host_words(), words) and (back.index, len(back)) == (2, 1)
    old = PaillierPartialDecryption.__new__(PaillierPartialDecryption)
    old.__setstate__(bare.__getstate__())
    assert old.proof is None


def test_header_and_prototypes_carry_the_transcript_entry_points():
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    for name in ("pai_sha256_rows", "pai_sha256_expand"):
        assert re.search(r"\bint " + name + r"\s*\(", header) and name in _native.PROTOTYPES
        assert hasattr(_native.load(), name)
    assert len(_native.PROTOTYPES["pai_sha256_rows"][1]) == 7 and len(_native.PROTOTYPES["pai_sha256_expand"][1]) == 10
    assert "pai_sha256_rows" in (ROOT / "INTEGRATION.md").read_text()
