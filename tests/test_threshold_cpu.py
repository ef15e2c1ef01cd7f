"""CPU: the integer side of threshold decryption (pailliercryptolib_python_amd/threshold.py) — deal, lagrange, theta — against a
Fraction model, and the whole scheme (partial decryptions, combine, the consistency test) in CPython integers.  No GPU, no native
library: everything here is what the dealer and the Python layer compute on the host."""
import itertools
import json
import math
import pickle
import random
from fractions import Fraction
from pathlib import Path

import pytest

from oracle import chacha20
from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierKeyShare, PaillierPartialDecryption
from pailliercryptolib_python_amd import threshold as th
from tests.test_gpu_recover import P_DIV, Q_DIV

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((1, 1), (2, 2), (3, 2), (5, 3), (16, 1), (16, 16))
DJN_X = 0xABCDEF1234567


def fixture_primes(bits):
    if bits == 256:
        return orc.seeded_prime(128, 2561), orc.seeded_prime(128, 2562)
    fx = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())[str(bits)]
    return int(fx["p"], 16), int(fx["q"], 16)


def frac_lagrange(indices, parties):
    """mu_i = Delta prod_(j != i) j / (j - i) as exact fractions"""
    D = math.factorial(parties)
    return [D * math.prod(Fraction(j, j - i) for j in indices if j != i) for i in indices]


def signed(mags, negs):
    return [-m if s else m for m, s in zip(mags, negs)]


# ---- deal -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", (256, 1024))
@pytest.mark.parametrize("parties,threshold", SHAPES)
def test_deal(bits, parties, threshold):
    p, q = fixture_primes(bits)
    n, lam = p * q, math.lcm(p - 1, q - 1)
    d, shares = th.deal(p, q, parties, threshold, th.SeededRng(bits + 100 * parties + threshold))
    assert d % lam == 0 and d % n == 1 and 0 <= d < n * lam
    assert len(shares) == parties and all(0 <= s < n * lam for s in shares)
    D = math.factorial(parties)
    rng = random.Random(bits + parties)
    subsets = [list(range(1, threshold + 1)), list(range(parties - threshold + 1, parties + 1))]
    subsets += [sorted(rng.sample(range(1, parties + 1), threshold)) for _ in range(4)]
    for S in subsets:
        mu = signed(*th.lagrange(S, parties))
        assert sum(m * shares[i - 1] for m, i in zip(mu, S)) % (n * lam) == D * d % (n * lam), S
    if threshold == 1:
        assert all(s == d for s in shares)
    else:
        assert len(set(shares)) == parties


def test_theta():
    p, q = fixture_primes(256)
    for parties in (1, 3, 16):
        D = math.factorial(parties)
        assert th.theta(p * q, parties) * 4 * D * D % (p * q) == 1
    with pytest.raises(ValueError):
        th.theta(3 * 1000003, 3)


# ---- lagrange against Fraction -----------------------------------------------------------------------------------------------------------
def test_lagrange_every_subset_up_to_8():
    count = 0
    for parties in range(1, 9):
        for t in range(1, parties + 1):
            for S in itertools.combinations(range(1, parties + 1), t):
                want = frac_lagrange(S, parties)
                assert all(w.denominator == 1 for w in want)
                assert signed(*th.lagrange(S, parties)) == [int(w) for w in want], (parties, S)
                count += 1
    assert count == sum(2 ** l - 1 for l in range(1, 9))


def test_lagrange_samples_at_16_and_the_bit_bound():
    rng = random.Random(16)
    worst = 0
    for _ in range(2000):
        t = rng.randrange(1, 17)
        S = rng.sample(range(1, 17), t)                      # any order: the coefficients follow the order given
        want = frac_lagrange(S, 16)
        mags, negs = th.lagrange(S, 16)
        assert signed(mags, negs) == [int(w) for w in want] and all(w.denominator == 1 for w in want)
        assert all(m > 0 for m in mags)
        worst = max(worst, max((2 * m).bit_length() for m in mags))
    assert worst <= th.MU_BITS_MAX <= 32 * th.MU_WORDS
    assert math.factorial(th.MAX_PARTIES) < 1 << 45


def test_lagrange_refusals():
    for bad in ([], [1, 1], [0, 1], [1, 6]):
        with pytest.raises(ValueError):
            th.lagrange(bad, 5)


# ---- the whole scheme in integers ---------------------------------------------------------------------------------------------------------
def combine_ints(n, parties, parts):
    """parts: {index: c_i} -> (m, consistent)"""
    nsq = n * n
    S = sorted(parts)
    x = 1
    for i, m, neg in zip(S, *th.lagrange(S, parties)):
        base = pow(parts[i], -1, nsq) if neg else parts[i]
        x = x * pow(base, 2 * m, nsq) % nsq
    if x % n != 1:
        return None, False
    return (x - 1) // n * th.theta(n, parties) % n, True


def test_scheme_recovers_every_message_from_every_subset():
    p, q = fixture_primes(256)
    n, nsq = p * q, p * q * p * q
    parties, threshold = 5, 3
    _, shares = th.deal(p, q, parties, threshold, th.SeededRng(53))
    D = math.factorial(parties)
    djn = orc.make_key(p, q, djn_x=DJN_X, bits=256)
    std = orc.make_key(p, q, djn_x=None, bits=256)
    rng = random.Random(5)
    msgs = [0, 1, n - 1, (n - 1) // 2, n // 3, rng.randrange(n)]
    cases = []
    for m in msgs:
        cases.append((orc.encrypt(djn, m, rng.getrandbits(djn.randbits)), m))
        cases.append((orc.encrypt(std, m, rng.randrange(1, n)), m))
    a, b = cases[-1], cases[-2]
    cases.append((a[0] * b[0] % nsq, (a[1] + b[1]) % n))                     # a sum
    cases.append((pow(a[0], 12345, nsq), a[1] * 12345 % n))                  # a scalar multiple
    cases.append((pow(pow(a[0], -1, nsq), 7, nsq), -7 * a[1] % n))           # a negative one
    cases.append((1, 0))
    cases.append((nsq - 1, None))                                            # -1: (-1)^(4 Delta^2 d) = 1, an encryption of 0
    for c, m in cases:
        parts = {i: pow(c, 2 * D * shares[i - 1], nsq) for i in range(1, parties + 1)}
        want = orc.decrypt_crt(djn, c)
        assert m is None or want == m
        for S in itertools.combinations(range(1, parties + 1), threshold):
            got, ok = combine_ints(n, parties, {i: parts[i] for i in S})
            assert ok and got == want, (S, m)
    # too few shares, and a share under a wrong index, fail the test modulo n
    c, m = cases[0][0], cases[0][1]
    c = orc.encrypt(djn, 1234567, 99)
    parts = {i: pow(c, 2 * D * shares[i - 1], nsq) for i in range(1, parties + 1)}
    for S in itertools.combinations(range(1, parties + 1), threshold - 1):
        assert combine_ints(n, parties, {i: parts[i] for i in S})[1] is False, S
    assert combine_ints(n, parties, {1: parts[1], 2: parts[2], 4: parts[3]})[1] is False
    assert combine_ints(n, parties, {1: parts[1], 2: parts[2], 3: parts[3]}) == (1234567, True)


# ---- refusals, pickling, repr, seeds ------------------------------------------------------------------------------------------------------
def test_refusals():
    p, q = fixture_primes(256)
    rng = th.SeededRng(1)
    for parties, threshold in ((3, 4), (17, 2), (0, 0), (0, 1), (3, 0)):
        with pytest.raises(ValueError):
            th.deal(p, q, parties, threshold, rng)
    assert math.gcd(P_DIV * Q_DIV, math.lcm(P_DIV - 1, Q_DIV - 1)) != 1
    with pytest.raises(ValueError, match="coprime"):
        th.deal(P_DIV, Q_DIV, 3, 2, rng)
    with pytest.raises(ValueError):
        th.deal(p, p, 3, 2, rng)


class _Pub:
    """stands in for a PaillierPublicKey where only n is read"""

    def __init__(self, n):
        self.n = n


def test_share_objects_pickle_and_hide_the_share():
    p, q = fixture_primes(256)
    _, shares = th.deal(p, q, 5, 3, th.SeededRng(7))
    pub = _Pub(p * q)
    sh = PaillierKeyShare(pub, 2, 5, 3, shares[1])
    assert sh.exponent() == 2 * 120 * shares[1]
    for text in (repr(sh), str(sh)):
        assert "2 of (5, 3)" in text
        assert str(shares[1]) not in text and hex(shares[1])[2:] not in text and str(sh.exponent()) not in text
    back = pickle.loads(pickle.dumps(sh))
    assert back == sh and back.exponent() == sh.exponent() and (back.index, back.parties, back.threshold) == (2, 5, 3)
    with pytest.raises(ValueError) as ei:
        PaillierKeyShare(pub, 6, 5, 3, shares[1])
    assert str(shares[1]) not in str(ei.value)
    with pytest.raises(ValueError) as ei:
        PaillierKeyShare(pub, 2, 5, 3, -shares[1])
    assert str(shares[1]) not in str(ei.value)
    with pytest.raises(TypeError):
        sh.partial_decrypt([1, 2, 3])


def test_select_parts_refuses_unusable_sets():
    pub = _Pub(35)
    import numpy as np

    def part(index, length=4, parties=5, threshold=3, n=35, packing=None):
        return PaillierPartialDecryption(_Pub(n), np.zeros((length, 2), dtype=np.uint32), index, parties, threshold,
                                         None if packing else [0] * length, length, packing)

    good = [part(4), part(1), part(5), part(2)]
    assert [p.index for p in th.select_parts(pub, good, False)] == [1, 2, 4]          # more than threshold: the smallest indices
    for bad in ([part(1), part(2)], [part(1), part(2), part(2)], [part(1), part(2), part(3, length=5)],
                [part(1), part(2), part(3, parties=6)], [part(1), part(2), part(3, threshold=2)], [part(1), part(2), part(3, n=33)],
                [part(1), part(2), part(6)], [part(1), part(2), part(0)], [], [part(1), part(2), part(3, packing=(16, 2, 0, 8))]):
        with pytest.raises(ValueError):
            th.select_parts(pub, bad, False)
    with pytest.raises(ValueError):
        th.select_parts(pub, good, True)
    blob = pickle.loads(pickle.dumps(good[0]))
    assert isinstance(blob._t, np.ndarray) and (blob.index, blob.parties, blob.threshold, len(blob)) == (4, 5, 3, 4)


def test_seeded_dealing_is_reproducible_and_the_stream_is_chacha20():
    p, q = fixture_primes(256)
    a = th.deal(p, q, 5, 3, th.SeededRng(42))
    assert a == th.deal(p, q, 5, 3, th.SeededRng(42))
    assert a[1] != th.deal(p, q, 5, 3, th.SeededRng(43))[1]
    key = list(range(1, 9))
    assert th._chacha_block(key, 7, (0, 0, 0)) == chacha20.block(key, 7, [0, 0, 0])
    seed = sum(k << (32 * i) for i, k in enumerate(key))
    rng = th.SeededRng(seed)
    first = rng(1 << 64)
    assert first == chacha20.block(key, 0, [0, 0, 0])[0] | chacha20.block(key, 0, [0, 0, 0])[1] << 32
    assert all(0 <= th.SeededRng(s)(10) < 10 for s in range(50))
