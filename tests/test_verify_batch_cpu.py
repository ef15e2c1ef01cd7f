"""CPU: the model of the batch verification of openings (pai_opening_fold / PaillierPublicKey.verify_openings).

fold_expect is the expectation of tests/test_gpu_verify_batch.py: CPython ints and pow only.  Here it is held to the definition of
an opening (tests.test_recover_cpu.reencrypt) on the 1024-bit fixture key: valid openings agree on both sides, a changed plaintext
does not pass, (m, n - r) passes exactly when the coefficients of those elements sum to an even number, and a multiple of p among the
r makes the unit test fail."""
import json
import math
import random
from pathlib import Path

from tests.test_recover_cpu import reencrypt

ROOT = Path(__file__).resolve().parent.parent


def fold_expect(n, cts, ms, rs, es, L):
    """(lhs, rhs, unit) of pai_opening_fold for segments of L consecutive rows: lhs[s] = prod ct_i^(e_i) mod n^2,
    rhs[s] = (1 + n M_s) B_s^n mod n^2 with M_s = sum e_i m_i mod n and B_s = prod r_i^(e_i) mod n; unit: every B_s is invertible
    modulo n (bit 0 of the device flag is its negation)."""
    nsq = n * n
    lhs, rhs, unit = [], [], True
    for s0 in range(0, len(cts), L):
        A, B, M = 1, 1, 0
        for c, m, r, e in zip(cts[s0:s0 + L], ms[s0:s0 + L], rs[s0:s0 + L], es[s0:s0 + L]):
            A = A * pow(c, e, nsq) % nsq
            B = B * pow(r, e, n) % n
            M = (M + e * m) % n
        lhs.append(A)
        rhs.append((1 + n * M) * pow(B, n, nsq) % nsq)
        unit = unit and math.gcd(B, n) == 1
    return lhs, rhs, unit


def fixture_1024():
    fx = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())["1024"]
    return int(fx["p"], 16), int(fx["q"], 16)


def batch(n, count, rng):
    ms = [rng.randrange(n) for _ in range(count)]
    rs = [rng.randrange(1, n) for _ in range(count)]
    return [reencrypt(n, m, r) for m, r in zip(ms, rs)], ms, rs


def test_valid_openings_agree():
    p, q = fixture_1024()
    n = p * q
    rng = random.Random(1)
    cts, ms, rs = batch(n, 13, rng)
    for lam in (32, 128):
        es = [rng.getrandbits(lam) for _ in cts]
        es[3] = 0
        for L in (1, 3, 13, 18):
            lhs, rhs, unit = fold_expect(n, cts, ms, rs, es, L)
            assert lhs == rhs and unit and len(lhs) == -(-13 // L)
    # one row, coefficient one: the two sides are the ciphertext and its re-encryption
    lhs, rhs, unit = fold_expect(n, cts[:1], ms[:1], rs[:1], [1], 1)
    assert lhs == [cts[0]] and rhs == [reencrypt(n, ms[0], rs[0])] and unit


def test_changed_plaintext_never_passes():
    """64 draws at 32-bit coefficients: a false pass needs e_j = 0 modulo n / gcd(mu_j, n) >= min(p, q) > 2^32, i.e. e_j = 0 —
    probability at most 64 * 2^-32 over the seeded draws (and the seed below has none)."""
    p, q = fixture_1024()
    n = p * q
    rng = random.Random(2)
    cts, ms, rs = batch(n, 8, rng)
    for draw in range(64):
        es = [rng.getrandbits(32) for _ in cts]
        j = draw % 8
        wrong = list(ms)
        wrong[j] = (ms[j] + 1 + rng.randrange(n - 1)) % n
        lhs, rhs, unit = fold_expect(n, cts, wrong, rs, es, 8)
        assert unit and lhs != rhs


def test_negated_randomness_passes_iff_the_coefficient_sum_is_even():
    p, q = fixture_1024()
    n = p * q
    rng = random.Random(3)
    cts, ms, rs = batch(n, 9, rng)
    seen = set()
    for draw in range(24):
        es = [rng.getrandbits(32) for _ in cts]
        J = rng.sample(range(9), 1 + draw % 4)
        neg = [n - r if i in J else r for i, r in enumerate(rs)]
        for i in J:
            assert reencrypt(n, ms[i], neg[i]) == n * n - cts[i]          # Enc(m, n - r) = -Enc(m, r): n is odd
        lhs, rhs, unit = fold_expect(n, cts, ms, neg, es, 9)
        even = sum(es[i] for i in J) % 2 == 0
        assert unit and (lhs == rhs) == even
        seen.add(even)
    assert seen == {True, False}


def test_a_multiple_of_p_among_r_fails_the_unit_test():
    p, q = fixture_1024()
    n = p * q
    rng = random.Random(4)
    cts, ms, rs = batch(n, 6, rng)
    es = [rng.getrandbits(32) | 1 for _ in cts]
    rs[2] = p
    cts[2] = reencrypt(n, ms[2], p)
    lhs, rhs, unit = fold_expect(n, cts, ms, rs, es, 3)
    assert not unit
    assert lhs == rhs                                                     # the identity holds; it is the proof that is void
    # ... which is why: p^2 | both sides of the segment, whatever m_2 is claimed
    ms[2] = (ms[2] + 1) % n
    lhs2, rhs2, _ = fold_expect(n, cts, ms, rs, es, 3)
    assert lhs2[0] % (p * p) == rhs2[0] % (p * p) == 0
