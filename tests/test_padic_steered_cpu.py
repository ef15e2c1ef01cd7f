"""CPU: steered ciphertexts (tests/_steer.py) on the cell-exact model of the balanced-digit decrypt kernel (tools/kara_model.py:
kara_pass_bal; csrc/mont_padic.hpp: kara_pass_bal, kernel modes PADIC_LDS_KMRB / PADIC_LDS_KMRBS).

The one-cell-per-column design rests on |d_k| < 36 (2^57 + 2^56) + 2^28 + 2^35 < 2^62.76 and |carry| < 2^34.  Real encryptions
and random residues reach 2^59.2 .. 2^60.3: their limbs are uniform after the first product and a column is a random walk.  A
steered ciphertext is the e_k-th root of a chosen digit pair, so that after schedule entry k the kernel's registers hold limbs
at +-2^28 and the next squaring runs its columns to 2^62.1 (2^61.7 on the 26 free limbs of a 768-bit prime).  Here, for every
key of tests/test_gpu_padic_kred.py: KEYS (the keys tests/test_gpu_padic_steered.py decrypts on the GPU):
  - at least one prime of every key is steerable, and both primes of the bench key,
  - pow(c, e_k, s^2) R == w* + v* s, and the model's registers after entry k ARE (w*, v*), limb for limb, in the two-sum form
    and both one-sum placements (where the only usable step lies beyond entry 16 — n0_one, entry 159 — for one target pair),
  - the squaring that follows has a column of at least 2^62 (2^61.5 at 26 limbs) and a carry outside the signed 33-bit range,
  - the chain started from the canonical Montgomery pair instead of the digit-form entry's lazy pair gives the same limbs from
    the first product on (the uniqueness the method rests on),
  - a random unit's chain over the same steps, and its next squaring, stay below 2^61."""
import math
import random

import pytest

from tests import _steer as st
from tests._steer import km
from tests.test_gpu_padic_kred import KEYS

REDS = {"two_sums": km.KMRB_RED, "one_sum": km.KMRBS_RED, "one_sum_twice": km.KMRBS_RED | km.ONES2}
_KEYS = {}


def key_of(ident):
    if ident not in _KEYS:
        _KEYS[ident] = KEYS[ident]()
    return _KEYS[ident]


def steerable(ident):
    """[(which, k)] of the key's primes that have a usable step."""
    key = key_of(ident)
    out = []
    for which in (0, 1):
        steps = st.usable_steps(st.prime_of(key, which))
        if steps:
            out.append((which, steps[0][0]))
    return out


def _cases():
    """(ident, which, pair index): every target pair on every steerable prime; one pair where the step is far."""
    out = []
    for ident in KEYS:
        for which, k in steerable(ident):
            for j in range(len(st.PAIRS) if k <= st.FAR_STEP else 1):
                out.append(pytest.param(ident, which, j, id=f"{ident}-{'pq'[which]}-{'_'.join(st.PAIRS[j])}"))
    return out


def _primes():
    return [pytest.param(ident, which, id=f"{ident}-{'pq'[which]}") for ident in KEYS for which, _ in steerable(ident)]


def test_every_key_has_a_steerable_prime():
    for ident in KEYS:
        got = steerable(ident)
        assert got, ident
        print(f"{ident}: " + ", ".join(f"{'pq'[w]}: k={k}" for w, k in got))
    assert [w for w, _ in steerable("bench-2048")] == [0, 1]
    assert [st.free_limbs(st.prime_of(key_of("seeded-1536"), w)) for w in (0, 1)] == [26, 26]
    assert all(st.free_limbs(st.prime_of(key_of(i), w)) == 35 for i in KEYS if i != "seeded-1536" for w in (0, 1))


def test_no_step_where_every_prefix_shares_a_factor():
    """The other prime of a structured key: steer() says so instead of returning a root that does not exist."""
    key = key_of("ones-1024")
    which = 1 - steerable("ones-1024")[0][0]
    s = st.prime_of(key, which)
    _, w, v = st.target_pairs(s)[0]
    assert st.steer(s, w, v) is None and st.steered_ciphertext(key, which, w, v, random.Random(1)) is None


_CHAINS = {}


def chain(ident, which, j, red_name):
    """(c, k, e_k, registers after entry k, trace) of target pair j on that prime, from the digit-form entry; computed once."""
    at = (ident, which, j, red_name)
    if at not in _CHAINS:
        key = key_of(ident)
        s = st.prime_of(key, which)
        _, w, v = st.target_pairs(s)[j]
        c = st.steered_ciphertext(key, which, w, v, random.Random(1000 * j + which))
        c_s, k, e = st.steer(s, w, v)
        assert c % (s * s) == c_s and k == dict(steerable(ident))[which]
        a, b, trace = st.model_chain(s, c, k, km.BalStats(), REDS[red_name], ct_bits=2 * key.bits)
        _CHAINS[at] = (c, k, e, (a, b), trace)
    return _CHAINS[at]


@pytest.mark.parametrize("ident,which,j", _cases())
def test_steered_registers_and_next_squaring(ident, which, j):
    s = st.prime_of(key_of(ident), which)
    s2 = s * s
    name, w, v = st.target_pairs(s)[j]
    free = st.free_limbs(s)
    for red_name, red in REDS.items():
        c, k, e, regs, _ = chain(ident, which, j, red_name)
        assert (pow(c, e, s2) * st.R - (km.value(w) + km.value(v) * s)) % s2 == 0
        assert regs == (w, v), (name, red_name)
        d, carry, at = st.next_squaring(s, *regs, red)
        print(f"{ident} {'pq'[which]} k={k} {name} {red_name}: max |d| = 2^{math.log2(d):.2f} at (form, column) {at}, max |carry| = 2^{math.log2(carry):.2f}")
        if free == 35:
            assert d >= 1 << 62
        else:
            assert d * d >= 1 << 123                                    # 2^61.5
        assert d < 36 * (3 << 56) + (1 << 28) + (1 << 35)               # the bound itself
        assert carry > 1 << 32                                          # outside the signed 33-bit range


@pytest.mark.parametrize("ident,which", _primes())
def test_canonical_start_and_random_ceiling(ident, which):
    """The chain started from the canonical Montgomery pair holds the same limbs as the one started from the digit-form
    entry's lazy pair from the first product on (first target pair).  A random unit's columns over entries 0 .. k and in the
    squaring after them stay below 2^61: what the older inputs could reach."""
    key = key_of(ident)
    s = st.prime_of(key, which)
    c, k, e, regs, trace = chain(ident, which, 0, "one_sum")
    a2, b2, trace2 = st.model_chain(s, c, k, km.BalStats(), km.KMRBS_RED, canonical=True)
    first = [kind for kind, _, _ in trace].index("mul")
    assert len(trace) == len(trace2) and trace[first:] == trace2[first:] and regs == (a2, b2)
    rng = random.Random(77 + which)
    rnd = rng.randrange(1, key.nsq)
    while math.gcd(rnd, key.n) != 1:
        rnd = rng.randrange(1, key.nsq)
    stats = km.BalStats()
    a, b, _ = st.model_chain(s, rnd, k, stats, km.KMRBS_RED, ct_bits=2 * key.bits)
    assert (km.value(a) + km.value(b) * s - pow(rnd, e, s * s) * st.R) % (s * s) == 0
    d, carry, _ = st.next_squaring(s, a, b, km.KMRBS_RED)
    top = max(stats.max_d, d)
    print(f"{ident} {'pq'[which]} random unit, entries 0 .. {k} and the next squaring: max |d| = 2^{math.log2(top):.2f}, "
          f"max |carry| = 2^{math.log2(max(stats.max_c, carry)):.2f}")
    assert top < 1 << 61
