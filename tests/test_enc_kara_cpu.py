"""CPU: the cells of the two-step Karatsuba product (a, b) * (c, 0) at 72 limbs (csrc/mont_padic.hpp: kara2_step_bal,
mul_kara2_c0_bal; kernel: k_encrypt_padic with KARA) in the model tools/kara_model.py, which runs every stored sum and every
column in 64-bit cells that wrap and asserts that each finished column, read as a signed integer, is the exact schoolbook
column of its step.

mul_kara2_c0_bal(check=True) holds every product to the one-step rule in CPython integers: w R = a c + m n,
v R = b c - m + m' n with m, m' the unique balanced quotients modulo R, and w + v n == (a + b n) c R^-1 (mod n^2).
Operand families: every limb of a, b, c and n at -2^28 and at 2^28 - 1; moduli whose halves sit at opposite extremes or are
equal, split at 18 and at 36 limbs; the structured moduli of tests/golden/extreme_keys.json; operands at the lazy bound;
quotient digits forced to -2^28 and to 2^28 - 1 by solving for the operand; a chain of 128 products; the balanced
conversions in both directions.  The largest column over all of them stays below 2^62.2 (36 (2^56 + 2^56) + 2^36)."""
import math
import random
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import kara_model as km  # noqa: E402

from tests.test_extreme_keys_cpu import load_extreme_keys  # noqa: E402

NL, HL, H = 72, 36, 18
RB, B, HB = km.RB, km.B, km.HB
R = 1 << (RB * NL)
LO, HI = -HB, HB - 1
BOUND = int(2 ** 62.2)
ST = km.Kara2Stats()                 # shared: the largest column over every test of this file


def odd(limbs):
    """the limb list with an odd lowest limb (a modulus), one step towards zero"""
    out = list(limbs)
    if out[0] % 2 == 0:
        out[0] += 1
    return out


def modulus(limbs):
    """a positive odd modulus with these balanced limbs (the top limb made positive)"""
    out = odd(limbs)
    if km.value(out) <= 0:
        out[-1] = HI
    n = km.value(out)
    assert n > 0 and n % 2 == 1 and km.bal_limbs(n, NL) == out
    return n


def blocks(width, first, second):
    return [(first if (i // width) % 2 == 0 else second) for i in range(NL)]


def bench_n():
    from oracle import paillier_oracle as orc

    return orc.BENCH_P * orc.BENCH_Q


def product(a, b, c, n):
    return km.mul_kara2_c0_bal(a, b, c, n, ST)


def test_limbs_at_the_extremes():
    """every limb of a, b, c and n at -2^28 or at 2^28 - 1, in every combination of the four"""
    for nl in ([HI] * NL, [LO] * (NL - 1) + [HI]):
        n = modulus(nl)
        for a in ([LO] * NL, [HI] * NL):
            for b in ([LO] * NL, [HI] * NL):
                for c in ([LO] * NL, [HI] * NL):
                    product(a, b, c, n)
    assert 2 ** 62 < ST.max_d < BOUND


@pytest.mark.parametrize("width", [18, 36])
def test_moduli_with_opposite_and_equal_halves(width):
    rng = random.Random(width)
    half = [rng.randrange(LO, HI + 1) for _ in range(width)]
    equal = [half[i % width] for i in range(NL)]
    for nl in (blocks(width, LO, HI), blocks(width, HI, LO), equal):
        n = modulus(nl)
        nb = km.bal_limbs(n, NL)
        if nl is equal:
            assert all(nb[i] == nb[i + width] for i in range(1, width) if i + width < NL - 1)
        ops = [[LO] * NL, [HI] * NL, blocks(width, LO, HI), blocks(width, HI, LO), blocks(18, HI, LO)]
        ops.append(km.bal_limbs(rng.randrange(-n // 2, n // 2), NL))
        for i, a in enumerate(ops):
            product(a, ops[(i + 1) % len(ops)], ops[(i + 2) % len(ops)], n)
    assert ST.max_d < BOUND


@pytest.mark.parametrize("entry", [e for e in load_extreme_keys() if e[2] == 1024], ids=lambda e: e[0])
def test_structured_moduli(entry):
    _, _, _, p, q = entry
    n = p * q
    rng = random.Random(n % 1000003)
    top = 51 * n // 100
    lazy_c = km.balance_halves(km.limbs(2 * n + (n >> 18) - 1, NL))
    ops = [km.bal_limbs(top, NL), km.bal_limbs(-top, NL), lazy_c, km.bal_limbs(rng.randrange(-n // 2, n // 2), NL),
           km.balance_halves(km.limbs(rng.randrange(n), NL)), km.bal_limbs(0, NL)]
    for i, a in enumerate(ops):
        w, v, _, _ = product(a, ops[(i + 1) % len(ops)], ops[(i + 2) % len(ops)], n)
        if i < 3:
            assert km.in_lazy_range(w, n) and km.in_lazy_range(v, n)
    assert ST.max_d < BOUND


def test_operands_at_the_lazy_bound():
    """|a|, |b| = 0.51 n with c = 2.01 n, the range of a table entry: w and v are back inside 0.51 n"""
    n = bench_n()
    top = 51 * n // 100
    c = km.balance_halves(km.limbs(2 * n + n // 100, NL))
    assert km.value(c) == 2 * n + n // 100
    for sa in (1, -1):
        for sb in (1, -1):
            w, v, _, _ = product(km.bal_limbs(sa * top, NL), km.bal_limbs(sb * top, NL), c, n)
            assert km.in_lazy_range(w, n) and km.in_lazy_range(v, n)


def centred(x):
    x %= R
    return x - R if x >= R // 2 else x


@pytest.mark.parametrize("digit", [LO, HI])
def test_quotient_digits_forced_to_the_extremes(digit):
    """a and b solved so that all 72 digits of m and of m' are -2^28 resp. 2^28 - 1"""
    n = bench_n()
    rng = random.Random(5)
    cv = rng.randrange(n) | 1
    c = km.balance_halves(km.limbs(cv, NL))
    M = km.value([digit] * NL)
    ci = pow(cv, -1, R)
    a = centred(-M * n * ci)                  # a c + M n == 0 (mod R)
    b = centred((M - M * n) * ci)             # b c - M + M n == 0 (mod R)
    al, bl = km.bal_limbs(a, NL), km.bal_limbs(b, NL)
    assert all(LO <= x <= HI for x in al[:-1] + bl[:-1]) and abs(al[-1]) <= HB and abs(bl[-1]) <= HB
    ST.q_ext.clear()
    _, _, m, m2 = product(al, bl, c, n)
    assert m == [digit] * NL and m2 == [digit] * NL
    assert ST.q_ext == {digit}
    assert ST.max_d < BOUND


def test_chain_of_128_products():
    """the encryption's loop: the first entry, then 127 products by entries below 2 n; the pair stays inside 0.51 n and is the
    product of the entries in CPython"""
    n = bench_n()
    n2 = n * n
    rng = random.Random(9)
    Ri = pow(R, -1, n2)
    first = rng.randrange(2 * n)
    a, b = km.balance_halves(km.limbs(first, NL)), [0] * NL
    acc = first % n2                          # a + b n == acc (mod n^2)
    for _ in range(127):
        cv = rng.randrange(2 * n)
        a, b, _, _ = product(a, b, km.balance_halves(km.limbs(cv, NL)), n)
        acc = acc * cv * Ri % n2
        assert km.in_lazy_range(a, n) and km.in_lazy_range(b, n)
        assert (km.value(a) + km.value(b) * n - acc) % n2 == 0
    # the exit's pair: (a + n, b - 1 + n), limbs in [0, 2^29)
    nb = km.bal_limbs(n, NL)
    ua, ub = km.from_balanced_plus_p(a, nb, 0), km.from_balanced_plus_p(b, nb, 1)
    assert (km.value(ua) + km.value(ub) * n - acc) % n2 == 0
    assert ST.max_d < BOUND


def test_balanced_conversions():
    n = bench_n()
    nb = km.bal_limbs(n, NL)
    rng = random.Random(11)
    for x in [0, 1, n - 1, 2 * n + (n >> 18) - 1, km.value([km.MASK] * (NL - 3)), km.value([HB] * (NL - 3)), km.value([HB - 1] * (NL - 3))] + \
            [rng.randrange(2 * n) for _ in range(20)]:
        r = km.balance_halves(km.limbs(x, NL))
        assert km.value(r) == x and all(LO <= d <= HI for d in r[:-1]) and r == km.bal_limbs(x, NL)
    for x in [0, 1, -1, 51 * n // 100, -(51 * n // 100)] + [rng.randrange(-n // 2, n // 2) for _ in range(20)]:
        for less in (0, 1):
            u = km.from_balanced_plus_p(km.bal_limbs(x, NL), nb, less)
            assert km.value(u) == x + n - less and all(0 <= d < B for d in u)


def test_multiply_adds_per_step():
    """3 906 for the four Karatsuba products and the collapse, 18 for the digits that enter the column and the stored sum
    separately; the one body of all four steps adds 72 for the carried-in digits and 36 for - q of the first quotient"""
    n = bench_n()
    nm, n0inv = km._bal_ctx(n, NL)
    x, ch = [1] * NL, [1] * HL
    st = km.Kara2Stats()
    km.kara2_step_bal(x, ch, None, None, nm, n0inv, st, False, False)
    assert st.macs == 4 * 3 * H * H + H + H + NL + HL == 3906 + 18 + 108
    km.kara2_step_bal(x, ch, x, ch, nm, n0inv, st, True, True)
    assert st.macs == 3906 + 18 + 108


def test_largest_column_of_the_file():
    """runs last: the record over every family above (alone: over the extreme limbs)"""
    if ST.max_d == 0:
        test_limbs_at_the_extremes()
    print({"kara2_max_col_log2": round(math.log2(ST.max_d), 3), "at": ST.at_d, "max_carry_log2": round(math.log2(ST.max_c), 3)})
    assert 2 ** 62 < ST.max_d < BOUND
    assert ST.max_c < 1 << 34
