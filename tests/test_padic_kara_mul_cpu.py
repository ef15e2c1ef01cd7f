"""CPU: the cell-exact model of the register-resident Karatsuba PRODUCT of the digit-pair engine (csrc/mont_padic.hpp:
kara_pass<KARA_MUL> / <KARA_MUL2>, mul_kara_reg; tools/kara_model.py: mul_kara).  At 36 limbs with all limbs 2^29 - 1 in
all four operands, digits at the lazy bound 2p + eps, difference limbs at +-(2^29 - 1) with opposite signs in both
operands, and seeded random pairs: no 64-bit cell wraps (kara_model asserts every cell), and both passes give exactly the
w, v of the row-wise product rule  w = (a c + m p) / R,  v = (a d + b c - m + R p + m' p) / R  on Python integers.  (The
kernel itself is held to the oracle on the GPU: tests/test_gpu_padic_kara_mul.py.)"""
import importlib.util
import random
from pathlib import Path

NL = 36


def extreme_primes(bits):
    """The structured primes of tests/golden/extreme_keys.json at one width: limbs all ones, all zero, low half ones / high half zero,
    and = 1 / = -1 modulo 2^58 (quotient digits t * n0inv with n0inv = 2^29 - 1 / 1)."""
    from tests.test_extreme_keys_cpu import load_extreme_keys

    out = sorted({v for _, _, b, p, q in load_extreme_keys() if b == bits for v in (p, q)})
    assert len(out) == 8
    return out


def _model():
    spec = importlib.util.spec_from_file_location("kara_model", Path(__file__).resolve().parent.parent / "tools" / "kara_model.py")
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    return km


def _rowwise(km, a, b, c, d, p):
    """The product rule as Padic::mul computes it: the unique quotients modulo R, then exact divisions."""
    R = 1 << (km.RB * NL)
    pinv = pow(p, -1, R)
    m = (-a * c * pinv) % R
    w, r = divmod(a * c + m * p, R)
    assert r == 0
    s = a * d + b * c - m + R * p
    m2 = (-s * pinv) % R
    v, r = divmod(s + m2 * p, R)
    assert r == 0
    return w, v


def test_kara_product_all_ones_limbs():
    km = _model()
    p = km.random_prime(1024, random.Random(5))
    R = 1 << (km.RB * NL)
    st = km.Stats()
    x = R - 1
    assert km.mul_kara(x, x, x, x, p, NL, st, in_range=False) == _rowwise(km, x, x, x, x, p)
    # the largest cells: a column of one product, the summed half products of two, the 128-bit middle cell of two
    assert st.max_col == NL * km.MASK * km.MASK < 1 << 64
    assert st.max_cc < 1 << 64 and st.max_d < 1 << 64
    assert 1 << 64 <= st.max_e < 1 << 66          # the sum of two product columns does pass 2^64: hence the wide cell


def test_kara_product_lazy_bound():
    km = _model()
    rng = random.Random(6)
    for p in [km.random_prime(bits, rng) for bits in (1024, 1000)] + extreme_primes(1024):
        top = 2 * p + (p >> 18) - 1
        st = km.Stats()
        for a, b, c, d in ((top, top, top, top), (top, 0, 0, top), (0, top, top, 0), (top, top, 1, 0), (p - 1, p - 1, p - 1, p - 1)):
            w, v = km.mul_kara(a, b, c, d, p, NL, st)
            assert (w, v) == _rowwise(km, a, b, c, d, p)
            assert w < top + 1 and v < top + 1          # the lazy bound holds for the next operation


def test_kara_product_opposite_sign_differences():
    km = _model()
    p = km.random_prime(1024, random.Random(7))
    H = NL // 2
    lo_hi = km.value([km.MASK] * H + [0] * H)           # x0 all ones, x1 zero: every difference +(2^29 - 1)
    hi_lo = km.value([0] * H + [km.MASK] * H)           # every difference -(2^29 - 1)
    alt = km.value([km.MASK if (i // H + i) % 2 else 0 for i in range(NL)])
    full = (1 << (km.RB * NL)) - 1
    st = km.Stats()
    ops = [lo_hi, hi_lo, alt, full - alt]
    for a in ops:
        for b in (lo_hi, hi_lo):
            for c in ops:
                for d in (hi_lo, lo_hi):
                    got = km.mul_kara(a, b, c, d, p, NL, st, in_range=False)
                    assert got == _rowwise(km, a, b, c, d, p)
    # ... and with the modulus itself at those extremes (one operand of every reduction column is p)
    for p in extreme_primes(1024):
        for a, b, c, d in ((lo_hi, hi_lo, hi_lo, lo_hi), (hi_lo, lo_hi, alt, full - alt), (full, full, full, full)):
            assert km.mul_kara(a, b, c, d, p, NL, st, in_range=False) == _rowwise(km, a, b, c, d, p)
    assert st.max_cc < 1 << 64 and st.max_d < 1 << 64


def test_kara_product_random_pairs():
    km = _model()
    rng = random.Random(8)
    st = km.Stats()
    for p in [km.random_prime(bits, rng) for bits in (1024, 1000)] + extreme_primes(1024):
        top = 2 * p + (p >> 18)
        for _ in range(12):
            a, b, c, d = (rng.randrange(top) for _ in range(4))
            assert km.mul_kara(a, b, c, d, p, NL, st) == _rowwise(km, a, b, c, d, p)
    assert st.max_col < 1 << 64 and st.max_cc < 1 << 64 and st.max_d < 1 << 64
