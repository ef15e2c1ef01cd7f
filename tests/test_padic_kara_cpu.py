"""CPU: the cell-exact model of the register-resident Karatsuba squaring of the digit-pair engine (csrc/mont_padic.hpp:
kara_pass / sqr_kara, tools/kara_model.py).  At 36 limbs (1024- and 1000-bit primes) and 24 limbs, with all limbs 2^29 - 1,
digits at the lazy bound 2p + eps, every difference limb at +-(2^29 - 1) with opposite signs in the two operands, and random
digits: no 64-bit cell wraps, the product columns are exact, and both passes give the exact w, v of the product rule, i.e.
the digit form of CPython's pow(x, 2, p^2).  (The kernel itself is held to the oracle on the GPU:
tests/test_gpu_padic_kara.py.)"""
import importlib.util
from pathlib import Path


def _model():
    spec = importlib.util.spec_from_file_location("kara_model", Path(__file__).resolve().parent.parent / "tools" / "kara_model.py")
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    return km


def test_kara_squaring_model_bounds_and_result():
    km = _model()
    st = km.run(rounds=1, seed=11)
    assert st.max_col < 1 << 64 and st.max_cc < 1 << 64 and st.max_d < 1 << 64


def test_kara_squaring_model_extreme_limbs():
    km = _model()
    NL = 36
    p = km.random_prime(1024, __import__("random").Random(2))
    R = 1 << (km.RB * NL)
    st = km.Stats()
    # all limbs 2^29 - 1: the largest product column (36 (2^29 - 1)^2 < 2^63.2) and the largest carries
    km.sqr_kara(R - 1, R - 1, p, NL, st, in_range=False)
    assert st.max_col == NL * km.MASK * km.MASK
    # opposite-sign differences in the two operands of 2 a b
    H = NL // 2
    x = km.value([km.MASK] * H + [0] * H)
    y = km.value([0] * H + [km.MASK] * H)
    km.sqr_kara(x, y, p, NL, st, in_range=False)
    km.sqr_kara(y, x, p, NL, st, in_range=False)
    # the digit form of pow(x, 2, p^2) at the lazy bound
    top = 2 * p + (p >> 18) - 1
    w, v = km.sqr_kara(top, top, p, NL, st)
    x = (top + top * p) % (p * p)
    assert (w + v * p) % (p * p) == pow(x, 2, p * p) * pow(R, -1, p * p) % (p * p)


def test_kara_squaring_model_extreme_primes():
    """The same corners with the modulus at the extremes (tests/golden/extreme_keys.json: limbs all ones, all zero, low half ones /
    high half zero, = 1 and = -1 modulo 2^58) on 36 limbs (1024-bit primes) and 24 limbs (512 bits, and 676 bits: the widest prime
    the geometry admits, R / p = 2^20 exactly); a run of squarings stays inside the lazy bound."""
    import random

    from tests.test_extreme_keys_cpu import load_extreme_keys

    km = _model()
    rng = random.Random(3)
    st = km.Stats()
    for bits, NL in ((1024, 36), (512, 24), (676, 24)):
        for p in sorted({v for _, _, b, p_, q_ in load_extreme_keys() if b == bits for v in (p_, q_)}):
            for a, b, ok in km.corners(p, NL, rng):
                km.sqr_kara(a, b, p, NL, st, in_range=ok)
            a, b = 2 * p - 1, 2 * p - 1
            for _ in range(4):
                a, b = km.sqr_kara(a, b, p, NL, st)
                assert a < 2 * p + (p >> 18) and b < 2 * p + (p >> 18)
    assert st.max_col < 1 << 64 and st.max_cc < 1 << 64 and st.max_d < 1 << 64
