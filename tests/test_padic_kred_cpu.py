"""CPU: the cell-exact model of the Montgomery reductions with their quotient products m p by Karatsuba columns
(csrc/mont_padic.hpp: kara_pass<FORM, true>; tools/kara_model.py: kara_pass(..., kred=True)), all four forms at 36 limbs,
with the product streams as they were and in the one-chain form the kernel mode PADIC_LDS_KMR pairs them with (vf=True).
The model asserts every 64-bit cell (the stored half products rq0 / rq2, every signed product and partial sum of -E, the
reduction column d) and that quotient digits, out and carry are those of the schoolbook column rule; here its w, v are held
to the row-wise product rule on Python integers and to CPython's pow, at
  - all limbs 2^29 - 1 in both operands and the modulus,
  - moduli whose halves sit at opposite extremes (every difference p[H + l] - p[l] at -(2^29 - 1) resp. +(2^29 - 1)) and a
    modulus with equal halves (every difference zero),
  - operands at the lazy bound 2p + eps,
  - inputs chosen so that the quotient digits come out all ones in one half and zero in the other: mq[i] - mq[H + i] at
    +(2^29 - 1) and at -(2^29 - 1) in every limb, for each of the four forms.
(The kernel itself is held to the oracle on the GPU: tests/test_gpu_padic_kred.py.)"""
import importlib.util
import random
from pathlib import Path

NL = 36
H = NL // 2
ALL = 15          # every form of kara_pass reduces by Karatsuba columns


def _model():
    spec = importlib.util.spec_from_file_location("kara_model", Path(__file__).resolve().parent.parent / "tools" / "kara_model.py")
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    return km


km = _model()
MASKS = (ALL, ALL | km.VF | km.VFM, km.KMR_RED)       # ... with the schoolbook-free product streams too; what the kernel runs
R = 1 << (km.RB * NL)
MASK = km.MASK


def rowwise_mul(a, b, c, d, p):
    pinv = pow(p, -1, R)
    m = (-a * c * pinv) % R
    w, r = divmod(a * c + m * p, R)
    assert r == 0
    s = a * d + b * c - m + R * p
    m2 = (-s * pinv) % R
    v, r = divmod(s + m2 * p, R)
    assert r == 0
    return w, v, m, m2


def both(a, b, c, d, p, st, in_range):
    """Product and (for c, d = a, b) squaring with every reduction by Karatsuba columns, against the row-wise rule."""
    w, v, _, _ = rowwise_mul(a, b, c, d, p)
    ws, vs, _, _ = rowwise_mul(a, b, a, b, p)
    assert km.mul_kara(a, b, c, d, p, NL, st, in_range=in_range, red=0) == (w, v)
    for red in MASKS:
        assert km.mul_kara(a, b, c, d, p, NL, st, in_range=in_range, red=red) == (w, v)
        assert km.sqr_kara(a, b, p, NL, st, in_range=in_range, red=red) == (ws, vs)
    if in_range:
        p2 = p * p
        assert (ws + vs * p) % p2 == pow(a + b * p, 2, p2) * pow(R, -1, p2) % p2
        assert (w + v * p) % p2 == (a + b * p) * (c + d * p) * pow(R, -1, p2) % p2


def structured_moduli():
    top = 1 << (km.RB - 1)
    return {
        "all_ones": km.value([MASK] * NL),
        "low_ones_high_1000": km.value([MASK] * H + [0] * (H - 1) + [top]),      # p[H + l] - p[l] = -(2^29 - 1) but the top
        "low_0001_high_ones": km.value([1] + [0] * (H - 1) + [MASK] * H),        # ... = +(2^29 - 1) but the lowest
        "equal_halves": km.value(([MASK - 2] + [0x0ABCDEF] * (H - 2) + [top]) * 2),   # every difference zero
    }


def test_counts_and_cell_bounds_all_ones():
    p = structured_moduli()["all_ones"]
    st = km.Stats()
    x = R - 1
    both(x, x, x, x, p, st, in_range=False)
    al = km.limbs(x, NL)
    nm = km.limbs(p, NL)
    n0inv = (-pow(p, -1, km.B)) % km.B
    for form in (km.SQR, km.SQR2, km.MUL, km.MUL2):
        for vf in (False, True) if form != km.MUL2 else (False,):
            km.kara_pass(form, al, al, al, nm, n0inv, st, x2=al, y2=al, kred=True, vf=vf)
            assert st.red_macs == 3 * H * H + H == 990
        km.kara_pass(form, al, al, al, nm, n0inv, st, x2=al, y2=al, kred=False)
        assert st.red_macs == NL * NL == 1296
    assert st.max_rq <= H * MASK * MASK < 1 << 63
    assert st.max_red_e <= H * MASK * MASK < 1 << 63
    assert st.max_d < 1 << 64 and st.max_cc < 1 << 64


def test_structured_moduli_extreme_operands():
    rng = random.Random(21)
    lo_hi = km.value([MASK] * H + [0] * H)
    hi_lo = km.value([0] * H + [MASK] * H)
    st = km.Stats()
    for name, p in structured_moduli().items():
        assert p % 2 == 1
        ops = [R - 1, lo_hi, hi_lo, 1, 0] + [rng.randrange(R) for _ in range(2)]
        for i, a in enumerate(ops):
            b, c, d = ops[(i + 1) % len(ops)], ops[(i + 2) % len(ops)], ops[(i + 3) % len(ops)]
            both(a, b, c, d, p, st, in_range=False)
    assert st.max_rq < 1 << 63 and st.max_red_e < 1 << 63 and st.max_d < 1 << 64
    assert st.dm_signs == {-1, 0, 1}


def test_lazy_bound_operands():
    from tests.test_padic_kara_mul_cpu import extreme_primes

    rng = random.Random(22)
    st = km.Stats()
    for p in [km.random_prime(bits, rng) for bits in (1024, 1000, 768)] + extreme_primes(1024):
        top = 2 * p + (p >> 18) - 1
        for a, b, c, d in ((top, top, top, top), (top, 0, 0, top), (0, top, top, 0), (p - 1, p - 1, p + 1, top),
                           tuple(rng.randrange(top + 1) for _ in range(4))):
            both(a, b, c, d, p, st, in_range=True)
            w, v, _, _ = rowwise_mul(a, b, c, d, p)
            assert w <= top and v <= top
    assert st.max_rq < 1 << 63 and st.max_red_e < 1 << 63 and st.max_d < 1 << 64


def _sqrt_mod_2n(v, n):
    """A square root of v (== 1 mod 8) modulo 2^n."""
    assert v % 8 == 1
    r = 1
    for bits in range(3, n):
        if (r * r - v) >> bits & 1:
            r += 1 << (bits - 1)
    assert (r * r - v) % (1 << n) == 0
    return r


def test_quotient_digits_all_ones_in_one_half():
    """Inputs solved for the quotient digits T = (ones, zero) and (zero, ones): every mq[i] - mq[H + i] is +(2^29 - 1)
    resp. -(2^29 - 1) while the modulus differences are at their extremes too.  m = -x y / p mod R for the first passes,
    m' = -(.. - m) / p mod R for the second ones."""
    rng = random.Random(23)
    nbits = km.RB * NL
    targets = {+1: km.value([MASK] * H + [0] * H), -1: km.value([0] * H + [MASK] * H)}
    mods = dict(structured_moduli())
    mods["random"] = rng.getrandbits(nbits - 21) | (1 << (nbits - 22)) | 1
    mods["one_mod_8"] = (rng.getrandbits(nbits - 21) | (1 << (nbits - 22))) & ~7 | 1
    for name, p in mods.items():
        pinv = pow(p, -1, R)
        nm = km.limbs(p, NL)
        n0inv = (-pow(p, -1, km.B)) % km.B
        for sign, T in targets.items():
            st = km.Stats()
            # KARA_MUL: a * 1 == -T p
            a = (-T * p) % R
            w, m = km.kara_pass(km.MUL, km.limbs(a, NL), km.limbs(1, NL), [0] * NL, nm, n0inv, st, kred=True)
            assert km.value(m) == T and km.value(w) == (a + T * p) // R
            assert st.dm_signs == {sign}
            # KARA_MUL2: a' * 0 + b * 1 - m + R p == -T p  with the m of some first pass
            m_in = rng.randrange(R)
            b = (m_in - T * p) % R
            st = km.Stats()
            v, m2 = km.kara_pass(km.MUL2, km.limbs(a, NL), [0] * NL, km.limbs(m_in, NL), nm, n0inv, st,
                                 x2=km.limbs(b, NL), y2=km.limbs(1, NL), kred=True)
            assert km.value(m2) == T and km.value(v) * R == b - m_in + R * p + T * p
            assert st.dm_signs == {sign}
            # KARA_SQR2: 2 a b - m + R p == -T p:  a odd, m of the parity of T p
            a = rng.randrange(R) | 1
            m_in = rng.randrange(R) & ~1 | (T * p & 1)
            b = ((m_in - T * p) // 2 * pow(a, -1, R)) % (R // 2)
            st = km.Stats()
            v, m2 = km.kara_pass(km.SQR2, km.limbs(a, NL), km.limbs(b, NL), km.limbs(m_in, NL), nm, n0inv, st, kred=True)
            assert km.value(m2) == T and km.value(v) * R == 2 * a * b - m_in + R * p + T * p
            assert st.dm_signs == {sign}
            # KARA_SQR: a^2 == -T p needs -T' p == 1 mod 8 (T' = T without its factor 2^(29 H)): T' == 7, so p == 1 mod 8
            if p % 8 == 1:
                sh = 0 if T & 1 else km.RB * H
                assert sh % 2 == 0
                a = _sqrt_mod_2n((-(T >> sh) * p) % (1 << (nbits - sh)), nbits - sh) << (sh // 2)
                assert (a * a + T * p) % R == 0
                st = km.Stats()
                al = km.limbs(a % R, NL)
                w, m = km.kara_pass(km.SQR, al, al, [0] * NL, nm, n0inv, st, kred=True)
                assert km.value(m) == T and km.value(w) * R == km.value(al) ** 2 + T * p
                assert st.dm_signs == {sign}
    assert any(p % 8 == 1 for p in mods.values())


def test_random_runs_match_pow():
    """Runs of squarings and products with every reduction by Karatsuba columns stay inside the lazy bound and give
    x^e in digit form."""
    rng = random.Random(24)
    st = km.Stats()
    for bits in (1024, 768):
        p = km.random_prime(bits, rng)
        p2 = p * p
        Rinv = pow(R, -1, p2)
        x = rng.randrange(p2)
        xr = x * R % p2
        a, b = xr % p, xr // p
        c, d = a, b
        e = 1
        for step in range(6):
            a, b = km.sqr_kara(a, b, p, NL, st, red=km.KMR_RED)
            e *= 2
            if step % 2:
                a, b = km.mul_kara(a, b, c, d, p, NL, st, red=km.KMR_RED)
                e += 1
            assert a < 2 * p + (p >> 18) and b < 2 * p + (p >> 18)
        assert (a + b * p) * Rinv % p2 == pow(x, e, p2)
