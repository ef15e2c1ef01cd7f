"""CPU: the cell-exact model of the balanced-digit passes with ONE stored sum per column (csrc/mont_padic.hpp: kara_pass_bal
with ONES, kernel mode PADIC_LDS_KMRBS; tools/kara_model.py: kara_pass_bal(ones=...), KMRBS_RED) against the model of the
two-sum form (KMRB_RED), on the operand families of tests/test_padic_balanced_cpu.py.

S_k = [2] V_k + U_k replaces V_k and U_k in the passes that have both Karatsuba quotient products and the one-chain product
stream: both passes of a squaring and the first pass of a product.  The model runs those passes in 64-bit cells that wrap and
asserts at every column that the finished column, read as a signed 64-bit integer, is the schoolbook column and |d| < 2^63 (so
S_k is needed modulo 2^64 only), that out and mq are in [-2^28, 2^28) and that the carry is exact.  Here every pass must give
out, mq and hence every carry (out's top limb is the last one; a differing carry changes the next digit) identical to the
two-sum form, in both placements of the newest quotient digit's terms (ONES2):
  - all limbs at -2^28 and all limbs at 2^28 - 1, operands and modulus,
  - second passes with every product of a column of one sign and quotient digits solved to all -2^28 / all 2^28 - 1,
  - first passes solved for quotient digits at the extremes (and at opposite extremes in the two halves),
  - the structured moduli of tests/golden/extreme_keys.json and of tests/test_padic_kred_cpu.py,
  - the lazy bound |a| = floor(0.51 s), a 768-bit prime on 36 limbs,
  - a chain of 200 mixed squarings and products against CPython modulo s^2.
(The kernel itself is held to the oracle on the GPU: tests/test_gpu_padic_onesum.py.)"""
import random

from tests.test_padic_balanced_cpu import HB, HI, LO, NL, H, R, centered, n0inv_of
from tests.test_padic_kara_mul_cpu import extreme_primes
from tests.test_padic_kred_cpu import _sqrt_mod_2n, km, structured_moduli

PLACEMENTS = (1, 2)                                        # the newest digit's terms onto S_k once / onto S_k and the column
ONE_SUM_REDS = (km.KMRBS_RED, km.KMRBS_RED | km.ONES2)
ONE_SUM_FORMS = (km.SQR, km.SQR2, km.MUL)                  # the sum of two products (MUL2) keeps its form


def test_masks():
    assert km.KMRBS_RED == km.KMRB_RED | km.ONES and not km.KMRB_RED & (km.ONES | km.ONES2)
    assert [km.red_ones(r) for r in (km.KMRB_RED, km.KMRBS_RED, km.KMRBS_RED | km.ONES2)] == [0, 1, 2]


def same_pass(form, x, y, mnin, nm, st):
    """The pass in the two-sum form and in both one-sum placements: identical out (top limb = last carry) and mq."""
    n0inv = n0inv_of(nm)
    yy = x if form == km.SQR else y
    ref = km.kara_pass_bal(form, x, yy, mnin, nm, n0inv, st, kred=True, vf=True)
    for ones in PLACEMENTS:
        got = km.kara_pass_bal(form, x, yy, mnin, nm, n0inv, st, kred=True, vf=True, ones=ones)
        assert got == ref, (form, ones)
    return ref


def test_switch_is_inert_where_the_pass_keeps_its_form():
    """ones leaves MUL2 and every pass without kred or vf as it is (the kernel's `ONES != 0 && KRED && VF && !SUM`)."""
    st = km.BalStats()
    n0inv = n0inv_of(HI)
    for form, kred, vf in ((km.MUL2, True, True), (km.MUL2, False, True), (km.SQR, False, True), (km.SQR2, True, False)):
        ref = km.kara_pass_bal(form, LO, HI, LO, HI, n0inv, st, x2=HI, y2=LO, kred=kred, vf=vf)
        macs = st.red_macs
        for ones in PLACEMENTS:
            assert km.kara_pass_bal(form, LO, HI, LO, HI, n0inv, st, x2=HI, y2=LO, kred=kred, vf=vf, ones=ones) == ref
            assert st.red_macs == macs


def test_all_limbs_at_the_extremes():
    st = km.BalStats()
    odd_lo = [-HB + 1] + [-HB] * (NL - 1)                  # a modulus must be odd
    for nm in (HI, odd_lo):
        for x in (LO, HI):
            for y in (LO, HI):
                for mnin in (x, y):
                    for form in ONE_SUM_FORMS:
                        same_pass(form, x, y, mnin, nm, st)
    assert st.max_d < 1 << 63
    # quotient multiply-adds: those of the two-sum form (990) and m[k] p[0] onto both S_k and the column for k < H, where the
    # two-sum form adds the finished U_k to the column; one more per column 1 .. NL where the newest digit's term is added twice
    n0inv = n0inv_of(HI)
    km.kara_pass_bal(km.SQR, LO, LO, LO, HI, n0inv, st, kred=True, vf=True, ones=1)
    assert st.red_macs == 3 * H * H + H + H == 1008
    km.kara_pass_bal(km.SQR, LO, LO, LO, HI, n0inv, st, kred=True, vf=True, ones=2)
    assert st.red_macs == 1008 + NL


def test_second_pass_columns_of_one_sign():
    """2 a b with every limb product of one sign and the quotient digits all at one extreme: the largest column of the doubled
    pass, 36 (2^57 + 2^56) (1 - eps); the cells that hold S_k wrap, the finished column must not."""
    nm = HI
    p = km.value(nm)
    worst = 0
    for x, y, T in ((LO, HI, LO), (LO, LO, HI), (HI, HI, HI), (HI, LO, LO)):
        Tv = km.value(T)
        prod = 2 * km.value(x) * km.value(y)
        m_in = centered(prod + Tv * p)
        st = km.BalStats()
        out, mq = same_pass(km.SQR2, x, y, m_in, nm, st)
        assert mq == T
        assert km.value(out) * R == prod - km.value(m_in) + Tv * p
        worst = max(worst, st.max_d)
    assert 0.999 * (NL * 3 << 56) < worst < 1 << 63


def test_first_pass_quotient_digits_at_the_extremes():
    rng = random.Random(41)
    nbits = km.RB * NL
    mods = dict(structured_moduli())
    mods["random"] = rng.getrandbits(nbits - 21) | (1 << (nbits - 22)) | 1
    mods["one_mod_8"] = (rng.getrandbits(nbits - 21) | (1 << (nbits - 22))) & ~7 | 1
    targets = (LO, HI, [-HB] * H + [HB - 1] * H, [HB - 1] * H + [-HB] * H)
    one = km.bal_limbs(1, NL)
    squares = 0
    for name, p in mods.items():
        nm = km.bal_limbs(p, NL)
        for T in targets:
            Tv = km.value(T)
            st = km.BalStats()
            a = centered(-Tv * p)                                       # KARA_MUL: a * 1 == -T p
            w, m = same_pass(km.MUL, a, one, [0] * NL, nm, st)
            assert m == T and km.value(w) * R == km.value(a) + Tv * p
            if p % 8 == 1 and T == LO:
                S = -Tv >> 28                                           # KARA_SQR: a^2 == -T p = 2^28 S p, S == 1 modulo 8
                a = centered(_sqrt_mod_2n(S * p % (1 << (nbits - 28)), nbits - 28) << 14)
                w, m = same_pass(km.SQR, a, a, [0] * NL, nm, st)
                assert m == T and km.value(w) * R == km.value(a) ** 2 + Tv * p
                squares += 1
    assert squares >= 2


def test_structured_moduli_and_lazy_bound():
    rng = random.Random(42)
    st = km.BalStats()
    primes = extreme_primes(1024) + [km.random_prime(1024, rng), km.random_prime(768, rng)]
    for p in primes:
        top = 51 * p // 100                                             # |a| = floor(0.51 s)
        ops = [km.bal_limbs(v, NL) for v in (top, -top, 0, 1, -1, p // 2, rng.randrange(-top, top + 1))]
        for i, a in enumerate(ops):
            b, c, d = ops[(i + 1) % len(ops)], ops[(i + 2) % len(ops)], ops[(i + 4) % len(ops)]
            sq, mu = km.sqr_kara_bal(a, b, p, st, km.KMRB_RED), km.mul_kara_bal(a, b, c, d, p, st, km.KMRB_RED)
            for red in ONE_SUM_REDS:
                assert km.sqr_kara_bal(a, b, p, st, red) == sq
                assert km.mul_kara_bal(a, b, c, d, p, st, red) == mu
            for w, v in (sq, mu):
                assert km.in_lazy_range(w, p) and km.in_lazy_range(v, p)
    # moduli that are no primes and leave no headroom (R / p < 2^20): cells only
    for p in structured_moduli().values():
        nm = km.bal_limbs(p, NL)
        for x in (LO, HI, centered(rng.randrange(R))):
            mnin = centered(rng.randrange(R))
            for form in ONE_SUM_FORMS:
                same_pass(form, x, HI, mnin, nm, st)
                same_pass(form, x, LO, mnin, nm, st)
    assert st.max_d < 1 << 63


def test_chain_of_200_against_pow():
    """200 mixed squarings and products: every step's pair is that of the two-sum form, limb for limb, in both placements, and
    the represented residue is CPython's."""
    rng = random.Random(43)
    for bits, unit in ((1024, True), (768, True), (1024, False)):
        p = km.random_prime(bits, rng)
        p2 = p * p
        Rinv = pow(R, -1, p2)
        x = rng.randrange(p2) if unit else p * rng.randrange(1, p)
        y = rng.randrange(p2)
        xr, yr = x * R % p2, y * R % p2
        a, b = km.to_balanced(km.limbs(xr % p, NL)), km.to_balanced(km.limbs(xr // p, NL))
        c, d = km.to_balanced(km.limbs(yr % p, NL)), km.to_balanced(km.limbs(yr // p, NL))
        st = km.BalStats()
        want = x
        for step in range(200):
            if rng.random() < 0.7:
                ref = km.sqr_kara_bal(a, b, p, st, km.KMRB_RED)
                for red in ONE_SUM_REDS:
                    assert km.sqr_kara_bal(a, b, p, st, red) == ref, step
                want = want * want % p2
            else:
                ref = km.mul_kara_bal(a, b, c, d, p, st, km.KMRB_RED)
                for red in ONE_SUM_REDS:
                    assert km.mul_kara_bal(a, b, c, d, p, st, red) == ref, step
                want = want * y % p2
            a, b = ref
            assert km.in_lazy_range(a, p) and km.in_lazy_range(b, p)
        assert (km.value(a) + km.value(b) * p) * Rinv % p2 == want
        assert st.max_d < 1 << 63
