"""CPU: the cell-exact model of the balanced-digit passes (csrc/mont_padic.hpp: kara_pass_bal, sqr_kara_reg_bal,
mul_kara_reg_bal, kernel mode PADIC_LDS_KMRB; tools/kara_model.py: kara_pass_bal) at the operands where a cell can overflow,
and the entry / exit conversions of the kernel (to_balanced, from_balanced_plus_p).

The model asserts at every column of every pass that the finished column d is the schoolbook column and |d| < 2^63, that the
stored sums U_k, V_k and the partial sums of -D, -E are within their bounds, and that out and mq are in [-2^28, 2^28); its
callers assert w R = x y + m p and v R = a d + b c - m + m' p on the represented integers.  Here:
  - all limbs at -2^28 and all limbs at 2^28 - 1, operands and modulus, all four forms and every reduction / stream form,
  - second passes with EVERY product of a column of the same sign in both streams: operands at the extremes, quotient digits
    forced to all -2^28 (or all 2^28 - 1) by solving for the incoming m — the largest column the engine can meet,
    36 (2^57 + 2^56) (1 - eps),
  - first passes solved for quotient digits all at -2^28 (and at opposite extremes in the two halves),
  - the structured moduli of tests/golden/extreme_keys.json (all-ones and all-zero limbs, halves at opposite extremes) and
    of tests/test_padic_kred_cpu.py (equal halves),
  - the lazy bound |a| = floor(0.51 s), a 768-bit prime on 36 limbs,
  - a chain of 200 random squarings and products against CPython modulo s^2, with the unsigned engine's exit beside it,
  - round trips of the entry and exit conversions at 0, 1, s - 1, s, s + 1 and 2s - 1 in either digit.
(The kernel itself is held to the oracle on the GPU: tests/test_gpu_padic_balanced.py.)"""
import random

from tests.test_padic_kara_mul_cpu import extreme_primes
from tests.test_padic_kred_cpu import _sqrt_mod_2n, km, structured_moduli

NL = 36
H = NL // 2
R = 1 << (km.RB * NL)
HB = km.HB
FORMS = (km.SQR, km.SQR2, km.MUL, km.MUL2)
REDS = (0, 15, 15 | km.VF | km.VFM | km.VFS, km.KMRB_RED)
LO, HI = [-HB] * NL, [HB - 1] * NL


def centered(x):
    """The representative of x modulo R in [-R/2, R/2) ... as balanced limbs (all NL digits in range)."""
    l = km.bal_limbs(x % R, NL)
    l[-1] = km.sfield(l[-1])
    return l


def n0inv_of(nm):
    return (-pow(km.value(nm), -1, km.B)) % km.B


def every_form(x, y, x2, y2, mnin, nm, st):
    """All four passes in every reduction / stream form on the same limb lists; the exact relations of each."""
    n0inv = n0inv_of(nm)
    p = km.value(nm)
    for form in FORMS:
        outs = set()
        for kred in (False, True):
            for vf in (False, True):
                yy = x if form == km.SQR else y
                out, mq = km.kara_pass_bal(form, x, yy, mnin, nm, n0inv, st, x2=x2, y2=y2, kred=kred, vf=vf)
                X, Y = km.value(x), km.value(yy)
                lhs = {km.SQR: X * X, km.SQR2: 2 * X * Y - km.value(mnin), km.MUL: X * Y,
                       km.MUL2: X * Y + km.value(x2) * km.value(y2) - km.value(mnin)}[form]
                assert km.value(out) * R == lhs + km.value(mq) * p
                outs.add((tuple(out), tuple(mq)))
        assert len(outs) == 1                              # the forms agree digit for digit


def test_all_limbs_at_the_extremes():
    st = km.BalStats()
    odd_lo = [-HB + 1] + [-HB] * (NL - 1)                  # a modulus must be odd
    for nm in (HI, odd_lo):
        for x in (LO, HI):
            for y in (LO, HI):
                every_form(x, y, y, x, x, nm, st)
                every_form(x, y, x, y, y, nm, st)
    assert st.max_d < 1 << 63 and st.max_v <= 2 * H << 56 and st.max_u <= H << 56
    n0inv = n0inv_of(HI)
    km.kara_pass_bal(km.SQR, LO, LO, LO, HI, n0inv, st, kred=True, vf=True)
    assert st.red_macs == 3 * H * H + H == 990
    km.kara_pass_bal(km.SQR, LO, LO, LO, HI, n0inv, st, kred=False, vf=True)
    assert st.red_macs == NL * NL == 1296


def test_second_pass_columns_of_one_sign():
    """2 a b resp. a d + b c with every limb product of one sign, the quotient digits all at one extreme and of the sign that
    makes every quotient product agree with them: m_in = (the products) + T p modulo R is just another balanced number."""
    nm = HI
    p = km.value(nm)
    n0inv = n0inv_of(nm)
    worst = 0
    for x, y, T in ((LO, HI, LO), (LO, LO, HI), (HI, HI, HI), (HI, LO, LO)):
        Tv = km.value(T)
        for form, kred, vf in ((km.SQR2, True, True), (km.SQR2, False, False), (km.MUL2, False, False), (km.MUL2, True, True)):
            st = km.BalStats()
            X, Y = km.value(x), km.value(y)
            prod = 2 * X * Y
            m_in = centered(prod + Tv * p)
            out, mq = km.kara_pass_bal(form, x, y, m_in, nm, n0inv, st, x2=y, y2=x, kred=kred, vf=vf)
            assert mq == T
            assert km.value(out) * R == prod - km.value(m_in) + Tv * p
            worst = max(worst, st.max_d)
    # 36 (2^57 + 2^56) = 2^62.75 less the rounding of 2^28 - 1: reached to within a thousandth, and inside the cell
    assert 0.999 * (NL * 3 << 56) < worst < 1 << 63


def test_first_pass_quotient_digits_at_the_extremes():
    """Operands solved for the quotient digits T = all -2^28, all 2^28 - 1 and the two halves at opposite extremes (every
    mq[i] - mq[H + i] at +-(2^29 - 1)), on the structured moduli and a prime = 1 modulo 8 (KARA_SQR needs a square)."""
    rng = random.Random(31)
    nbits = km.RB * NL
    mods = dict(structured_moduli())
    mods["random"] = rng.getrandbits(nbits - 21) | (1 << (nbits - 22)) | 1
    mods["one_mod_8"] = (rng.getrandbits(nbits - 21) | (1 << (nbits - 22))) & ~7 | 1
    targets = (LO, HI, [-HB] * H + [HB - 1] * H, [HB - 1] * H + [-HB] * H)
    one = km.bal_limbs(1, NL)
    squares = 0
    for name, p in mods.items():
        nm = km.bal_limbs(p, NL)
        n0inv = n0inv_of(nm)
        for T in targets:
            Tv = km.value(T)
            for kred, vf in ((True, True), (False, False)):
                st = km.BalStats()
                a = centered(-Tv * p)                                   # KARA_MUL: a * 1 == -T p
                w, m = km.kara_pass_bal(km.MUL, a, one, [0] * NL, nm, n0inv, st, kred=kred, vf=vf)
                assert m == T and km.value(w) * R == km.value(a) + Tv * p
                if p % 8 == 1 and T == LO:
                    # KARA_SQR: a^2 == -T p = 2^28 S p with S = 1 + 2^29 + ... == 1 modulo 8
                    S = -Tv >> 28
                    a = centered(_sqrt_mod_2n(S * p % (1 << (nbits - 28)), nbits - 28) << 14)
                    assert (km.value(a) ** 2 + Tv * p) % R == 0
                    w, m = km.kara_pass_bal(km.SQR, a, a, [0] * NL, nm, n0inv, st, kred=kred, vf=vf)
                    assert m == T and km.value(w) * R == km.value(a) ** 2 + Tv * p
                    squares += 1
    assert squares >= 2


def test_structured_moduli_and_lazy_bound():
    rng = random.Random(32)
    st = km.BalStats()
    primes = extreme_primes(1024) + [km.random_prime(1024, rng), km.random_prime(768, rng)]
    for p in primes:
        top = 51 * p // 100                                             # |a| = floor(0.51 s)
        ops = [km.bal_limbs(v, NL) for v in (top, -top, 0, 1, -1, p // 2, rng.randrange(-top, top + 1))]
        for red in REDS:
            for i, a in enumerate(ops):
                b, c, d = ops[(i + 1) % len(ops)], ops[(i + 2) % len(ops)], ops[(i + 4) % len(ops)]
                for w, v in (km.sqr_kara_bal(a, b, p, st, red), km.mul_kara_bal(a, b, c, d, p, st, red)):
                    assert km.in_lazy_range(w, p) and km.in_lazy_range(v, p)
                    assert all(-HB <= t < HB for t in w[:-1] + v[:-1])
    # moduli that are no primes and leave no headroom (R / p < 2^20): cells only
    for p in structured_moduli().values():
        nm = km.bal_limbs(p, NL)
        assert km.value(nm) == p
        for x in (LO, HI, centered(rng.randrange(R))):
            every_form(x, HI, LO, x, centered(rng.randrange(R)), nm, st)
    assert st.max_d < 1 << 63


def unsigned_exit(a, b, p):
    """The row-wise exit of the kernel on a pair of its own form (a in [0, 2p), b lazy): product by the plain element 1, then
    L = v (+ 1 if w >= p) reduced into [0, p) by two conditional subtractions."""
    pinv = pow(p, -1, R)
    assert 0 <= a < 4 * p and 0 <= b < 4 * p
    m = -a * pinv % R
    w = (a + m * p) // R
    s = b - m + R * p
    v = (s + (-s * pinv % R) * p) // R
    assert 0 <= w < 2 * p
    L = v + (1 if w >= p else 0)
    assert 0 <= L < 3 * p
    return L % p


def balanced_exit(al, bl, p):
    nb = km.bal_limbs(p, NL)
    ua, ub = km.from_balanced_plus_p(al, nb, 0), km.from_balanced_plus_p(bl, nb, 1)
    assert all(0 <= t <= km.MASK for t in ua + ub)
    A, Bv = km.value(ua), km.value(ub)
    assert A == km.value(al) + p and Bv == km.value(bl) - 1 + p
    return A, Bv


def test_chain_of_200_against_pow():
    """200 random squarings and products in balanced digits: the invariant is closed, the represented residue is CPython's,
    and the exit gives the words of the unsigned engine run on the same schedule (units and non-units)."""
    rng = random.Random(33)
    for bits, unit in ((1024, True), (768, True), (1024, False)):
        p = km.random_prime(bits, rng)
        p2 = p * p
        Rinv = pow(R, -1, p2)
        x = rng.randrange(p2) if unit else p * rng.randrange(1, p)
        y = rng.randrange(p2)
        xr, yr = x * R % p2, y * R % p2
        ua, ub, uc, ud = xr % p, xr // p, yr % p, yr // p                # the unsigned engine's pair (tools/kara_model.py)
        a, b = km.to_balanced(km.limbs(ua, NL)), km.to_balanced(km.limbs(ub, NL))
        c, d = km.to_balanced(km.limbs(uc, NL)), km.to_balanced(km.limbs(ud, NL))
        st, ust = km.BalStats(), km.Stats()
        want = x
        for step in range(200):
            if rng.random() < 0.7:
                a, b = km.sqr_kara_bal(a, b, p, st)
                ua, ub = km.sqr_kara(ua, ub, p, NL, ust, red=km.KMR_RED)
                want = want * want % p2
            else:
                a, b = km.mul_kara_bal(a, b, c, d, p, st)
                ua, ub = km.mul_kara(ua, ub, uc, ud, p, NL, ust, red=km.KMR_RED)
                want = want * y % p2
            assert km.in_lazy_range(a, p) and km.in_lazy_range(b, p)
            assert all(-HB <= t < HB for t in a[:-1] + b[:-1]) and abs(a[-1]) < 1 << 12 and abs(b[-1]) < 1 << 12
        assert (km.value(a) + km.value(b) * p) * Rinv % p2 == want
        A, Bv = balanced_exit(a, b, p)
        assert 0 <= A < 2 * p and 0 <= Bv < 2 * p
        assert (A + Bv * p) % p2 == (ua + ub * p) % p2
        assert unsigned_exit(A, Bv, p) == unsigned_exit(ua, ub, p)
        assert unsigned_exit(A, Bv, p) == want // p                     # the exit product leaves w + v p == want: L = want // p
        assert st.max_d < 1 << 63


def test_entry_and_exit_round_trips():
    rng = random.Random(34)
    for p in (km.random_prime(1024, rng), km.random_prime(768, rng), extreme_primes(1024)[0], extreme_primes(1024)[-1]):
        p2 = p * p
        vals = (0, 1, p - 1, p, p + 1, 2 * p - 1)
        for av in vals:
            for bv in vals:
                a, b = km.to_balanced(km.limbs(av, NL)), km.to_balanced(km.limbs(bv, NL))
                assert km.value(a) == av and km.value(b) == bv
                assert all(-HB <= t < HB for t in a[:-1] + b[:-1])
                A, Bv = balanced_exit(a, b, p)                           # the schedule-free path: straight back out
                assert (A + Bv * p) % p2 == (av + bv * p) % p2
                assert unsigned_exit(A, Bv, p) == unsigned_exit(av, bv, p)
        # after one operation the pair is inside the invariant and the exit's first digit inside [0, 2s)
        st = km.BalStats()
        a, b = km.to_balanced(km.limbs(2 * p - 1, NL)), km.to_balanced(km.limbs(2 * p - 1, NL))
        w, v = km.sqr_kara_bal(a, b, p, st)
        A, Bv = balanced_exit(w, v, p)
        assert 0 <= A < 2 * p and 0 <= Bv < 2 * p
