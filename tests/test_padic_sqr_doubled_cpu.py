"""CPU: the cell-exact model of the first pass of a squaring, w = (a^2 + m p) / R, in the one-sum form with the off-diagonal
products summed on the DOUBLED operand (csrc/mont_padic.hpp: kara_pass_bal<KARA_SQR, true, true, ONES, DSYM>, KRED_DSYM, in
kernel mode PADIC_LDS_KMRBT when built with PAI_KMRBT_PARTS & 4: profiles/r25/README.md; tools/kara_model.py: kara_pass_bal
with dsym) against the shipped pass (the off-diagonal products on a chain of their own that is shifted once per column) and
against the rule on plain integers (rule_first_pass below).

x_i (2 x_l) and (x_i x_l) << 1 are the same 64-bit word, so every stored sum S_k, the chain e and with them the finished
column are the same cells: out, mq and the carry out of every column must be those of the shipped pass, bit for bit, in both
placements of the newest quotient digit's terms.  Inputs: random limbs, all limbs at -2^28, all at 2^28 - 1, alternating
extremes, and the two halves at opposite extremes (every x[H + i] - x[i] at +-(2^29 - 1), doubled 2^30 - 2: the largest
int32 the pass forms), each on the moduli all limbs at 2^28 - 1, all at -2^28 (odd), random primes of 1024 and 768 bits and
the structured moduli of tests/test_padic_kred_cpu.py; whole squarings in a chain of 200 against CPython modulo s^2.

Bounds (36 limbs, H = 18).  A stored sum is S_k = V_k + U_k, at most 2 H products of the operand and 2 H quotient products,
each at most 2^56: |S_k| <= 72 2^56 < 2^62.17, so in this pass not even the stored sum wraps; with the doubled operand a
single term is at most 2^57 (2^59 for the half differences), which the 64-bit cell holds modulo 2^64.  The finished column is
36 (2^56 + 2^56) + 2^35 < 2^62.18 in magnitude.  Each test prints the largest stored sum and the largest finished column it met.
(The kernel itself is held to its predecessor and to the oracle on the GPU: tests/test_gpu_padic_sqr_doubled.py.)"""
import math
import random

from tests.test_padic_balanced_cpu import HB, HI, LO, NL, H, R, centered, n0inv_of
from tests.test_padic_kara_mul_cpu import extreme_primes
from tests.test_padic_kred_cpu import km, structured_moduli

PLACEMENTS = (1, 2)
S_BOUND = 4 * H << 56                                      # 2 H operand products and 2 H quotient products of 2^56
D_BOUND = (2 * NL << 56) + (1 << 35)                       # NL + NL products of 2^56 and the carry
ALT = [-HB if i % 2 else HB - 1 for i in range(NL)]
ALT2 = [HB - 1 if i % 2 else -HB for i in range(NL)]
HALVES = ([-HB] * H + [HB - 1] * H, [HB - 1] * H + [-HB] * H)
ODD_LO = [-HB + 1] + [-HB] * (NL - 1)                      # a modulus must be odd


def report(name, st):
    print(f"{name}: largest |stored sum| 2^{math.log2(max(st.max_s, 1)):.3f}, largest |column| 2^{math.log2(st.max_d):.3f}, "
          f"largest |carry| 2^{math.log2(max(st.max_c, 1)):.3f}")


def rule_first_pass(x, nm, n0inv):
    """w = (x^2 + m p) / R column by column on plain integers: (out, mq, the carry out of every column)."""
    mq, out, carries = [0] * NL, [0] * NL, []
    carry = 0
    for k in range(2 * NL - 1):
        lo, hi = max(0, k - NL + 1), min(k, NL - 1)
        d = carry + sum(x[i] * x[k - i] for i in range(lo, hi + 1))
        d += sum(mq[i] * nm[k - i] for i in range(lo, min(hi, k - 1) + 1))
        if k < NL:
            mq[k] = km.sfield((d * n0inv) & km.MASK)
            d += mq[k] * nm[0]
            assert d % km.B == 0
            carry = d >> km.RB
        else:
            out[k - NL] = km.sfield(d)
            carry = (d + HB) >> km.RB
        carries.append(carry)
    out[NL - 1] = carry
    return out, mq, carries


def same_first_pass(x, nm, st):
    """The pass in the shipped form, on plain integers and on the doubled operand, both placements: identical out, mq, carries."""
    n0inv = n0inv_of(nm)
    out, mq, carries = rule_first_pass(x, nm, n0inv)
    assert km.value(out) * R == km.value(x) ** 2 + km.value(mq) * km.value(nm)
    for ones in PLACEMENTS:
        t0, t1 = [], []
        ref = km.kara_pass_bal(km.SQR, x, x, [0] * NL, nm, n0inv, km.BalStats(), kred=True, vf=True, ones=ones, trace=t0)
        got = km.kara_pass_bal(km.SQR, x, x, [0] * NL, nm, n0inv, st, kred=True, vf=True, ones=ones, dsym=True, trace=t1)
        assert ref == (out, mq) and t0 == carries, ones
        assert got == (out, mq), ones
        assert t1 == carries and len(t1) == 2 * NL - 1, ones
    assert st.max_s <= S_BOUND and st.max_d < D_BOUND < 1 << 63
    return out, mq


def test_mask_and_model_switch():
    assert km.DSYM == 512 and not km.KMRBT_RED & km.DSYM and not km.KMRBS_RED & km.DSYM
    # the quotient multiply-adds stay those of the one-sum pass: the doubled operand changes the operand products only
    a, b = km.BalStats(), km.BalStats()
    n0inv = n0inv_of(HI)
    km.kara_pass_bal(km.SQR, LO, LO, [0] * NL, HI, n0inv, a, kred=True, vf=True, ones=1)
    km.kara_pass_bal(km.SQR, LO, LO, [0] * NL, HI, n0inv, b, kred=True, vf=True, ones=1, dsym=True)
    assert a.red_macs == b.red_macs == 3 * H * H + H + H
    # the other forms and the two-sum pass ignore it
    rng = random.Random(70)
    x, y = centered(rng.randrange(R)), centered(rng.randrange(R))
    for form in (km.SQR2, km.MUL):
        assert km.kara_pass_bal(form, x, y, LO, HI, n0inv, km.BalStats(), kred=True, vf=True, ones=1, dsym=True) == \
            km.kara_pass_bal(form, x, y, LO, HI, n0inv, km.BalStats(), kred=True, vf=True, ones=1)


def test_limbs_at_the_extremes():
    st = km.BalStats()
    for nm in (HI, ODD_LO):
        for x in (LO, HI, ALT, ALT2) + HALVES:
            same_first_pass(x, nm, st)
    report("limbs at the extremes", st)
    # all limbs of one sign, modulus and quotient digits to match: the stored sums reach 0.49 of their bound at least
    assert st.max_s > S_BOUND // 4


def test_random_limbs_on_primes_and_structured_moduli():
    rng = random.Random(71)
    st = km.BalStats()
    moduli = extreme_primes(1024) + [km.random_prime(1024, rng), km.random_prime(768, rng)] + list(structured_moduli().values())
    for p in moduli:
        nm = km.bal_limbs(p, NL)
        top = 51 * p // 100
        for x in (centered(rng.randrange(R)), [rng.randrange(-HB, HB) for _ in range(NL)], km.bal_limbs(top, NL),
                  km.bal_limbs(-top, NL), LO, HI, ALT, HALVES[0], HALVES[1]):
            same_first_pass(x, nm, st)
    report("random limbs, primes and structured moduli", st)


def test_chain_of_200_squarings_against_pow():
    """Whole squarings (both passes) with and without the doubled operand: the same pair limb for limb, the residue CPython's."""
    rng = random.Random(72)
    for bits in (1024, 768):
        p = km.random_prime(bits, rng)
        p2 = p * p
        x = rng.randrange(p2)
        xr = x * R % p2
        a, b = km.to_balanced(km.limbs(xr % p, NL)), km.to_balanced(km.limbs(xr // p, NL))
        st = km.BalStats()
        want = x
        for step in range(200):
            ref = km.sqr_kara_bal(a, b, p, km.BalStats(), km.KMRBS_RED)
            for red in (km.KMRBS_RED | km.DSYM, km.KMRBS_RED | km.ONES2 | km.DSYM, km.KMRBT_RED | km.DSYM):
                assert km.sqr_kara_bal(a, b, p, st, red) == ref, step
            a, b = ref
            want = want * want % p2
            assert km.in_lazy_range(a, p) and km.in_lazy_range(b, p)
        assert (km.value(a) + km.value(b) * p) * pow(R, -1, p2) % p2 == want
        report(f"chain of 200 squarings at {bits} bits", st)
        assert st.max_d < 1 << 63
