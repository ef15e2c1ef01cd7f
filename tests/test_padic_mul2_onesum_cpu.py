"""CPU: the cell-exact model of the second pass of a product, v = (a d + b c - m + m' p) / R, in the one-sum form with Karatsuba
quotient products (csrc/mont_padic.hpp: kara_pass_bal<KARA_MUL2, true, true, ONES>, in kernel mode PADIC_LDS_KMRBT when built with
-DPAI_KMRBT_PARTS=3, not the shipped build: profiles/r20/README.md; tools/kara_model.py: kara_pass_bal_sum, KMRBT_RED) against the shipped second pass (kara_pass_bal(MUL2, vf=True), schoolbook
quotient products, the product stream as one chain V_k) and against the rule on plain integers (schoolbook_second_pass), on
the operand families of tests/test_padic_onesum_cpu.py and tests/test_padic_balanced_cpu.py.

S_k = V_k + U_k now sums the half products of both pairs and the quotient stream; the model runs the pass in 64-bit cells that
wrap and asserts at every column that the finished column, read as a signed 64-bit integer, is the schoolbook column and
below 2^63.  Here out, mq and every carry must be those of the shipped pass, bit for bit, in both placements of the newest
quotient digit's terms:
  - all limbs at -2^28 and all limbs at 2^28 - 1 in all four operands, the incoming m and the modulus,
  - second passes with every product of a column of one sign in both streams and the incoming m solved so that the quotient
    digits are all -2^28 / all 2^28 - 1 (and at opposite extremes in the two halves),
  - the structured moduli of tests/golden/extreme_keys.json and of tests/test_padic_kred_cpu.py,
  - the lazy bound |a| = floor(0.51 s), a 768-bit prime on 36 limbs,
  - a chain of 200 mixed squarings and products against CPython modulo s^2.
Each test prints the largest finished column and the largest carry it met.
(The kernel itself is held to the oracle on the GPU: tests/test_gpu_padic_stage.py.)"""
import math
import random

from tests.test_padic_balanced_cpu import HB, HI, LO, NL, H, R, centered, n0inv_of
from tests.test_padic_kara_mul_cpu import extreme_primes
from tests.test_padic_kred_cpu import km, structured_moduli

PLACEMENTS = (1, 2)                                        # the newest digit's terms onto S_k once / onto S_k and the column
STAGE_REDS = (km.KMRBT_RED, km.KMRBT_RED | km.ONES2)


def report(name, st):
    print(f"{name}: largest |column| 2^{math.log2(st.max_d):.3f}, largest |carry| 2^{math.log2(max(st.max_c, 1)):.3f}")


def same_second_pass(x, y, x2, y2, mnin, nm, st):
    """The pass in the shipped form, on plain integers and in both one-sum placements: identical out, mq and carries."""
    n0inv = n0inv_of(nm)
    ref = km.kara_pass_bal(km.MUL2, x, y, mnin, nm, n0inv, km.BalStats(), x2=x2, y2=y2, kred=False, vf=True)
    out, mq, carries = km.schoolbook_second_pass(x, y, x2, y2, mnin, nm, n0inv)
    assert (out, mq) == ref                                # the shipped pass is the rule: its carries are `carries`
    assert out[NL - 1] == carries[-1] and len(carries) == 2 * NL - 1
    for ones in PLACEMENTS:
        got = km.kara_pass_bal_sum(x, y, x2, y2, mnin, nm, n0inv, st, ones=ones)
        assert got[0] == out and got[1] == mq, ones
        assert got[2] == carries, ones
    assert st.max_d < 1 << 63
    return out, mq


def test_masks_and_counts():
    assert km.KMRBT_RED == km.KMRBS_RED | 1 << km.MUL2 and not km.KMRBS_RED >> km.MUL2 & 1
    assert [km.red_ones(r) for r in STAGE_REDS] == [1, 2]
    # quotient multiply-adds of the pass: those of the one-sum first pass (tests/test_padic_onesum_cpu.py), against 1 296
    st = km.BalStats()
    n0inv = n0inv_of(HI)
    km.kara_pass_bal_sum(LO, HI, HI, LO, LO, HI, n0inv, st, ones=1)
    assert st.red_macs == 3 * H * H + H + H == 1008
    km.kara_pass_bal_sum(LO, HI, HI, LO, LO, HI, n0inv, st, ones=2)
    assert st.red_macs == 1008 + NL


def test_all_limbs_at_the_extremes():
    st = km.BalStats()
    odd_lo = [-HB + 1] + [-HB] * (NL - 1)                  # a modulus must be odd
    for nm in (HI, odd_lo):
        for x in (LO, HI):
            for y in (LO, HI):
                for x2 in (LO, HI):
                    for y2 in (LO, HI):
                        for mnin in (LO, HI):
                            same_second_pass(x, y, x2, y2, mnin, nm, st)
    report("all limbs at the extremes", st)
    assert st.max_d < 1 << 63


def test_second_pass_columns_of_one_sign():
    """a d + b c with every limb product of one sign in both streams and the quotient digits all at one extreme, of the sign
    that makes every quotient product agree with them: the largest column of the pass, 36 (2^57 + 2^56) (1 - eps); the cells
    that hold S_k wrap, the finished column must not."""
    nm = HI
    p = km.value(nm)
    worst = 0
    halves = ([-HB] * H + [HB - 1] * H, [HB - 1] * H + [-HB] * H)
    for x, y, T in ((LO, HI, LO), (LO, LO, HI), (HI, HI, HI), (HI, LO, LO), (LO, HI, halves[0]), (HI, HI, halves[1])):
        Tv = km.value(T)
        prod = 2 * km.value(x) * km.value(y)               # x y + y x
        m_in = centered(prod + Tv * p)
        st = km.BalStats()
        out, mq = same_second_pass(x, y, y, x, m_in, nm, st)
        assert mq == T
        assert km.value(out) * R == prod - km.value(m_in) + Tv * p
        if T in (LO, HI):
            worst = max(worst, st.max_d)
        report("columns of one sign", st)
    assert 0.999 * (NL * 3 << 56) < worst < 1 << 63


def test_structured_moduli_and_lazy_bound():
    rng = random.Random(52)
    st = km.BalStats()
    primes = extreme_primes(1024) + [km.random_prime(1024, rng), km.random_prime(768, rng)]
    for p in primes:
        top = 51 * p // 100                                             # |a| = floor(0.51 s)
        ops = [km.bal_limbs(v, NL) for v in (top, -top, 0, 1, -1, p // 2, rng.randrange(-top, top + 1))]
        nm = km.bal_limbs(p, NL)
        for i, a in enumerate(ops):
            b, c, d = ops[(i + 1) % len(ops)], ops[(i + 2) % len(ops)], ops[(i + 4) % len(ops)]
            mu = km.mul_kara_bal(a, b, c, d, p, st, km.KMRBS_RED)
            for red in STAGE_REDS:
                assert km.mul_kara_bal_stage(a, b, c, d, p, st, red) == mu
            assert km.in_lazy_range(mu[0], p) and km.in_lazy_range(mu[1], p)
            same_second_pass(a, d, b, c, centered(rng.randrange(R)), nm, st)
    # moduli that are no primes and leave no headroom (R / p < 2^20): cells only
    for p in structured_moduli().values():
        nm = km.bal_limbs(p, NL)
        for x in (LO, HI, centered(rng.randrange(R))):
            mnin = centered(rng.randrange(R))
            same_second_pass(x, HI, HI, x, mnin, nm, st)
            same_second_pass(x, LO, HI, x, mnin, nm, st)
    report("structured moduli and lazy bound", st)
    assert st.max_d < 1 << 63


def test_chain_of_200_against_pow():
    """200 mixed squarings and products: every product's pair is that of the shipped form, limb for limb, in both placements,
    and the represented residue is CPython's."""
    rng = random.Random(53)
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
                ref = km.sqr_kara_bal(a, b, p, st, km.KMRBS_RED)
                want = want * want % p2
            else:
                ref = km.mul_kara_bal(a, b, c, d, p, st, km.KMRBS_RED)
                for red in STAGE_REDS:
                    assert km.mul_kara_bal_stage(a, b, c, d, p, st, red) == ref, step
                want = want * y % p2
            a, b = ref
            assert km.in_lazy_range(a, p) and km.in_lazy_range(b, p)
        assert (km.value(a) + km.value(b) * p) * Rinv % p2 == want
        report(f"chain of 200 at {bits} bits", st)
        assert st.max_d < 1 << 63
