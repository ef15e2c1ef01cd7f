"""Cell-exact model of the register-resident Karatsuba squaring and product of the digit-pair engine (csrc/mont_padic.hpp:
kara_pass, sqr_kara, mul_kara_reg).

It follows kara_pass column by column: 32-bit signed difference limbs, signed 64-bit limb products, the product column X_k
accumulated modulo 2^64, its carry stream cc and the reduction column d.  Beside every 64-bit cell it keeps the unbounded
value and records the largest one, and it asserts that
  - every difference limb fits int32 and every signed product int64,
  - X_k (accumulated modulo 2^64) equals the schoolbook column sum_i x_i y_(k-i) exactly,
  - cc, d and the carries never reach 2^64,
  - w = (a^2 + m p) / R and v = (2 a b - m + R p + m' p) / R exactly, and w + v p == (a + b p)^2 R^-1 (mod p^2),
  - with kred (kara_pass<FORM, true>): the quotient products m p of the reduction by the same column form,
    Y_k = Q0_k + (Q0 + Q2 - E)_(k-H) + Q2_(k-2H) = U_k + U_(k-H) - E_(k-H) with U_k = Q0_k + Q2_(k-H), Q0 = m0 p0,
    Q2 = m1 p1, E = (m0 - m1)(p0 - p1): the stored sums U_k (one chain of at most H products each) fit 64 bits, every signed product and every partial sum of -E fits int64, the reduction column d (exact modulo
    2^64 at every partial sum) ends as the schoolbook column in [0, 2^64), and the quotient digits, out and the carry are
    those of the schoolbook rule; the multiply-adds of the reduction are counted (3 H^2 + H instead of NL^2),
  - with vf (kara_pass<FORM, KRED, true>; not for MUL2): the product stream as V_k = P0_k + P2_(k-H), one chain kept for H
    columns, X_k = V_k + V_(k-H) - D_(k-H); a square sums the pairs i < l once and doubles the sum (likewise their signed
    products in -D): the chains, the doubled sums and V_k fit 64 bits resp. int64, X_k is the schoolbook column,
  - for a product: the summed half products of a d + b c fit 64 bits, their signed difference part fits int64, the middle
    part is non-negative and enters through a 128-bit cell, and w, v are those of the row-wise product rule.
The balanced-digit form (kara_pass_bal, one signed 64-bit cell per column) has its own model below: kara_pass_bal.
The product (a, b) * (c, 0) beyond 36 limbs in two half-width steps (kara2_step_bal, mul_kara2_c0_bal: the 72-limb encryption
kernel) follows it: kara2_step_bal, in wrapping 64-bit cells, every finished column asserted to be the exact schoolbook column.
Run: python tools/kara_model.py [rounds]
"""
import random
import sys

RB = 29
B = 1 << RB
MASK = B - 1
M64 = (1 << 64) - 1


def limbs(x, n):
    return [(x >> (RB * i)) & MASK for i in range(n)]


def value(l):
    return sum(v << (RB * i) for i, v in enumerate(l))


class Stats:
    def __init__(self):
        self.max_cc = self.max_d = self.max_col = self.max_run = self.max_e = 0
        self.max_rq = self.max_red_e = 0      # kred: largest stored half product, largest |partial sum of -E|
        self.red_macs = 0                     # multiply-adds of the quotient products in the last pass
        self.dm_signs = set()                 # kred: signs of mq[i] - mq[H + i] met


SQR, SQR2, MUL, MUL2 = 0, 1, 2, 3     # kara_pass<FORM>: KARA_SQR, KARA_SQR2, KARA_MUL, KARA_MUL2
VF = 16                               # sqr_kara_reg<RED>: the squaring's product streams in the one-chain form V_k
VFM = 32                              # mul_kara_reg<RED>: the same for the first pass of a product (a c)
KMR_RED = 1 << SQR | 1 << SQR2 | 1 << MUL | VF | VFM      # Padic::PADIC_KMR_RED: what kernel mode PADIC_LDS_KMR runs


def kara_pass(form, x, y, mnin, nm, n0inv, st, x2=None, y2=None, kred=False, vf=False):
    """One pass of kara_pass<FORM>; x, y (x2, y2: the second pair of MUL2), mnin, nm are limb lists.  Returns (out limbs,
    quotient limbs).  form may be given as False / True for the two squaring passes."""
    form = int(form)
    sym, dbl, summ = form == SQR, form == SQR2, form == MUL2
    second = dbl or summ
    NL = len(x)
    H = NL // 2
    NP = 2 * H - 1
    nx = [x[i + H] - x[i] for i in range(H)]
    dy = [y[i] - y[i + H] for i in range(H)]
    nx2 = [x2[i + H] - x2[i] for i in range(H)] if summ else [0] * H
    dy2 = [y2[i] - y2[i + H] for i in range(H)] if summ else [2 * d for d in dy]
    yd = [v << 1 for v in y]
    for v in nx + dy + nx2 + dy2:
        assert -(1 << 31) <= v < (1 << 31), "difference limb leaves int32"
    for v in yd:
        assert v < (1 << 32)

    def half(o, j):
        s = 0
        lo, hi = (0, j) if j < H else (j - H + 1, H - 1)
        for i in range(lo, hi + 1):
            l = j - i
            if not sym:
                s += x[o + i] * y[o + l]
            elif i < l:
                s += x[o + i] * yd[o + l]
            elif i == l:
                s += x[o + i] * y[o + i]
            if summ:
                s += x2[o + i] * y2[o + l]
            assert s <= M64, "half-product coefficient wraps"
        return s

    def column(xx, yy, k):
        return sum(xx[i] * yy[k - i] for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1))

    p0 = [0] * NP
    p2 = [0] * NP
    pv = [0] * (H + NP)  # vf: V_k = P0_k + P2_(k-H) of the product stream
    cc = carry = 0
    mq = [0] * NL
    out = [0] * NL
    ru = [0] * (H + NP)  # kred: U_k = Q0_k + Q2_(k-H) of the quotient stream, live for H columns each
    dm = [0] * H         # kred: mq[i] - mq[H + i]
    ndp = [nm[H + l] - nm[l] for l in range(H)]
    macs = 0
    for k in range(2 * NL - 1):
        t = 0            # unbounded running value; the cell holds t mod 2^64
        nd = [0, 0]      # MUL2: -D_j of either pair, two signed 64-bit cells (their sum can pass 2^63)
        mid = H <= k < H + NP
        if vf and not summ:
            # V_k = P0_k + P2_(k-H) as one chain, kept for H columns: X_k = V_k + V_(k-H) - D_(k-H); a square takes the
            # pairs i < l once and doubles their sum (off), likewise in -D (ndo)
            vk = off = ndo = 0
            for o, jj, on in ((0, k, k < NP), (H, k - H, mid)):
                if not on:
                    continue
                lo, hi = (0, jj) if jj < H else (jj - H + 1, H - 1)
                for i in range(lo, hi + 1):
                    l = jj - i
                    if not sym:
                        vk += x[o + i] * y[o + l]
                    elif i < l:
                        off += x[o + i] * y[o + l]
                    elif i == l:
                        vk += x[o + i] * y[o + i]
                    assert vk <= M64 and off <= M64, "chain of half products wraps"
            if sym:
                assert off << 1 <= M64
                vk += off << 1
            assert vk <= M64, "V_k wraps"
            st.max_run = max(st.max_run, vk)
            if k < H + NP:
                pv[k] = vk
            else:
                assert vk == 0
            t = vk + (pv[k - H] if k >= H else 0)
            if mid:
                j = k - H
                lo, hi = (0, j) if j < H else (j - H + 1, H - 1)
                for i in range(lo, hi + 1):
                    l = j - i
                    pr = nx[i] * dy[l]
                    assert -(1 << 63) <= pr < (1 << 63), "signed product leaves int64"
                    if not sym:
                        t += pr
                    elif i < l:
                        ndo += pr
                        assert -(1 << 62) <= ndo < (1 << 62), "signed sum of the pairs i < l does not double in int64"
                    elif i == l:
                        t += pr
                t += ndo << 1
        elif k < NP:
            p0[k] = half(0, k)
            t += p0[k]
        if mid and not (vf and not summ):
            j = k - H
            p2[j] = half(H, j)
            if not summ:
                t += p0[j] + p2[j]
            st.max_run = max(st.max_run, t)
            lo, hi = (0, j) if j < H else (j - H + 1, H - 1)
            for i in range(lo, hi + 1):
                l = j - i
                if summ:
                    for g, pr in enumerate((nx[i] * dy[l], nx2[i] * dy2[l])):
                        assert -(1 << 63) <= pr < (1 << 63), "signed product leaves int64"
                        nd[g] += pr
                        assert -(1 << 63) <= nd[g] < (1 << 63), "signed sum leaves int64"
                    continue
                if not sym:
                    pr = nx[i] * dy[l]
                elif i < l:
                    pr = nx[i] * dy2[l]
                elif i == l:
                    pr = nx[i] * dy[i]
                else:
                    continue
                assert -(1 << 63) <= pr < (1 << 63), "signed product leaves int64"
                t += pr
                st.max_run = max(st.max_run, t)
        if k >= 2 * H and not (vf and not summ):
            t += p2[k - 2 * H]
        # the cell is exact modulo 2^64; the column itself must be the schoolbook one and lie in [0, 2^64)
        want = column(x, y, k) + (column(x2, y2, k) if summ else 0)
        if summ:
            e0 = p0[k - H] + p2[k - H] + nd[0] + nd[1] if mid else 0       # the middle part: enters through the 128-bit cell
            assert t + e0 == want, (k, t, e0, want)
            assert e0 >= 0
        else:
            assert t == want, (k, t, want)
        assert 0 <= t <= M64
        st.max_col = max(st.max_col, t)
        c = t + cc
        assert c <= M64, "product stream wraps"
        st.max_cc = max(st.max_cc, c)
        cc = c >> RB
        if summ and mid:
            e = e0 + (c & MASK)
            assert 0 <= e < (1 << 128)
            st.max_e = max(st.max_e, e)
            cc += e >> RB
            assert cc <= M64
            c = e & M64
        lowc = (c & MASK) << 1 if dbl else (c & MASK)
        d = lowc
        if second:
            d += (MASK - mnin[k]) + (1 if k == 0 else 0) if k < NL else nm[k - NL] - (1 if k == NL else 0)
        lo, hi = (0, k - 1) if k < NL else (k - NL + 1, NL - 1)
        # the schoolbook column up to (not including) the column's own digit
        school = d + carry + sum(mq[i] * nm[k - i] for i in range(lo, hi + 1))
        if not kred:
            macs += hi - lo + 1 + (1 if k < NL else 0)
            d = school
            if k < NL:
                mq[k] = ((d & 0xFFFFFFFF) * n0inv) & MASK
                d += mq[k] * nm[0]
            else:
                out[k - NL] = d & MASK
        else:
            # d is the 64-bit cell (exact modulo 2^64 at every partial sum: signed terms); dt its unbounded value
            dt = d
            has_u, midr = k < H + NP, H <= k < H + NP
            u = 0                                           # U_k = Q0_k + Q2_(k-H): one chain of multiply-adds
            e = 0                                           # partial sum of -E_j (chained onto d in the kernel)

            def signed(a, b):
                nonlocal dt, e, macs
                assert -(1 << 31) <= a < (1 << 31) and -(1 << 31) <= b < (1 << 31), "signed operand leaves int32"
                pr = a * b
                assert -(1 << 63) <= pr < (1 << 63), "signed product leaves int64"
                e += pr
                assert -(1 << 63) <= e < (1 << 63), "partial sum of -E leaves int64"
                st.max_red_e = max(st.max_red_e, abs(e))
                dt += pr
                macs += 1

            if k < NP:
                lo0, hi0 = (0, k - 1) if k < H else (k - H + 1, H - 1)
                for i in range(lo0, hi0 + 1):
                    if i != k - 1:
                        u += mq[i] * nm[k - i]
                        macs += 1
            if midr:
                j = k - H
                lo2, hi2 = (0, j) if j < H else (j - H + 1, H - 1)
                for i in range(lo2, hi2 + 1):
                    l = j - i
                    if i == j and k < NL:
                        signed(mq[i], ndp[0])
                    elif H + i != k - 1:
                        u += mq[H + i] * nm[H + l]
                        macs += 1
                        signed(dm[i], ndp[l])
            if k >= H:
                dt += ru[k - H]
            dt += carry
            if 1 <= k <= H:
                u += mq[k - 1] * nm[1]
                macs += 1
            if H <= k - 1 < NL:
                u += mq[k - 1] * nm[H + 1]
                macs += 1
                signed(dm[k - 1 - H], ndp[1])
            if k < H:
                mq[k] = ((((dt & 0xFFFFFFFF) + (u & 0xFFFFFFFF)) & 0xFFFFFFFF) * n0inv) & MASK
                u += mq[k] * nm[0]
                macs += 1
                dt += u
            else:
                if has_u:
                    dt += u
                if k < NL:
                    assert dt == school, (k, dt, school)      # all but the own digit: m[k] (p[H] - (p[H] - p[0])) follows
                    mq[k] = ((dt & 0xFFFFFFFF) * n0inv) & MASK
                    dt += mq[k] * nm[0]
                    u += mq[k] * nm[H]
                    macs += 2
                    dm[k - H] = mq[k - H] - mq[k]
                    assert -(1 << 31) <= dm[k - H] < (1 << 31)
                    st.dm_signs.add((dm[k - H] > 0) - (dm[k - H] < 0))
                else:
                    out[k - NL] = dt & MASK
            assert u <= M64, "stored sum of half products of the quotient stream wraps"
            st.max_rq = max(st.max_rq, u)
            if has_u:
                ru[k] = u
            else:
                assert u == 0
            # the cell is the schoolbook column: same digit, same value, inside [0, 2^64)
            want_d = school + (mq[k] * nm[0] if k < NL else 0)
            assert dt == want_d and 0 <= dt <= M64, (k, dt, want_d)
            if k < NL:
                assert mq[k] == ((school & 0xFFFFFFFF) * n0inv) & MASK
            d = dt
        assert d <= M64, "reduction column wraps"
        st.max_d = max(st.max_d, d)
        carry = d >> RB
    top = carry + (cc << 1 if dbl else cc) + (nm[NL - 1] if second else 0)
    assert top <= 0xFFFFFFFF
    st.red_macs = macs
    out[NL - 1] = top          # unmasked here: the caller checks that it fits 29 bits where the digits are in range
    return out, mq


def mul_kara(a, b, c, d, p, NL, st, in_range=True, red=0):
    """(a, b) * (c, d) -> (w, v) by the two product passes (mul_kara_reg<red>: bit FORM of red = that pass reduces by
    Karatsuba columns); checks them against the row-wise product rule
    w = (a c + m p) / R, v = (a d + b c - m + R p + m' p) / R on Python integers (m, m' the unique quotients modulo R)."""
    R = 1 << (RB * NL)
    nm = limbs(p, NL)
    n0inv = (-pow(p, -1, B)) % B
    al, bl, cl, dl = limbs(a, NL), limbs(b, NL), limbs(c, NL), limbs(d, NL)
    assert (value(al), value(bl), value(cl), value(dl)) == (a, b, c, d)
    w, m = kara_pass(MUL, al, cl, [0] * NL, nm, n0inv, st, kred=bool(red >> MUL & 1), vf=bool(red & VFM))
    v, m2 = kara_pass(MUL2, al, dl, m, nm, n0inv, st, x2=bl, y2=cl, kred=bool(red >> MUL2 & 1))
    W, M, V, M2 = value(w), value(m), value(v), value(m2)
    pinv = pow(p, -1, R)
    assert M == (-a * c * pinv) % R and W == (a * c + M * p) // R and (a * c + M * p) % R == 0
    s = a * d + b * c - M + R * p
    assert M2 == (-s * pinv) % R and V * R == s + M2 * p
    if in_range:
        assert max(w) <= MASK and max(v) <= MASK, "result limb beyond 29 bits"
        p2 = p * p
        assert (W + V * p) % p2 == (a + b * p) * (c + d * p) * pow(R, -1, p2) % p2
    return W, V


def sqr_kara(a, b, p, NL, st, in_range=True, red=0):
    """(a, b) -> (w, v) by the two passes (sqr_kara_reg<red>); checks the exact relations."""
    R = 1 << (RB * NL)
    nm = limbs(p, NL)
    n0inv = (-pow(p, -1, B)) % B
    al, bl = limbs(a, NL), limbs(b, NL)
    assert value(al) == a and value(bl) == b
    w, m = kara_pass(SQR, al, al, [0] * NL, nm, n0inv, st, kred=bool(red >> SQR & 1), vf=bool(red & VF))
    v, m2 = kara_pass(SQR2, al, bl, m, nm, n0inv, st, kred=bool(red >> SQR2 & 1), vf=bool(red & VF))
    W, M, V, M2 = value(w), value(m), value(v), value(m2)
    assert (a * a + M * p) % R == 0 and W == (a * a + M * p) // R
    assert V * R == 2 * a * b - M + R * p + M2 * p
    if in_range:
        assert max(w) <= MASK and max(v) <= MASK, "result limb beyond 29 bits"
        x = (a + b * p) % (p * p)
        Rinv = pow(R, -1, p * p)
        # (a, b) ~ x R^-1... : w + v p == (a + b p)^2 R^-1  (mod p^2), i.e. the digit form of the square
        assert (W + V * p) % (p * p) == (x * x * Rinv) % (p * p) == pow(x, 2, p * p) * Rinv % (p * p)
    return W, V


# ---- balanced digits: one carry stream per column (kara_pass_bal, sqr_kara_reg_bal, mul_kara_reg_bal; kernel mode
# PADIC_LDS_KMRB) ---------------------------------------------------------------------------------------------------------
# Limbs are signed digits in [-2^28, 2^28) (the top limb keeps what is left), the modulus limbs and the quotient digits
# too.  The model follows kara_pass_bal cell by cell on unbounded integers and asserts that
#   - every limb, difference limb and quotient digit fits int32 and every signed product int64,
#   - every stored sum is within its bound: |V_k| <= H 2^56 (2 H 2^56 for the sum of two products), |U_k| <= H 2^56, the half
#     products likewise, |D_j|, |E_j| partial sums < H 2^58 — so each 64-bit cell holds its value exactly, not only modulo 2^64,
#   - the finished column d_k is the schoolbook column [2] X_k - min_k + sum_i mq_i nm_(k-i) + carry and |d_k| < 2^63,
#   - mq and out (all but the top limb) are in [-2^28, 2^28), d_k + mq_k nm_0 == 0 (mod 2^29) for k < NL,
#   - (callers) w R = x y + m p and v R = a d + b c - m + m' p exactly.
VFS = 64                              # mul_kara_reg_bal<RED>: the second pass of a product (sum of two products) as one chain too
KMRB_RED = KMR_RED | VFS              # Padic::PADIC_KMRB_RED: what kernel mode PADIC_LDS_KMRB runs
HB = B >> 1                           # 2^28
# One stored sum per column (kernel mode PADIC_LDS_KMRBS): the passes with both kred and vf (both of a squaring, the first of a
# product) keep S_k = [2] V_k + U_k instead of V_k and U_k; the column is S_k + S_(k-H) - [2] D_(k-H) - E_(k-H) - min_k + carry.
# The model runs that pass in 64-bit cells that WRAP (S_k is needed modulo 2^64 only: [2] V_k + U_k can pass 2^63) and asserts
# that the finished column, read as a signed 64-bit integer, is the schoolbook column.  ONES2 on top: the terms of the newest
# quotient digit go onto the sum and onto the column separately instead of onto the sum before the column is formed.
ONES, ONES2 = 128, 256
KMRBS_RED = KMRB_RED | ONES           # Padic::PADIC_KMRBS_RED: what kernel mode PADIC_LDS_KMRBS runs
DSYM = 512                            # Padic::KRED_DSYM: the first pass of a squaring sums its off-diagonal products on the doubled
                                      # operand (kernel mode PADIC_LDS_KMRBT with PAI_KMRBT_PARTS & 4)
M64 = (1 << 64) - 1


def red_ones(red):
    """Padic::ones(RED): 0 = two stored sums, 1 / 2 = one, the newest digit's terms once / twice."""
    return (2 if red & ONES2 else 1) if red & ONES else 0


def sfield(v):
    """The signed 29-bit field of a word."""
    v &= MASK
    return v - B if v >= HB else v


def bal_limbs(x, n):
    """Balanced digits of the signed integer x: n - 1 digits in [-2^28, 2^28), the top limb keeps the rest."""
    out = []
    for _ in range(n - 1):
        r = sfield(x)
        out.append(r)
        x = (x - r) >> RB
    out.append(x)
    return out


def to_balanced(x):
    """Padic::to_balanced: lazy unsigned limbs -> balanced digits of the same integer (int32 cells)."""
    r, c = [], 0
    for j in range(len(x) - 1):
        t = x[j] + c
        assert -(1 << 31) <= t + HB < (1 << 31)
        r.append(sfield(t))
        c = (t + HB) >> RB
    r.append(x[-1] + c)
    assert -(1 << 31) <= r[-1] < (1 << 31)
    return r


def from_balanced_plus_p(x, nb, less):
    """Padic::from_balanced_plus_p: balanced digits of x and of p -> limbs in [0, 2^29) of x + p - less (which must lie in [0, R))."""
    r, c = [], -less
    for j in range(len(x)):
        t = x[j] + nb[j] + c
        assert -(1 << 31) <= t < (1 << 31)
        r.append(t & MASK)
        c = t >> RB
    assert c == 0, "x + p - less leaves [0, R)"
    return r


class BalStats:
    def __init__(self):
        self.max_d = self.max_v = self.max_u = self.max_e = 0
        self.max_s = 0                        # largest |S_k| of a one-sum pass as a plain integer (the cell holds it modulo 2^64)
        self.max_c = 0                        # largest |carry| out of a finished column
        self.at_d = None                      # (form, column) of the largest finished column
        self.red_macs = 0


def kara_pass_bal(form, x, y, mnin, nm, n0inv, st, x2=None, y2=None, kred=False, vf=False, ones=0, dsym=False, trace=None):
    """One pass of kara_pass_bal<FORM, KRED, VF, ONES, DSYM> on signed limb lists; returns (out limbs, quotient limbs).
    dsym (one-sum first pass of a squaring only): the off-diagonal products take the doubled operand (yd, dy2) and go straight
    onto s and e, in 64-bit cells that wrap, instead of a chain of their own that is shifted.  trace: a list that receives the
    carry out of every column."""
    form = int(form)
    sym, dbl, summ = form == SQR, form == SQR2, form == MUL2
    second = dbl or summ
    NL = len(x)
    H = NL // 2
    NP = 2 * H - 1
    assert NL % 2 == 0 and NL <= 36
    i32 = lambda v: -(1 << 31) <= v < (1 << 31)
    for v in list(x) + list(y) + list(x2 or []) + list(y2 or []) + list(mnin) + list(nm):
        assert i32(v)
    nx = [x[i + H] - x[i] for i in range(H)]
    dy = [y[i] - y[i + H] for i in range(H)]
    nx2 = [x2[i + H] - x2[i] for i in range(H)] if summ else [0] * H
    dy2 = [y2[i] - y2[i + H] for i in range(H)] if summ else [2 * d for d in dy]
    yd = [2 * v for v in y]
    ndp = [nm[H + l] - nm[l] for l in range(H)]
    for v in nx + dy + nx2 + dy2 + yd + ndp:
        assert i32(v), "difference or doubled limb leaves int32"
    vbound = (2 if summ else 1) * H << 56
    dbound = (2 if summ else 1) * H << 58

    def smul(a, b, T=1 << 31):
        assert -T <= a < T and -T <= b < T               # two int32: the product fits int64
        return a * b

    def rng(j):
        return (0, j) if j < H else (j - H + 1, H - 1)

    def dot(xx, yy, lo, hi, k):
        """sum of xx[i] yy[k - i] over lo <= i <= hi (the reference sums: plain integers)"""
        return sum(map(int.__mul__, xx[lo:hi + 1], yy[k - hi:k - lo + 1][::-1]))

    def half(o, j):
        s = 0
        lo, hi = rng(j)
        for i in range(lo, hi + 1):
            l = j - i
            if not sym:
                s += smul(x[o + i], y[o + l])
            elif i < l:
                s += smul(x[o + i], yd[o + l])
            elif i == l:
                s += smul(x[o + i], y[o + i])
            if summ:
                s += smul(x2[o + i], y2[o + l])
        assert abs(s) <= vbound, "half-product coefficient beyond its bound"
        return s

    def column(xx, yy, k):
        return dot(xx, yy, max(0, k - NL + 1), min(k, NL - 1), k)

    p0, p2 = [0] * NP, [0] * NP
    pv = [0] * (H + NP)
    ru = [0] * (H + NP)
    dm = [0] * H
    mq, out = [0] * NL, [0] * NL
    carry = 0
    macs = 0
    ones = ones if kred and vf and not summ else 0      # as the kernel: the other passes keep their form
    ss = [0] * (H + NP)                                 # ones: S_k, 64-bit cells

    def finish(k, d, school):
        """The finished column: the schoolbook one, inside a signed 64-bit cell; only now it is shifted.  Returns the carry."""
        assert d == school + (mq[k] * nm[0] if k < NL else 0), (k, d, school)
        assert -(1 << 63) <= d and d + HB < (1 << 63), "finished column leaves int64"
        if abs(d) > st.max_d:
            st.max_d, st.at_d = abs(d), (form, k)
        if k < NL:
            assert -HB <= mq[k] < HB and d % B == 0
            c = d >> RB
        else:
            assert -HB <= out[k - NL] < HB
            c = (d + HB) >> RB
            assert c * B + out[k - NL] == d
        st.max_c = max(st.max_c, abs(c))
        return c

    for k in range(2 * NL - 1):
        mid = H <= k < H + NP
        if ones:
            # every cell below is a 64-bit word that wraps; only the finished column is read as a signed integer
            j = k - H
            s = off = 0
            for o, jj, on in ((0, k, k < NP), (H, j, mid)):
                if not on:
                    continue
                lo, hi = rng(jj)
                for i in range(lo, hi + 1):
                    l = jj - i
                    if dbl:
                        s = (s + smul(x[o + i], yd[o + l])) & M64
                    elif not sym:
                        s = (s + smul(x[o + i], y[o + l])) & M64
                    elif i < l and dsym:
                        s = (s + smul(x[o + i], yd[o + l])) & M64
                    elif i < l:
                        off = (off + smul(x[o + i], y[o + l])) & M64
                    elif i == l:
                        s = (s + smul(x[o + i], y[o + i])) & M64
            if sym and not dsym:
                s = (s + (off << 1)) & M64
            if k < NP:
                lo0, hi0 = (0, k - 1) if k < H else (k - H + 1, H - 1)
                for i in range(lo0, hi0 + 1):
                    if i != k - 1:
                        s = (s + smul(mq[i], nm[k - i])) & M64
                        macs += 1
            if mid:
                lo2, hi2 = rng(j)
                for i in range(lo2, hi2 + 1):
                    if not (i == j and k < NL) and H + i != k - 1:
                        s = (s + smul(mq[H + i], nm[H + j - i])) & M64
                        macs += 1
            newest = 1 <= k <= NL
            nn = 1 if k <= H else H + 1
            if ones == 1 and newest:
                s = (s + smul(mq[k - 1], nm[nn])) & M64
                macs += 1
            e = ss[k - H] if k >= H else 0
            if mid:
                nd = 0
                lo, hi = rng(j)
                for i in range(lo, hi + 1):
                    l = j - i
                    if dbl:
                        e = (e + smul(nx[i], dy2[l])) & M64
                    elif not sym:
                        e = (e + smul(nx[i], dy[l])) & M64
                    elif i < l and dsym:
                        e = (e + smul(nx[i], dy2[l])) & M64
                    elif i < l:
                        nd = (nd + smul(nx[i], dy[l])) & M64
                    elif i == l:
                        e = (e + smul(nx[i], dy[i])) & M64
                if sym and not dsym:
                    e = (e + (nd << 1)) & M64
                for i in range(lo, hi + 1):
                    if i == j and k < NL:
                        e = (e + smul(mq[i], ndp[0])) & M64
                        macs += 1
                    elif H + i != k - 1:
                        e = (e + smul(dm[i], ndp[j - i])) & M64
                        macs += 1
            if second and k < NL:
                e = (e + smul(mnin[k], -1)) & M64
            if H <= k - 1 < NL:
                e = (e + smul(dm[k - 1 - H], ndp[1])) & M64
                macs += 1
            d = (e + s + carry) & M64
            if ones == 2 and newest:
                s = (s + smul(mq[k - 1], nm[nn])) & M64
                d = (d + smul(mq[k - 1], nm[nn])) & M64
                macs += 2
            lo, hi = (0, k - 1) if k < NL else (k - NL + 1, NL - 1)
            want = column(x, y, k)
            school = (2 * want if dbl else want) - (mnin[k] if second and k < NL else 0) + carry + dot(mq, nm, lo, hi, k)
            if k < NL:
                mq[k] = sfield(((d & 0xFFFFFFFF) * n0inv) & 0xFFFFFFFF)
                d = (d + smul(mq[k], nm[0])) & M64
                s = (s + smul(mq[k], nm[0 if k < H else H])) & M64
                macs += 2
                if k >= H:
                    dm[k - H] = mq[k - H] - mq[k]
                    assert i32(dm[k - H])
            else:
                out[k - NL] = sfield(d)
            # S_k on plain integers: [2] V_k + U_k with every quotient digit up to mq[k]; the cell is that modulo 2^64
            s_int = 0
            for o, jj, on in ((0, k, k < NP), (H, j, mid)):
                if on:
                    lo, hi = rng(jj)
                    s_int += (2 if dbl else 1) * dot(x[o:o + H], y[o:o + H], lo, hi, jj) + dot(mq[o:o + H], nm[o:o + H], lo, hi, jj)
            assert s_int & M64 == s, (k, s_int, s)
            st.max_s = max(st.max_s, abs(s_int))
            if k < H + NP:
                ss[k] = s
            else:
                assert s == 0
            carry = finish(k, d - (1 << 64) if d >> 63 else d, school)
            if trace is not None:
                trace.append(carry)
            continue
        t = 0
        if vf:
            vk = off = nd = 0
            for o, jj, on in ((0, k, k < NP), (H, k - H, mid)):
                if not on:
                    continue
                lo, hi = rng(jj)
                for i in range(lo, hi + 1):
                    l = jj - i
                    if not sym:
                        vk += smul(x[o + i], y[o + l])
                    elif i < l:
                        off += smul(x[o + i], y[o + l])
                    elif i == l:
                        vk += smul(x[o + i], y[o + i])
                    if summ:
                        vk += smul(x2[o + i], y2[o + l])
            if sym:
                vk += off << 1
            assert abs(vk) <= vbound, "V_k beyond its bound"
            st.max_v = max(st.max_v, abs(vk))
            if k < H + NP:
                pv[k] = vk
            else:
                assert vk == 0
            t = vk + (pv[k - H] if k >= H else 0)
            if mid:
                j = k - H
                lo, hi = rng(j)
                e = 0
                for i in range(lo, hi + 1):
                    l = j - i
                    if not sym:
                        e += smul(nx[i], dy[l])
                    elif i < l:
                        nd += smul(nx[i], dy[l])
                    elif i == l:
                        e += smul(nx[i], dy[i])
                    if summ:
                        e += smul(nx2[i], dy2[l])
                e += nd << 1
                assert abs(e) < dbound, "-D_j beyond its bound"
                t += e
        else:
            if k < NP:
                p0[k] = half(0, k)
                t += p0[k]
            if mid:
                j = k - H
                p2[j] = half(H, j)
                t += p0[j] + p2[j]
                lo, hi = rng(j)
                e = 0
                for i in range(lo, hi + 1):
                    l = j - i
                    if not sym:
                        e += smul(nx[i], dy[l])
                    elif i < l:
                        e += smul(nx[i], dy2[l])
                    elif i == l:
                        e += smul(nx[i], dy[i])
                    if summ:
                        e += smul(nx2[i], dy2[l])
                assert abs(e) < dbound, "-D_j beyond its bound"
                t += e
            if k >= 2 * H:
                t += p2[k - 2 * H]
        want = column(x, y, k) + (column(x2, y2, k) if summ else 0)
        assert t == want, (k, t, want)
        d = (t << 1) if dbl else t
        if second and k < NL:
            d += smul(mnin[k], -1)
        lo, hi = (0, k - 1) if k < NL else (k - NL + 1, NL - 1)
        school = d + carry + dot(mq, nm, lo, hi, k)
        if not kred:
            macs += hi - lo + 1 + (1 if k < NL else 0)
            d = school
            if k < NL:
                mq[k] = sfield(((d & 0xFFFFFFFF) * n0inv) & 0xFFFFFFFF)
                d += smul(mq[k], nm[0])
            else:
                out[k - NL] = sfield(d)
        else:
            has_u, midr = k < H + NP, H <= k < H + NP
            u = e = 0

            def signed(a, b):
                nonlocal d, e, macs
                pr = smul(a, b)
                e += pr
                assert abs(e) < (H << 58), "partial sum of -E beyond its bound"
                st.max_e = max(st.max_e, abs(e))
                d += pr
                macs += 1

            if k < NP:
                lo0, hi0 = (0, k - 1) if k < H else (k - H + 1, H - 1)
                for i in range(lo0, hi0 + 1):
                    if i != k - 1:
                        u += smul(mq[i], nm[k - i])
                        macs += 1
            if midr:
                j = k - H
                lo2, hi2 = rng(j)
                for i in range(lo2, hi2 + 1):
                    l = j - i
                    if i == j and k < NL:
                        signed(mq[i], ndp[0])
                    elif H + i != k - 1:
                        u += smul(mq[H + i], nm[H + l])
                        macs += 1
                        signed(dm[i], ndp[l])
            if k >= H:
                d += ru[k - H]
            d += carry
            if 1 <= k <= H:
                u += smul(mq[k - 1], nm[1])
                macs += 1
            if H <= k - 1 < NL:
                u += smul(mq[k - 1], nm[H + 1])
                macs += 1
                signed(dm[k - 1 - H], ndp[1])
            if k < H:
                mq[k] = sfield(((((d & 0xFFFFFFFF) + (u & 0xFFFFFFFF)) & 0xFFFFFFFF) * n0inv) & 0xFFFFFFFF)
                u += smul(mq[k], nm[0])
                macs += 1
                d += u
            else:
                if has_u:
                    d += u
                if k < NL:
                    assert d == school, (k, d, school)
                    mq[k] = sfield(((d & 0xFFFFFFFF) * n0inv) & 0xFFFFFFFF)
                    d += smul(mq[k], nm[0])
                    u += smul(mq[k], nm[H])
                    macs += 2
                    dm[k - H] = mq[k - H] - mq[k]
                    assert i32(dm[k - H])
                else:
                    out[k - NL] = sfield(d)
            assert abs(u) <= (H << 56), "U_k beyond its bound"
            st.max_u = max(st.max_u, abs(u))
            if has_u:
                ru[k] = u
            else:
                assert u == 0
        carry = finish(k, d, school)
        if trace is not None:
            trace.append(carry)
    assert i32(carry)
    out[NL - 1] = carry
    st.red_macs = macs
    return out, mq


def _bal_ctx(p, NL):
    return bal_limbs(p, NL), (-pow(p, -1, B)) % B


def mul_kara_bal(al, bl, cl, dl, p, st, red=KMRB_RED):
    """(a, b) * (c, d) -> (w, v) limb lists by mul_kara_reg_bal<red> on balanced limb lists; checks w R = a c + m p and
    v R = a d + b c - m + m' p on the represented integers and the product rule modulo p^2."""
    NL = len(al)
    R = 1 << (RB * NL)
    nm, n0inv = _bal_ctx(p, NL)
    assert value(nm) == p
    w, m = kara_pass_bal(MUL, al, cl, [0] * NL, nm, n0inv, st, kred=bool(red >> MUL & 1), vf=bool(red & VFM), ones=red_ones(red))
    v, m2 = kara_pass_bal(MUL2, al, dl, m, nm, n0inv, st, x2=bl, y2=cl, kred=bool(red >> MUL2 & 1), vf=bool(red & VFS))
    a, b, c, d = value(al), value(bl), value(cl), value(dl)
    W, M, V, M2 = value(w), value(m), value(v), value(m2)
    assert W * R == a * c + M * p
    assert V * R == a * d + b * c - M + M2 * p
    assert 2 * abs(M) <= R + (R >> 28) and 2 * abs(M2) <= R + (R >> 28)
    p2 = p * p
    assert (W + V * p - (a + b * p) * (c + d * p) * pow(R, -1, p2)) % p2 == 0
    return w, v


def sqr_kara_bal(al, bl, p, st, red=KMRB_RED):
    """(a, b)^2 by sqr_kara_reg_bal<red> on balanced limb lists; checks w R = a^2 + m p and v R = 2 a b - m + m' p."""
    NL = len(al)
    R = 1 << (RB * NL)
    nm, n0inv = _bal_ctx(p, NL)
    w, m = kara_pass_bal(SQR, al, al, [0] * NL, nm, n0inv, st, kred=bool(red >> SQR & 1), vf=bool(red & VF), ones=red_ones(red),
                         dsym=bool(red & DSYM))
    v, m2 = kara_pass_bal(SQR2, al, bl, m, nm, n0inv, st, kred=bool(red >> SQR2 & 1), vf=bool(red & VF), ones=red_ones(red))
    a, b = value(al), value(bl)
    W, M, V, M2 = value(w), value(m), value(v), value(m2)
    assert W * R == a * a + M * p
    assert V * R == 2 * a * b - M + M2 * p
    p2 = p * p
    assert (W + V * p - (a + b * p) ** 2 * pow(R, -1, p2)) % p2 == 0
    return w, v


# ---- the second pass of a product in the one-sum form (kara_pass_bal<KARA_MUL2, true, true, ONES>; kernel mode PADIC_LDS_KMRBT
# with PAI_KMRBT_PARTS & 2: the default since profiles/r25/) ----
# v = (x y + x2 y2 - min + m' p) / R with Karatsuba quotient products and ONE stored sum per column: S_k = V_k + U_k, where V_k now
# sums the half products of BOTH pairs (|V_k| <= 2 H 2^56) and -D_(k-H) of both pairs goes onto e, the chain that does not wait for
# the previous column's carry.  Every cell is a 64-bit word that WRAPS; the finished column, read as a signed 64-bit integer, must
# be the schoolbook column, the same integer as in the shipped pass (kara_pass_bal(MUL2, vf=True)), so mq, out and the carries are
# bit for bit the same.  The functions above stay as they are.
KMRBT_RED = KMRBS_RED | 1 << MUL2     # Padic::PADIC_KMRBT_RED: what kernel mode PADIC_LDS_KMRBT runs with PAI_KMRBT_PARTS & 2


def schoolbook_second_pass(x, y, x2, y2, mnin, nm, n0inv):
    """The rule itself on plain integers, column by column: (out, mq, carries) of v = (x y + x2 y2 - min + m' p) / R."""
    NL = len(x)
    mq, out, carries = [0] * NL, [0] * NL, []
    carry = 0
    for k in range(2 * NL - 1):
        lo, hi = max(0, k - NL + 1), min(k, NL - 1)
        d = sum(x[i] * y[k - i] + x2[i] * y2[k - i] for i in range(lo, hi + 1)) + carry
        if k < NL:
            d += sum(mq[i] * nm[k - i] for i in range(k)) - mnin[k]
            mq[k] = sfield(((d & 0xFFFFFFFF) * n0inv) & 0xFFFFFFFF)
            d += mq[k] * nm[0]
            assert d % B == 0
            carry = d >> RB
        else:
            d += sum(mq[i] * nm[k - i] for i in range(k - NL + 1, NL))
            out[k - NL] = sfield(d)
            carry = (d + HB) >> RB
        carries.append(carry)
    out[NL - 1] = carry
    return out, mq, carries


def kara_pass_bal_sum(x, y, x2, y2, mnin, nm, n0inv, st, ones=1):
    """kara_pass_bal<KARA_MUL2, true, true, ONES> in wrapping 64-bit cells: (out limbs, quotient limbs, carries)."""
    NL = len(x)
    H = NL // 2
    NP = 2 * H - 1
    assert NL % 2 == 0 and NL <= 36 and ones in (1, 2)
    i32 = lambda v: -(1 << 31) <= v < (1 << 31)
    assert all(i32(v) for v in list(x) + list(y) + list(x2) + list(y2) + list(mnin) + list(nm))
    nx = [x[i + H] - x[i] for i in range(H)]
    dy = [y[i] - y[i + H] for i in range(H)]
    nx2 = [x2[i + H] - x2[i] for i in range(H)]
    dy2 = [y2[i] - y2[i + H] for i in range(H)]
    ndp = [nm[H + l] - nm[l] for l in range(H)]
    assert all(i32(v) for v in nx + dy + nx2 + dy2 + ndp), "difference limb leaves int32"

    def smul(a, b):
        assert i32(a) and i32(b)
        return a * b

    def rng(j):
        return (0, j) if j < H else (j - H + 1, H - 1)

    mq, out, carries = [0] * NL, [0] * NL, []
    dm = [0] * H
    ss = [0] * (H + NP)
    carry = 0                                            # a 64-bit word: the arithmetic shift of the finished column
    macs = 0
    for k in range(2 * NL - 1):
        mid = H <= k < H + NP
        j = k - H
        s = 0
        for o, jj, on in ((0, k, k < NP), (H, j, mid)):
            if not on:
                continue
            lo, hi = rng(jj)
            for i in range(lo, hi + 1):
                l = jj - i
                s = (s + smul(x[o + i], y[o + l])) & M64
                s = (s + smul(x2[o + i], y2[o + l])) & M64
        if k < NP:
            lo0, hi0 = (0, k - 1) if k < H else (k - H + 1, H - 1)
            for i in range(lo0, hi0 + 1):
                if i != k - 1:
                    s = (s + smul(mq[i], nm[k - i])) & M64
                    macs += 1
        if mid:
            lo2, hi2 = rng(j)
            for i in range(lo2, hi2 + 1):
                if not (i == j and k < NL) and H + i != k - 1:
                    s = (s + smul(mq[H + i], nm[H + j - i])) & M64
                    macs += 1
        newest = 1 <= k <= NL
        nn = 1 if k <= H else H + 1
        if ones == 1 and newest:
            s = (s + smul(mq[k - 1], nm[nn])) & M64
            macs += 1
        e = ss[k - H] if k >= H else 0
        if mid:
            lo, hi = rng(j)
            for i in range(lo, hi + 1):
                l = j - i
                e = (e + smul(nx[i], dy[l])) & M64
                e = (e + smul(nx2[i], dy2[l])) & M64
            for i in range(lo, hi + 1):
                if i == j and k < NL:
                    e = (e + smul(mq[i], ndp[0])) & M64
                    macs += 1
                elif H + i != k - 1:
                    e = (e + smul(dm[i], ndp[j - i])) & M64
                    macs += 1
        if k < NL:
            e = (e + smul(mnin[k], -1)) & M64
        if H <= k - 1 < NL:
            e = (e + smul(dm[k - 1 - H], ndp[1])) & M64
            macs += 1
        d = (e + s + carry) & M64
        if ones == 2 and newest:
            s = (s + smul(mq[k - 1], nm[nn])) & M64
            d = (d + smul(mq[k - 1], nm[nn])) & M64
            macs += 2
        # the schoolbook column without the column's own digit, on plain integers
        lo, hi = max(0, k - NL + 1), min(k, NL - 1)
        school = sum(x[i] * y[k - i] + x2[i] * y2[k - i] for i in range(lo, hi + 1)) - (mnin[k] if k < NL else 0) + _s64(carry)
        school += sum(mq[i] * nm[k - i] for i in (range(k) if k < NL else range(k - NL + 1, NL)))
        assert _s64(d) == school, ("column", k)
        if k < NL:
            mq[k] = sfield(((d & 0xFFFFFFFF) * n0inv) & 0xFFFFFFFF)
            d = (d + smul(mq[k], nm[0])) & M64
            school += mq[k] * nm[0]
            s = (s + smul(mq[k], nm[0 if k < H else H])) & M64
            macs += 2
            if k >= H:
                dm[k - H] = mq[k - H] - mq[k]
                assert i32(dm[k - H])
            assert -HB <= mq[k] < HB and school % B == 0
        else:
            out[k - NL] = sfield(d)
        # the finished column, read as a signed 64-bit integer, is the schoolbook column and lies below 2^63
        assert _s64(d) == school and -(1 << 63) <= school and school + HB < (1 << 63), ("finished column", k)
        if abs(school) > st.max_d:
            st.max_d, st.at_d = abs(school), (MUL2, k)
        if k < H + NP:
            ss[k] = s
        else:
            assert s == 0
        c = (_s64(d) if k < NL else _s64(d) + HB) >> RB
        st.max_c = max(st.max_c, abs(c))
        carries.append(c)
        carry = c & M64
    assert i32(_s64(carry))
    out[NL - 1] = _s64(carry)
    st.red_macs = macs
    return out, mq, carries


def mul_kara_bal_stage(al, bl, cl, dl, p, st, red=KMRBT_RED):
    """(a, b) * (c, d) -> (w, v) limb lists as kernel mode PADIC_LDS_KMRBT forms them (mul_kara_lds_bal<PADIC_KMRBT_RED>): the
    first pass of mul_kara_bal, the second by kara_pass_bal_sum; the relations of mul_kara_bal."""
    assert red & (1 << MUL2) and red_ones(red)
    NL = len(al)
    R = 1 << (RB * NL)
    nm, n0inv = _bal_ctx(p, NL)
    assert value(nm) == p
    w, m = kara_pass_bal(MUL, al, cl, [0] * NL, nm, n0inv, st, kred=True, vf=True, ones=red_ones(red))
    v, m2, _ = kara_pass_bal_sum(al, dl, bl, cl, m, nm, n0inv, st, ones=red_ones(red))
    a, b, c, d = value(al), value(bl), value(cl), value(dl)
    W, M, V, M2 = value(w), value(m), value(v), value(m2)
    assert W * R == a * c + M * p
    assert V * R == a * d + b * c - M + M2 * p
    assert 2 * abs(M) <= R + (R >> 28) and 2 * abs(M2) <= R + (R >> 28)
    p2 = p * p
    assert (W + V * p - (a + b * p) * (c + d * p) * pow(R, -1, p2)) % p2 == 0
    return w, v


def in_lazy_range(l, p):
    """The invariant of the balanced engine: |value| < 0.51 p."""
    return 100 * abs(value(l)) < 51 * p


def run_bal(rounds=1, seed=2):
    rng = random.Random(seed)
    st = BalStats()
    for bits, NL in ((1024, 36), (768, 36), (600, 24)):
        H = NL // 2
        for _ in range(rounds):
            p = random_prime(bits, rng)
            lo, hi = [-HB] * NL, [HB - 1] * NL
            alt = [(-HB if (i // H + i) % 2 else HB - 1) for i in range(NL)]
            cs = [lo, hi, alt, [-v - 1 for v in alt], bal_limbs(51 * p // 100, NL), bal_limbs(-(51 * p // 100), NL), bal_limbs(0, NL)]
            cs += [bal_limbs(rng.randrange(-p // 2, p // 2), NL) for _ in range(3)]
            for red in (0, 15 | VF | VFM | VFS, KMRB_RED, KMRBS_RED, KMRBS_RED | ONES2):
                for i, a in enumerate(cs):
                    b, c, d = cs[(i + 1) % len(cs)], cs[(i + 3) % len(cs)], cs[(i + 5) % len(cs)]
                    sqr_kara_bal(a, b, p, st, red)
                    mul_kara_bal(a, b, c, d, p, st, red)
            a, b = cs[4], cs[5]
            c, d = cs[-1], cs[-2]
            for _ in range(6):
                a, b = sqr_kara_bal(a, b, p, st)
                a, b = mul_kara_bal(a, b, c, d, p, st)
                assert in_lazy_range(a, p) and in_lazy_range(b, p)
    return st


# ---- (a, b) * (c, 0) beyond 36 limbs in two half-width steps (csrc/mont_padic.hpp: kara2_step_bal, mul_kara2_c0_bal) --------
# X = 2^(29 HL), HL = NL / 2, R = X^2, c = c0 + c1 X:
#     w:  T = (a c0 + q0 n) / X          w = (T + a c1 + q1 n) / X
#     v:  S = (b c0 - q0 + q0' n) / X    v = (S + b c1 - q1 + q1' n) / X
# One step is NL + HL - 1 columns; its four HL x HL products (x_lo c_h, q_h n_lo at column 0; x_hi c_h, q_h n_hi at column HL)
# are split at H = HL / 2 and share ONE stored sum S_k per column, kept in a 64-bit cell that WRAPS.  The model asserts that every
# finished column, read as a signed 64-bit integer, is the exact schoolbook column of the step, and records the largest one.
class Kara2Stats:
    def __init__(self):
        self.max_d = 0                        # largest |finished column|
        self.max_c = 0                        # largest |carry|
        self.at_d = None                      # (second, has_tin, column) of the largest column
        self.macs = 0                         # multiply-adds of the last step
        self.q_ext = set()                    # extreme quotient digits met: -2^28, 2^28 - 1


def _s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def kara2_step_bal(x, ch, tin, qin, nm, n0inv, st, second, has_tin):
    """One step of kara2_step_bal on signed limb lists: (out limbs, quotient digits).  second: the v stream (qsel = -1, qin the
    first quotient's digits); has_tin: the second step of a stream (tin the first step's result, else zero)."""
    NL = len(x)
    assert NL % 4 == 0 and NL <= 72 and len(ch) == NL // 2 and len(nm) == NL
    HL, H = NL // 2, NL // 4
    NP = 2 * H - 1
    NU, NK = HL + H + NP, NL + HL - 1
    i32 = lambda v: -(1 << 31) <= v < (1 << 31)
    nx = [x[H + i] - x[i] for i in range(H)] + [x[HL + H + i] - x[HL + i] for i in range(H)]
    dy = [ch[i] - ch[H + i] for i in range(H)]
    ndp = [nm[H + l] - nm[l] for l in range(H)] + [nm[HL + H + l] - nm[HL + l] for l in range(H)]
    assert all(i32(v) for v in nx + dy + ndp)
    dm = [None] * H
    q = [None] * HL
    out = [None] * NL
    ss = [None] * NU
    carry = 0
    macs = 0
    lo_of = lambda j: 0 if j < H else j - H + 1
    hi_of = lambda j: j if j < H else H - 1

    def smul(a, b):
        nonlocal macs
        assert i32(a) and i32(b)
        macs += 1
        return a * b

    for k in range(NK):
        kh = k - HL
        s = 0
        for o in (0, 1):
            c, xo = (kh, HL) if o else (k, 0)
            if 0 <= c < NP:
                for i in range(lo_of(c), hi_of(c) + 1):
                    s += smul(x[xo + i], ch[c - i])
            if c >= H and c - H < NP:
                j = c - H
                for i in range(lo_of(j), hi_of(j) + 1):
                    s += smul(x[xo + H + i], ch[H + j - i])
        if 0 <= kh < NP:
            for i in range(lo_of(kh), hi_of(kh) + 1):
                s += smul(q[i], nm[HL + kh - i])
        if kh >= H and kh - H < NP:
            j = kh - H
            for i in range(lo_of(j), hi_of(j) + 1):
                s += smul(q[H + i], nm[HL + H + j - i])
        if k < NP:
            for i in range(lo_of(k), hi_of(k) + 1):
                if i < k:
                    s += smul(q[i], nm[k - i])
        if k >= H and k - H < NP:
            j = k - H
            for i in range(lo_of(j), hi_of(j) + 1):
                if not (i == j and k < HL):
                    s += smul(q[H + i], nm[H + j - i])
        s &= M64
        e = ss[k - H] if k >= H else 0
        for o in (0, 1):
            j = (kh if o else k) - H
            if 0 <= j < NP:
                for i in range(lo_of(j), hi_of(j) + 1):
                    e += smul(nx[o * H + i], dy[j - i])
                for i in range(lo_of(j), hi_of(j) + 1):
                    if o == 0 and i == j and k < HL:
                        e += smul(q[i], ndp[0])
                    else:
                        e += smul(dm[i], ndp[o * H + j - i])
        # one body serves all four steps: the carried-in digit (zero in the first step of a stream) is one multiply-add by a
        # run-time 1, the first quotient's digit one by qsel = -1 (v stream) or 0 (w stream)
        if k < NL:
            e += smul(tin[k] if has_tin else 0, 1)
        if k < HL:
            e += smul(qin[k] if second else 0, -1 if second else 0)
        d = (e + s + carry) & M64
        # the exact schoolbook column of the step without the column's own digit
        col = sum(x[i] * ch[k - i] for i in range(NL) if 0 <= k - i < HL)
        col += sum(q[i] * nm[k - i] for i in range(min(k, HL)) if 0 <= k - i < NL)
        col += (tin[k] if has_tin and k < NL else 0) - (qin[k] if second and k < HL else 0) + _s64(carry)
        assert _s64(d) == col, ("column", k)
        if k < HL:
            q[k] = sfield(d * n0inv)
            if q[k] in (-HB, HB - 1):
                st.q_ext.add(q[k])
            d = (d + smul(q[k], nm[0])) & M64
            col += q[k] * nm[0]
            assert _s64(d) == col and col % B == 0
            if k < H:
                s = (s + smul(q[k], nm[0])) & M64
            else:
                s = (s + smul(q[k], nm[H])) & M64
                dm[k - H] = q[k - H] - q[k]
                assert i32(dm[k - H])
        else:
            out[k - HL] = sfield(d)
        if abs(col) > st.max_d:
            st.max_d, st.at_d = abs(col), (second, has_tin, k)
        assert abs(col) < 1 << 63
        if k < NU:
            ss[k] = s
        carry = (_s64(d) if k < HL else _s64(d) + HB) >> RB
        st.max_c = max(st.max_c, abs(carry))
        carry &= M64
    out[NL - 1] = _s64(carry)
    assert i32(out[NL - 1])
    st.macs = macs
    return out, q


def balance_halves(u):
    """Padic::balance_half on both halves of an entry's unsigned limbs: the balanced digits of the same integer."""
    NL = len(u)
    r, cy = [], 0
    for j in range(NL):
        t = u[j] + cy
        assert -(1 << 31) <= t + HB < (1 << 31)
        r.append(sfield(t))
        cy = (t + HB) >> RB
    r[NL - 1] += cy << RB
    assert -(1 << 31) <= r[-1] < (1 << 31)
    return r


def mul_kara2_c0_bal(al, bl, cl, n, st, check=True):
    """(a, b) * (c, 0) -> (w, v, m digits, m' digits) by mul_kara2_c0_bal on balanced limb lists; with `check` the one-step
    rule in CPython: w R = a c + m n, v R = b c - m + m' n, the same balanced quotients, and the product rule modulo n^2."""
    NL = len(al)
    HL = NL // 2
    R = 1 << (RB * NL)
    nm, n0inv = _bal_ctx(n, NL)
    assert value(nm) == n
    c0, c1 = cl[:HL], cl[HL:]
    t, q0 = kara2_step_bal(al, c0, None, None, nm, n0inv, st, False, False)
    w, q1 = kara2_step_bal(al, c1, t, None, nm, n0inv, st, False, True)
    s, q2 = kara2_step_bal(bl, c0, None, q0, nm, n0inv, st, True, False)
    v, q3 = kara2_step_bal(bl, c1, s, q1, nm, n0inv, st, True, True)
    m, m2 = q0 + q1, q2 + q3
    if check:
        a, b, c = value(al), value(bl), value(cl)
        W, M, V, M2 = value(w), value(m), value(v), value(m2)
        Mref = one_step_quotient(a * c, n, NL)
        assert M == Mref and W * R == a * c + M * n
        M2ref = one_step_quotient(b * c - M, n, NL)
        assert M2 == M2ref and V * R == b * c - M + M2 * n
        n2 = n * n
        assert (W + V * n - (a + b * n) * c * pow(R, -1, n2)) % n2 == 0
    return w, v, m, m2


def one_step_quotient(z, n, NL):
    """The balanced quotient of the one-step rule: m == -z / n (mod R) with every digit in [-2^28, 2^28)."""
    R = 1 << (RB * NL)
    m = (-z * pow(n, -1, R)) % R
    digs = []
    for _ in range(NL):
        r = sfield(m)
        digs.append(r)
        m = (m - r) >> RB
    return value(digs)


def run_kara2(rounds=1, seed=3, NL=72, bits=2048):
    rng = random.Random(seed)
    st = Kara2Stats()
    for _ in range(rounds):
        n = random_prime(bits // 2, rng) * random_prime(bits - bits // 2, rng)
        lo, hi = [-HB] * NL, [HB - 1] * NL
        cs = [lo, hi, bal_limbs(51 * n // 100, NL), bal_limbs(-(51 * n // 100), NL), bal_limbs(0, NL)]
        cs += [bal_limbs(rng.randrange(-n // 2, n // 2), NL) for _ in range(2)]
        for i, a in enumerate(cs):
            b, c = cs[(i + 1) % len(cs)], cs[(i + 3) % len(cs)]
            mul_kara2_c0_bal(a, b, c, n, st)
    return st


def random_prime(bits, rng):
    while True:
        c = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if all(c % q for q in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)) and pow(2, c - 1, c) == 1:
            return c


def corners(p, NL, rng):
    """Digit pairs at the extremes: all limbs 2^29 - 1, the lazy bound 2p + eps, zero, opposite-sign differences."""
    R = 1 << (RB * NL)
    H = NL // 2
    top = 2 * p + (p >> 18)                       # 2p + eps: the lazy bound of the engine (R / p >= 2^20)
    ones = R - 1
    lo_hi = value([MASK] * H + [0] * H)           # x0 all ones, x1 zero: every difference +(2^29 - 1)
    hi_lo = value([0] * H + [MASK] * H)           # every difference -(2^29 - 1)
    alt = value([MASK if (i // H + i) % 2 else 0 for i in range(NL)])
    out = [(ones, ones, False), (lo_hi, hi_lo, False), (hi_lo, lo_hi, False), (alt, ones - alt, False),
           (top - 1, top - 1, True), (top - 1, 0, True), (0, top - 1, True), (p - 1, p - 1, True), (1, 0, True), (0, 0, True)]
    for _ in range(4):
        out.append((rng.randrange(top), rng.randrange(top), True))
    return out


def run(rounds=2, seed=1, red=0):
    rng = random.Random(seed)
    st = Stats()
    for bits, NL in ((1024, 36), (1000, 36), (600, 24)):
        for _ in range(rounds):
            p = random_prime(bits, rng)
            cs = corners(p, NL, rng)
            for a, b, ok in cs:
                sqr_kara(a, b, p, NL, st, in_range=ok, red=red)
            for i, (a, b, ok) in enumerate(cs):          # products: every corner against itself, its neighbour, its mirror
                for c, d, ok2 in (cs[i], cs[(i + 1) % len(cs)], (b, a, ok)):
                    mul_kara(a, b, c, d, p, NL, st, in_range=ok and ok2, red=red)
        # a run of squarings stays inside the lazy bound
        p = random_prime(bits, rng)
        a, b = rng.randrange(2 * p), rng.randrange(2 * p)
        for _ in range(8):
            a, b = sqr_kara(a, b, p, NL, st, red=red)
            assert a < 2 * p + (p >> 18) and b < 2 * p + (p >> 18)
        # ... and so does a run of products by a fixed element (the table build)
        c, d = rng.randrange(2 * p), rng.randrange(2 * p)
        for _ in range(8):
            a, b = mul_kara(a, b, c, d, p, NL, st, red=red)
            assert a < 2 * p + (p >> 18) and b < 2 * p + (p >> 18)
    return st


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    s = run(rounds)
    run(rounds, red=KMR_RED)
    r = run(rounds, red=15 | VF | VFM)
    print({"red_max_rq_log2": r.max_rq.bit_length(), "red_max_e_log2": r.max_red_e.bit_length(), "red_max_d_log2": r.max_d.bit_length()})
    bst = run_bal(rounds)
    print({"bal_max_d_log2": bst.max_d.bit_length(), "bal_max_v_log2": bst.max_v.bit_length(), "bal_max_u_log2": bst.max_u.bit_length(),
           "bal_max_e_log2": bst.max_e.bit_length(), "bal_red_macs": bst.red_macs})
    k2 = run_kara2(rounds)
    print({"kara2_max_col_log2": k2.max_d.bit_length(), "kara2_at": k2.at_d, "kara2_max_carry_log2": k2.max_c.bit_length(),
           "kara2_macs_last_step": k2.macs})
    print({"max_col_log2": s.max_col.bit_length(), "max_cc_log2": s.max_cc.bit_length(),
           "max_d_log2": s.max_d.bit_length(), "max_running_log2": s.max_run.bit_length(), "max_mid_cell_log2": s.max_e.bit_length()})
