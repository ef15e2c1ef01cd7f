"""Cell-exact model of the register-resident Karatsuba squaring and product of the digit-pair engine (csrc/mont_padic.hpp:
kara_pass, sqr_kara, mul_kara_reg).

It follows kara_pass column by column: 32-bit signed difference limbs, signed 64-bit limb products, the product column X_k
accumulated modulo 2^64, its carry stream cc and the reduction column d.  Beside every 64-bit cell it keeps the unbounded
value and records the largest one, and it asserts that
  - every difference limb fits int32 and every signed product int64,
  - X_k (accumulated modulo 2^64) equals the schoolbook column sum_i x_i y_(k-i) exactly,
  - cc, d and the carries never reach 2^64,
  - w = (a^2 + m p) / R and v = (2 a b - m + R p + m' p) / R exactly, and w + v p == (a + b p)^2 R^-1 (mod p^2),
  - for a product: the summed half products of a d + b c fit 64 bits, their signed difference part fits int64, the middle
    part is non-negative and enters through a 128-bit cell, and w, v are those of the row-wise product rule.
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


SQR, SQR2, MUL, MUL2 = 0, 1, 2, 3     # kara_pass<FORM>: KARA_SQR, KARA_SQR2, KARA_MUL, KARA_MUL2


def kara_pass(form, x, y, mnin, nm, n0inv, st, x2=None, y2=None):
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
    cc = carry = 0
    mq = [0] * NL
    out = [0] * NL
    for k in range(2 * NL - 1):
        t = 0            # unbounded running value; the cell holds t mod 2^64
        nd = [0, 0]      # MUL2: -D_j of either pair, two signed 64-bit cells (their sum can pass 2^63)
        mid = H <= k < H + NP
        if k < NP:
            p0[k] = half(0, k)
            t += p0[k]
        if mid:
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
        if k >= 2 * H:
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
        for i in range(lo, hi + 1):
            if i != k - 1:
                d += mq[i] * nm[k - i]
        d += carry
        if 1 <= k and k - 1 < NL:
            d += mq[k - 1] * nm[1]
        if k < NL:
            mq[k] = ((d & 0xFFFFFFFF) * n0inv) & MASK
            d += mq[k] * nm[0]
        else:
            out[k - NL] = d & MASK
        assert d <= M64, "reduction column wraps"
        st.max_d = max(st.max_d, d)
        carry = d >> RB
    top = carry + (cc << 1 if dbl else cc) + (nm[NL - 1] if second else 0)
    assert top <= 0xFFFFFFFF
    out[NL - 1] = top          # unmasked here: the caller checks that it fits 29 bits where the digits are in range
    return out, mq


def mul_kara(a, b, c, d, p, NL, st, in_range=True):
    """(a, b) * (c, d) -> (w, v) by the two product passes (mul_kara_reg); checks them against the row-wise product rule
    w = (a c + m p) / R, v = (a d + b c - m + R p + m' p) / R on Python integers (m, m' the unique quotients modulo R)."""
    R = 1 << (RB * NL)
    nm = limbs(p, NL)
    n0inv = (-pow(p, -1, B)) % B
    al, bl, cl, dl = limbs(a, NL), limbs(b, NL), limbs(c, NL), limbs(d, NL)
    assert (value(al), value(bl), value(cl), value(dl)) == (a, b, c, d)
    w, m = kara_pass(MUL, al, cl, [0] * NL, nm, n0inv, st)
    v, m2 = kara_pass(MUL2, al, dl, m, nm, n0inv, st, x2=bl, y2=cl)
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


def sqr_kara(a, b, p, NL, st, in_range=True):
    """(a, b) -> (w, v) by the two passes; checks the exact relations."""
    R = 1 << (RB * NL)
    nm = limbs(p, NL)
    n0inv = (-pow(p, -1, B)) % B
    al, bl = limbs(a, NL), limbs(b, NL)
    assert value(al) == a and value(bl) == b
    w, m = kara_pass(False, al, al, [0] * NL, nm, n0inv, st)
    v, m2 = kara_pass(True, al, bl, m, nm, n0inv, st)
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


def run(rounds=2, seed=1):
    rng = random.Random(seed)
    st = Stats()
    for bits, NL in ((1024, 36), (1000, 36), (600, 24)):
        for _ in range(rounds):
            p = random_prime(bits, rng)
            cs = corners(p, NL, rng)
            for a, b, ok in cs:
                sqr_kara(a, b, p, NL, st, in_range=ok)
            for i, (a, b, ok) in enumerate(cs):          # products: every corner against itself, its neighbour, its mirror
                for c, d, ok2 in (cs[i], cs[(i + 1) % len(cs)], (b, a, ok)):
                    mul_kara(a, b, c, d, p, NL, st, in_range=ok and ok2)
        # a run of squarings stays inside the lazy bound
        p = random_prime(bits, rng)
        a, b = rng.randrange(2 * p), rng.randrange(2 * p)
        for _ in range(8):
            a, b = sqr_kara(a, b, p, NL, st)
            assert a < 2 * p + (p >> 18) and b < 2 * p + (p >> 18)
        # ... and so does a run of products by a fixed element (the table build)
        c, d = rng.randrange(2 * p), rng.randrange(2 * p)
        for _ in range(8):
            a, b = mul_kara(a, b, c, d, p, NL, st)
            assert a < 2 * p + (p >> 18) and b < 2 * p + (p >> 18)
    return st


if __name__ == "__main__":
    s = run(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
    print({"max_col_log2": s.max_col.bit_length(), "max_cc_log2": s.max_cc.bit_length(),
           "max_d_log2": s.max_d.bit_length(), "max_running_log2": s.max_run.bit_length(), "max_mid_cell_log2": s.max_e.bit_length()})
