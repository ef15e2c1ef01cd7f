"""Steered ciphertexts for the 36-limb digit-pair decrypt kernel (csrc/kernels_padic.hpp: k_dec_a_padic in the balanced modes)
and the kernel's steps on the cell-exact model (tools/kara_model.py).

In the balanced modes every result digit satisfies |w|, |v| < 0.51 s (csrc/mont_padic.hpp, the invariant above kara_pass_bal),
so a pair with |w|, |v| < 0.49 s is the ONLY pair of its residue w + v s (mod s^2) the kernel can hold.  After schedule entry k
the kernel holds c^(e_k) R mod s^2, e_k the (odd) prefix of s - 1 the sliding-window schedule has consumed; where
gcd(e_k, s (s - 1)) = 1 the e_k-th root of any unit exists and is unique, so
    c_s = ((w* + v* s) R^-1) ^ (e_k^-1 mod s (s - 1))  mod s^2
puts the chosen limbs (w*, v*) into the kernel's registers, and the squarings of entry k + 1 start from them.  Targets with
all free limbs at +-2^28 drive the columns of that squaring to within a factor 1.6 of the bound 36 (2^57 + 2^56) that the
one-cell-per-column design rests on; real encryptions and random residues stay a factor six below it."""
import math

from tests.test_codec_keys_cpu import schedule_value, sliding_schedule
from tests.test_padic_kred_cpu import km

NL = 36
H = NL // 2
RBITS = km.RB * NL
R = 1 << RBITS
HB = km.HB
TBL_ENTRIES = 32                     # csrc/geo_ops.hpp: PADIC_TBL_ENTRIES = 2^(PADIC_SLIDE_BITS - 1)
FAR_STEP = 16                        # a first usable step beyond this: one target pair through the model only


def free_limbs(s):
    """Target limbs that may sit at an extreme with |w*| < 0.49 s left: 35 at 1024-bit primes, 26 at 768 bits."""
    return 35 if s.bit_length() > 1015 else 26


def targets(free):
    """{name: balanced limb list}, the top NL - free limbs zero."""
    pad = [0] * (NL - free)
    lo, hi = [-HB] * free + pad, [HB - 1] * free + pad
    alt = [(-HB if i & 1 else HB - 1) for i in range(free)] + pad        # odd columns of a^2: every product negative
    lower = (free + 1) // 2                                              # 18 = H of 35: nx = a[H + i] - a[i] at +(2^29 - 1)
    half = [-HB] * lower + [HB - 1] * (free - lower) + pad               # (13 of 26: the columns through both halves keep one sign)
    mirror = lambda l: [-v - 1 for v in l[:free]] + pad
    return {"LO": lo, "HI": hi, "ALT": alt, "ALT_M": mirror(alt), "HALF": half, "HALF2": mirror(half)}


PAIRS = (("LO", "LO"), ("HI", "LO"), ("LO", "HI"), ("ALT", "ALT"), ("ALT", "ALT_M"), ("HALF", "HALF2"))


def target_pairs(s):
    t = targets(free_limbs(s))
    out = [(a + "," + b, t[a], t[b]) for a, b in PAIRS]
    for _, w, v in out:
        assert 100 * abs(km.value(w)) < 49 * s and 100 * abs(km.value(v)) < 49 * s
    return out


def usable_steps(s):
    """[(k, e_k)]: schedule entries k >= 1 of s - 1 that end in a product, are followed by at least one squaring and whose
    consumed exponent e_k is invertible modulo the group order s (s - 1)."""
    ops = sliding_schedule(s - 1)
    out = []
    for k in range(1, len(ops) - 1):
        if ops[k][1] == 0xFF or ops[k + 1][0] < 1:
            continue
        e = schedule_value(ops[:k + 1])
        if math.gcd(e, s * (s - 1)) == 1:
            out.append((k, e))
    return out


def steer(s, target_w, target_v):
    """(c_s, k, e_k): the residue modulo s^2 after whose schedule entry k (the smallest usable one) the kernel's registers hold
    the limbs (target_w, target_v); None where no entry is usable."""
    steps = usable_steps(s)
    if not steps:
        return None
    k, e = steps[0]
    s2 = s * s
    W, V = km.value(target_w), km.value(target_v)
    assert 0 < abs(W) and 100 * abs(W) < 49 * s and 100 * abs(V) < 49 * s     # a unit, and the only pair of its residue
    x = (W + V * s) * pow(R, -1, s2) % s2
    c = pow(x, pow(e, -1, s * (s - 1)), s2)
    assert pow(c, e, s2) == x
    return c, k, e


def crt(a, b, p2, q2):
    return (a + p2 * ((b - a) * pow(p2, -1, q2) % q2)) % (p2 * q2)


def prime_of(key, which):
    return (key.p, key.q)[which]


def steered_ciphertext(key, which, target_w, target_v, rng):
    """A ciphertext modulo n^2 that is steered modulo prime `which` squared and a random unit modulo the other's; None if
    that prime has no usable step.  It is a unit, so the oracle defines its decryption."""
    s, o = prime_of(key, which), prime_of(key, 1 - which)
    got = steer(s, target_w, target_v)
    if got is None:
        return None
    u = rng.randrange(1, o * o)
    while u % o == 0:
        u = rng.randrange(1, o * o)
    c = crt(got[0], u, s * s, o * o)
    assert c % (s * s) == got[0] and math.gcd(c, key.n) == 1
    return c


# ---- the kernel's steps on the model ----------------------------------------------------------------------------------------
def entry_pair(s, c, ct_bits):
    """csrc/kernels_padic.hpp: padic_to_digit_form — the sum over the base-R digits c_i of the ciphertext of the row-wise
    products (c_i, 0) * digits(R^(i+2) mod s^2), w_i = (c_i ka + m s) / R, v_i = (c_i kb - m + R s + m' s) / R, no final
    subtraction; then to_balanced.  Returns balanced limb lists."""
    s2 = s * s
    sinv = pow(s, -1, R)
    nd = (ct_bits + RBITS - 1) // RBITS
    assert c < 1 << ct_bits
    K = R * R % s2
    sw = sv = 0
    for i in range(nd):
        ci = (c >> (RBITS * i)) & (R - 1)
        ka, kb = K % s, K // s
        m = -ci * ka * sinv % R
        w, r = divmod(ci * ka + m * s, R)
        assert r == 0
        t = ci * kb - m + R * s
        v, r = divmod(t + (-t * sinv % R) * s, R)
        assert r == 0
        sw, sv = sw + w, sv + v
        K = K * R % s2
    assert (sw + sv * s - c * R) % s2 == 0 and sw < R >> 1 and sv < R >> 1
    return km.to_balanced(km.limbs(sw, NL)), km.to_balanced(km.limbs(sv, NL))


def canonical_pair(s, c):
    x = c * R % (s * s)
    return km.to_balanced(km.limbs(x % s, NL)), km.to_balanced(km.limbs(x // s, NL))


def model_chain(s, c, upto_k, stats, red, ct_bits=None, canonical=False):
    """The steps of k_dec_a_padic in the balanced modes on tools/kara_model.py: digit-form entry (or, canonical=True, the
    canonical Montgomery pair of c), base^2, the odd powers base^(2i+1) up to the largest index that schedule entries
    0 .. upto_k read (the kernel builds all of them, in this order), then schedule entries 1 .. upto_k.
    Returns (a, b, trace): the registers after entry upto_k and [(kind, a, b)] of every squaring / product in order."""
    ops = sliding_schedule(s - 1)
    assert 0 <= upto_k < len(ops) and ops[0][0] == 0
    a, b = canonical_pair(s, c % (s * s)) if canonical else entry_pair(s, c, ct_bits)
    trace = []

    def sqr(a, b):
        a, b = km.sqr_kara_bal(a, b, s, stats, red)
        trace.append(("sqr", a, b))
        return a, b

    def mul(a, b, c_, d_):
        a, b = km.mul_kara_bal(a, b, c_, d_, s, stats, red)
        trace.append(("mul", a, b))
        return a, b

    need = max(idx for _, idx in ops[:upto_k + 1] if idx != 0xFF)
    assert need < TBL_ENTRIES
    table = [(a, b)]
    b2 = sqr(a, b)
    for _ in range(need):
        table.append(mul(*table[-1], *b2))
    a, b = table[ops[0][1]]
    for nsq, idx in ops[1:upto_k + 1]:
        for _ in range(nsq):
            a, b = sqr(a, b)
        if idx != 0xFF:
            a, b = mul(a, b, *table[idx])
    return a, b, trace


def next_squaring(s, a, b, red):
    """The first squaring of the entry that follows, from the registers (a, b): (largest |column|, largest |carry|, where)."""
    st = km.BalStats()
    km.sqr_kara_bal(a, b, s, st, red)
    return st.max_d, st.max_c, st.at_d
