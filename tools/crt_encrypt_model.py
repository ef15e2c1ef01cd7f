"""Python-int model of the owner-side CRT encryption (csrc/dispatch_encrypt_crt.hpp), step by step, with the ranges the kernels
rely on asserted:

  1. hs_s = hs mod s^2 for s = p, q                                   (host, table-build time)
  2. o_s  = hs_s^r mod s^2                                            (k_encrypt_padic with the context of s, all-zero message)
  3. Garner lift (k_crt_lift): h = (o_q - o_p) * (p^-2 mod q^2) mod q^2,  o = o_p + p^2 h = hs^r mod n^2
  4. ct = (1 + m n) * o mod n^2   [apply_obfuscator: ct * o]          (k_encrypt, the obfuscator-given modes)

The message factor joins AFTER the lift (one pass of products modulo n^2); `fold` below is the per-prime alternative the issue
describes, 1 + m n == 1 + (m s' mod s) s (mod s^2), kept as a cross-check of the same identity.

    python tools/crt_encrypt_model.py            # self-check on a small key
"""
from __future__ import annotations

RB = 29


def enc_nl(prime_bits: int) -> int:
    """limbs of the encryption digit engine for a prime of this width (csrc/padic_enc_kernels.hip: padic_enc_nl_for_n_bits)"""
    if prime_bits >= 700 and RB * 36 >= prime_bits + 20:
        return 36
    if prime_bits >= 1400 and RB * 72 >= prime_bits + 20:
        return 72
    return 0


def lift_nl(q2_bits: int) -> int:
    """limbs of the lane-group geometry of q^2 (geo_for_bits: R = 2^(29 NL) > 4 q^2)"""
    for nl in (36, 72, 112, 144, 224, 288):
        if RB * nl >= q2_bits + 2:
            return nl
    return 0


def constants(p: int, q: int, hs: int) -> dict:
    if p > q:
        p, q = q, p
    p2, q2 = p * p, q * q
    x = pow(p, -1, q)
    pinv = x * (2 - p * x) % q2                      # one Hensel step from p^-1 mod q
    assert p * pinv % q2 == 1
    pinv2 = pinv * pinv % q2
    assert p2 * pinv2 % q2 == 1 and pinv2 == pow(p2, -1, q2)
    return {"p": p, "q": q, "p2": p2, "q2": q2, "pinv2": pinv2, "hs_p": hs % p2, "hs_q": hs % q2}


def half_pow(c: dict, r: int):
    """step 2: the two half-width exponentiations, canonical residues"""
    assert r >= 0
    op, oq = pow(c["hs_p"], r, c["p2"]), pow(c["hs_q"], r, c["q2"])
    assert 0 <= op < c["p2"] < c["q2"] and 0 <= oq < c["q2"]
    return op, oq


def lift(c: dict, op: int, oq: int, nl: int = 0) -> int:
    """step 3 as k_crt_lift computes it; nl: limbs of the lift's geometry (0: chosen from q^2)"""
    q2, p2 = c["q2"], c["p2"]
    nl = nl or lift_nl(q2.bit_length())
    R = 1 << (RB * nl)
    assert nl and R > 4 * q2                              # lazy operands below 2 q^2, no subtraction between products
    d = oq - op + q2
    assert 0 < d < 2 * q2                                 # p < q: o_p < p^2 < q^2
    h = d * c["pinv2"] % q2
    x = op + p2 * h
    assert 0 <= x < p2 * q2 and x < R * R                 # canonical as it stands; fits the 2 NL limbs the kernel writes from
    return x


def fold(c: dict, m: int, n: int):
    """(1, m s' mod s): the plain base-s digit pair of 1 + m n modulo s^2, for s = p and s = q"""
    p, q = c["p"], c["q"]
    fp, fq = m * q % p, m * p % q
    assert (1 + fp * p) % c["p2"] == (1 + m * n) % c["p2"] and (1 + fq * q) % c["q2"] == (1 + m * n) % c["q2"]
    return fp, fq


def obfuscator(c: dict, r: int) -> int:
    return lift(c, *half_pow(c, r))


def encrypt(p: int, q: int, hs: int, m: int, r: int) -> int:
    c = constants(p, q, hs)
    n = c["p"] * c["q"]
    nsq = n * n
    o = obfuscator(c, r)
    assert o == pow(hs, r, nsq)
    ct = (1 + m * n) % nsq * o % nsq
    # the per-prime fold reaches the same residues
    fp, fq = fold(c, m, n)
    op, oq = half_pow(c, r)
    assert ct % c["p2"] == (1 + fp * c["p"]) * op % c["p2"] and ct % c["q2"] == (1 + fq * c["q"]) * oq % c["q2"]
    return ct


def apply_obfuscator(p: int, q: int, hs: int, ct: int, r: int) -> int:
    c = constants(p, q, hs)
    n = c["p"] * c["q"]
    return ct * obfuscator(c, r) % (n * n)


if __name__ == "__main__":
    P, Q = (1 << 89) - 1, (1 << 107) - 1
    N = P * Q
    HS = pow(0x1234567, 2 * N, N * N)
    for m_, r_ in ((0, 0), (1, 1), (N - 1, (1 << 60) - 1), (P, 12345)):
        assert encrypt(P, Q, HS, m_, r_) == (1 + m_ * N) * pow(HS, r_, N * N) % (N * N)
    print("crt_encrypt_model: ok")
