"""Generates tests/golden/limit_keys.json: prime pairs whose n^2 sits at the limit of the Montgomery geometry it lives on.  The
lane-group engine keeps lazy residues in [0, 2M), M = n^2, between products, which is sound because R = 2^(29 NL) >= 4M
(csrc/paillier_capi.hip: geo_for_bits admits 29 NL >= bits(M) + 2).  Every other key of the suite has R/M >= 16 (key sizes are
multiples of 4, and the limit widths of extreme_keys.json are limits of the digit geometries: n^2 is 78 or more bits below R
there).  Here, with B = 29 NL - 2 the widest n^2 a geometry of NL limbs admits:

    hi    the largest n = p q found below isqrt(2^B - 1): n^2 has B bits and R/M is just above 4 (nothing to spare)
    lo    the smallest n found above isqrt(2^(B-1)): n^2 still has B bits and R/M is just below 8 (the smallest modulus that
          still takes this geometry rather than the next one down ... where one exists)

`hi` and `lo` for the lane-group geometries NL = 36, 72, 112, 144, 224, 288 (n of 521 / 1043 / 1623 / 2087 / 3247 / 4175 bits);
`hi` alone for the latency geometries NL = 48, 96, 192 (n of 695 / 1391 / 2783 bits; NL = 288 is shared with the lane groups).
p != q have equal bit width.  Plain directed searches from fixed starting points with the oracle's Miller-Rabin test behind a
sieve of the primes below 2000; no random numbers.  With pb the width of one prime:

    hi    p = the largest prime <= isqrt(top) - 2^(pb-20), q = the largest prime <= top // p,     top = isqrt(2^B - 1)
    lo    p = the smallest prime >= isqrt(bot) + 2^(pb-20), q = the smallest prime > bot // p,    bot = isqrt(2^(B-1)) + 1

    python tests/golden/make_limit_keys.py
"""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from oracle import paillier_oracle as orc  # noqa: E402

LANE_GROUP_NL = (36, 72, 112, 144, 224, 288)
LATENCY_NL = (48, 96, 192)
SIEVE = [s for s in range(3, 2000, 2) if all(s % d for d in range(3, int(s ** 0.5) + 1, 2))]


def search(start, step):
    """First probable prime among the odd numbers start, start + step, ... (step = +-2; an even start moves one step first)"""
    c = start if start & 1 else start + step // 2
    while not (all(c % s for s in SIEVE) and orc.is_probable_prime(c)):
        c += step
    return c


def hi_pair(B):
    top = math.isqrt((1 << B) - 1)
    pb = (top.bit_length() + 1) // 2
    p = search(math.isqrt(top) - (1 << (pb - 20)), -2)
    return p, search(top // p, -2)


def lo_pair(B):
    bot = math.isqrt(1 << (B - 1)) + 1
    pb = (bot.bit_length() + 1) // 2
    p = search(math.isqrt(bot) + (1 << (pb - 20)), 2)
    return p, search(bot // p + 1, 2)


def main():
    out = []
    for nl in sorted(LANE_GROUP_NL + LATENCY_NL):
        B = 29 * nl - 2
        pairs = {"hi": hi_pair(B)}
        if nl in LANE_GROUP_NL:
            pairs["lo"] = lo_pair(B)
        for kind, (p, q) in pairs.items():
            n = p * q
            assert p != q and p.bit_length() == q.bit_length() and (n * n).bit_length() == B, (nl, kind)
            assert math.gcd(n, (p - 1) * (q - 1)) == 1, (nl, kind)
            out.append({"kind": kind, "nl": nl, "engine": "lane_group" if nl in LANE_GROUP_NL else "latency",
                        "n_bits": n.bit_length(), "prime_bits": p.bit_length(), "p": hex(p), "q": hex(q)})
        print(nl, "ok", file=sys.stderr)
    (Path(__file__).parent / "limit_keys.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
