"""Generates tests/golden/extreme_keys.json: prime pairs whose limbs sit at the extremes the kernels' carry, borrow and
lazy-bound arguments depend on (every other key of the suite is random).  Plain directed searches from fixed starting points
with the oracle's Miller-Rabin test; no random numbers.  Families, for primes of b bits (NL = digit-pair limbs serving b,
H = 29 NL / 2, the split of the Karatsuba halves):

    ones        q = largest prime below 2^b, p = the next one below: every limb above the lowest is all ones
    zeros       p = smallest prime >= 3 * 2^(b-2), q = the next one: every limb between the top two bits and the lowest is zero
    ones_zeros  p of `zeros`, q of `ones`: the CRT halves at opposite extremes, q - p ~ 2^(b-2)
    half        p = largest prime <= 3 * 2^(b-2) + 2^H - 1: low Karatsuba half all ones, high half zero below the top bits;
                q of `ones`
    n0          p = smallest prime 3 * 2^(b-2) + 1 + j 2^58, q = largest prime 2^b - 1 - j 2^58: p = 1, q = -1 and n = -1
                modulo 2^58, so the 29-bit Montgomery constants n0inv are 2^29 - 1 (p), 1 (q), 1 (n) and 2^29 - 1 (n^2 = 1)
    n0_one      p of `n0`, q = largest prime 2^b + 1 - j 2^58 (j >= 1): both = 1 modulo 2^58, n0inv = 2^29 - 1 for n and n^2

All six at b = 512, 1024, 1536, 2048; `ones` alone at the widest prime each digit geometry admits (29 NL - 20 bits: 676, 1604,
2068 — csrc/padic_dec_kernels.hip: padic_nl_for_prime_bits, csrc/pair_kernels.hip: pair_nl_for_prime_bits / pair_nl_for_n_bits).

    python tests/golden/make_extreme_keys.py
"""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from oracle import paillier_oracle as orc  # noqa: E402

NL = {512: 24, 676: 24, 1024: 36, 1536: 56, 1604: 56, 2048: 72, 2068: 72}
WIDTHS = (512, 1024, 1536, 2048)
LIMIT_WIDTHS = (676, 1604, 2068)


def search(start, step):
    """First probable prime among start, start + step, start + 2 step, ..."""
    c = start
    while not orc.is_probable_prime(c):
        c += step
    return c


def families(b):
    top = 3 << (b - 2)
    ones_q = search((1 << b) - 1, -2)
    ones_p = search(ones_q - 2, -2)
    zeros_p = search(top + 1, 2)
    zeros_q = search(zeros_p + 2, 2)
    h = 29 * NL[b] // 2
    half_p = search(top + (1 << h) - 1, -2)
    n0_p = search(top + 1, 1 << 58)
    n0_q = search((1 << b) - 1, -(1 << 58))
    one_q = search((1 << b) + 1 - (1 << 58), -(1 << 58))
    return {"ones": (ones_p, ones_q), "zeros": (zeros_p, zeros_q), "ones_zeros": (zeros_p, ones_q), "half": (half_p, ones_q),
            "n0": (n0_p, n0_q), "n0_one": (n0_p, one_q)}


def main():
    out = []
    for b in sorted(WIDTHS + LIMIT_WIDTHS):
        fams = families(b) if b in WIDTHS else None
        if fams is None:
            q = search((1 << b) - 1, -2)
            fams = {"ones": (search(q - 2, -2), q)}
        for name, (p, q) in fams.items():
            n = p * q
            assert p != q and n.bit_length() == 2 * b and math.gcd(n, (p - 1) * (q - 1)) == 1, (b, name)
            out.append({"family": name, "prime_bits": b, "p": hex(p), "q": hex(q)})
        print(b, "ok", file=sys.stderr)
    (Path(__file__).parent / "extreme_keys.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
