"""Generates tests/golden/safe_prime_keys.json: keys of two SAFE primes (p = 2 p' + 1, q = 2 q' + 1 with p', q' prime), the
setting in which a proof of correct partial decryption (pailliercryptolib_python_amd/threshold.py) has its
full soundness 2^-127.  The package's own key generator does not make such primes.

    toy     two 64-bit safe primes (n of 128 bits): the integer model's tests
    k1024   two 512-bit safe primes (n of 1024 bits): the integer model and the device path

Candidates come from the ChaCha20 stream of threshold.SeededRng under a fixed seed per prime: p' odd with its two top bits set,
both p' and 2 p' + 1 free of the primes below 2000, then threshold.is_probable_prime on both.

    python tests/golden/make_safe_prime_keys.py
"""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
from pailliercryptolib_python_amd import threshold as th  # noqa: E402

SIEVE = [s for s in range(3, 2000, 2) if all(s % d for d in range(3, int(s ** 0.5) + 1, 2))]


def safe_prime(bits: int, seed: int) -> int:
    rng = th.SeededRng(seed)
    while True:
        h = rng(1 << (bits - 1)) | (3 << (bits - 3)) | 1          # p' of bits - 1 bits, so p = 2 p' + 1 has `bits` with the top two set
        p = 2 * h + 1
        if all(h % s and p % s for s in SIEVE) and th.is_probable_prime(h) and th.is_probable_prime(p):
            return p


def main():
    out = []
    for name, bits, seed in (("toy", 64, 0x5AFE0064), ("k1024", 512, 0x5AFE0512)):
        p, q = safe_prime(bits, seed), safe_prime(bits, seed + 1)
        n = p * q
        assert p != q and n.bit_length() == 2 * bits and math.gcd(n, (p - 1) * (q - 1)) == 1
        assert th.safe_primes(p, q) and th.small_order_factor(p, q) == 0
        out.append({"name": name, "key_bits": 2 * bits, "p": hex(p), "q": hex(q)})
        print(name, "ok", file=sys.stderr)
    (Path(__file__).parent / "safe_prime_keys.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
