"""Times randomness recovery against decryption on the same device-resident batch, and the public check of the openings:
sk.prikey.recover_r_words, sk.prikey.decrypt_words and PaillierPublicKey.verify_opening for batches 16 .. 2^16 at a 2048-bit key
and 2^14 at 3072- and 4096-bit keys.  The two private calls are timed ALTERNATING in one loop (one warm-up each, then `--reps`
pairs), host clock around a device synchronise; per-kernel milliseconds come from a separate profiled call (pai_profile_last).
Every batch is checked before it is timed: verify_opening of (decrypt, recover_r) must be all True.  One JSON line per batch.

    python tools/recover_time.py [--out profiles/r15/recover_time.jsonl] [--reps 5] [--quick]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batches / 16 (plumbing check)")
    args = ap.parse_args()
    import numpy as np
    import torch

    from oracle import paillier_oracle as orc
    from pailliercryptolib_python_amd import (PaillierEncryptedNumber, PaillierOpening, PaillierPrivateKey, PaillierPublicKey, _native,
                                              engine)
    from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey

    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def once(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    plan = [(2048, [16, 256, 4096, 16384, 65536]), (3072, [16384]), (4096, [16384])]
    for bits, batches in plan:
        p, q = _native.keygen(bits, True, seed=4000 + bits)
        key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=bits)
        pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
        sk = PaillierPrivateKey(pk, p, q)
        h = pk.pubkey.handle
        full = max(batches) // (16 if args.quick else 1)
        rng = np.random.default_rng(bits)
        m_all = torch.from_numpy(rng.integers(0, 2**31, (full, h.n_words), dtype=np.int64).astype(np.int32)).to(h.device)
        m_all[:, -1] = 0                                                       # residues below n
        ct_all = pk.pubkey.encrypt_words(m_all, True, h.random_r(full))
        torch.cuda.synchronize()
        for N in [max(1, b // (16 if args.quick else 1)) for b in batches]:
            ct = ct_all[:N].contiguous()
            zeros = np.zeros(N, dtype=np.int32)
            x = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, ct), exponents=zeros, length=N)
            first_ms = once(lambda: sk.prikey.recover_r_words(ct))             # (the very first call of a key builds the exponents)
            r = sk.prikey.recover_r_words(ct)
            m = sk.prikey.decrypt_words(ct)
            assert torch.equal(m, m_all[:N]), "decryption does not return the plaintexts"
            op = PaillierOpening(pk, m, r, zeros, N)
            assert bool(pk.verify_opening(x, op).all()), "an opening does not verify"
            rec_ms, dec_ms = [], []
            for _ in range(args.reps):
                rec_ms.append(once(lambda: sk.prikey.recover_r_words(ct)))
                dec_ms.append(once(lambda: sk.prikey.decrypt_words(ct)))
            ver_ms = [once(lambda: pk.verify_opening(x, op)) for _ in range(max(2, args.reps // 2))]
            engine.profile_enable(True)
            sk.prikey.recover_r_words(ct)
            kern = engine.profile_last()
            sk.prikey.decrypt_words(ct)
            kern_dec = engine.profile_last()
            engine.profile_enable(False)
            med_r, med_d = statistics.median(rec_ms), statistics.median(dec_ms)
            emit({"what": "recover_r", "bits": bits, "N": N, "recover_ms": med_r, "recover_spread_ms": max(rec_ms) - min(rec_ms),
                  "decrypt_ms": med_d, "decrypt_spread_ms": max(dec_ms) - min(dec_ms), "ratio": med_r / med_d,
                  "verify_ms": statistics.median(ver_ms), "first_call_ms": first_ms, "recover_kernels_ms": kern,
                  "decrypt_kernels_ms": kern_dec})
        del m_all, ct_all
        h.trim()


if __name__ == "__main__":
    main()
