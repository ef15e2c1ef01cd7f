"""Times the owner-side CRT encryption against the public route on device-resident operands: pk.encrypt_words against
sk.encrypt_words (PAI_TUNE crtenc_min=0 forces the route), per-kernel milliseconds of the two half exponentiations, the lift and
the product modulo n^2 from pai_profile_last, the build time and bytes of the base-p / base-q tables, and a sweep of N for the
hand-over edge.  One warm-up, five repeats, median and spread (max - min).  One JSON line per measurement.

    python tools/crt_encrypt_time.py [--out profiles/r07/crt_encrypt_time.jsonl] [--bits 1536,2048,3072,4096] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bits", default="1536,2048,3072,4096")
    ap.add_argument("--quick", action="store_true", help="N / 16 (plumbing check)")
    args = ap.parse_args()
    tune = [kv for kv in os.environ.get("PAI_TUNE", "").split(",") if kv and not kv.startswith("crtenc_min=")]
    os.environ["PAI_TUNE"] = ",".join(tune + ["crtenc_min=0"])
    import numpy as np
    import torch

    from oracle import paillier_oracle as orc
    from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, _native, engine
    from pailliercryptolib_python_amd.bindings import ipclPublicKey

    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), max(ts) - min(ts)

    for bits in [int(b) for b in args.bits.split(",")]:
        p, q = _native.keygen(bits, True, seed=4000 + bits)
        key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=bits)
        pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
        sk = PaillierPrivateKey(pk, p, q)
        pub, h, sh = pk.pubkey, pk.pubkey.handle, sk.prikey.handle
        full = (1 << 20) if bits <= 2048 else 65536
        if args.quick:
            full //= 16
        rng = np.random.default_rng(bits)
        m_all = torch.from_numpy(rng.integers(0, 2**31, (full, h.n_words), dtype=np.int64).astype(np.int32)).to(h.device)
        m_all[:, -1] = 0                                                       # residues below n
        r_all = h.random_r(full)
        for route, first in (("crt", lambda: sk.prikey.encrypt_words(m_all[:64], r_all[:64])),
                             ("public", lambda: pub.encrypt_words(m_all[:64], True, r_all[:64]))):
            t0 = time.perf_counter()
            first()
            torch.cuda.synchronize()
            info = sh.crt_table_info() if route == "crt" else h.table_info()
            emit({"what": "table_build", "bits": bits, "route": route, "first_call_ms": (time.perf_counter() - t0) * 1e3, **info})
        a = sk.prikey.encrypt_words(m_all[:4096], r_all[:4096])
        assert torch.equal(a, pub.encrypt_words(m_all[:4096], True, r_all[:4096])), "routes disagree"
        sweep = sorted({full >> k for k in range(0, 13, 2)} | {full})
        for N in sweep:
            m, r = m_all[:N].contiguous(), r_all[:N].contiguous()
            med_p, spr_p = timed(lambda: pub.encrypt_words(m, True, r))
            med_c, spr_c = timed(lambda: sk.prikey.encrypt_words(m, r))
            engine.profile_enable(True)
            sk.prikey.encrypt_words(m, r)
            kern = engine.profile_last()
            pub.encrypt_words(m, True, r)
            kern_pub = engine.profile_last()
            engine.profile_enable(False)
            emit({"what": "encrypt_words", "bits": bits, "N": N, "public_ms": med_p, "public_spread_ms": spr_p, "crt_ms": med_c,
                  "crt_spread_ms": spr_c, "ratio": med_c / med_p, "crt_wins": med_p - med_c > max(spr_p, spr_c),
                  "crt_kernels_ms": kern, "public_kernels_ms": kern_pub})
        del m_all, r_all
        h.trim()


if __name__ == "__main__":
    main()
