"""Times the batch verification of openings against the per-element one on the same device-resident batch:
PaillierPublicKey.verify_openings and PaillierPublicKey.verify_opening for batches 16 .. 2^20 at a 2048-bit key — the fused fold
(k_open_fold) and, side by side, the composition fold (PAI_DISABLE=open_fold) — and 2^14 at 3072- and 4096-bit keys (composition
only).  One warm-up of each, then `--reps` ALTERNATING pairs, host clock around a device synchronise; per-kernel milliseconds come
from a separate profiled call (pai_profile_last).  Every batch is verified before it is timed: both calls must be all True.
One JSON line per batch and route.

--wbits runs the window-width sweep of k_open_fold instead (the measurement behind the default of PAI_TUNE open_wbits): the fold alone
(engine.PublicKeyHandle.opening_fold, 128-bit coefficients, the default segmentation) at 2^16 and 2^20 rows of the 2048-bit key
with open_wbits = 2, 1, 3, 4, 2 in that order, both sides compared on every call, per-kernel milliseconds from the profile.

    python tools/verify_time.py [--out profiles/r16/verify_time.jsonl] [--reps 5] [--quick] [--max-log2 20]
    python tools/verify_time.py --wbits [--out profiles/r16/open_fold_wbits.jsonl] [--quick] [--max-log2 20]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="batches / 16 (plumbing check)")
    ap.add_argument("--max-log2", type=int, default=20, help="largest batch at 2048 bits")
    ap.add_argument("--bits", type=int, nargs="*", default=[2048, 3072, 4096])
    ap.add_argument("--wbits", action="store_true", help="sweep PAI_TUNE open_wbits over k_open_fold instead of timing the API")
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

    def set_disabled(name, on):
        cur = [k for k in os.environ.get("PAI_DISABLE", "").split(",") if k and k != name]
        os.environ["PAI_DISABLE"] = ",".join(cur + ([name] if on else []))

    def set_tune(name, value):
        cur = [kv for kv in os.environ.get("PAI_TUNE", "").split(",") if kv and kv.split("=")[0] != name]
        os.environ["PAI_TUNE"] = ",".join(cur + ([f"{name}={value}"] if value is not None else []))

    plan = {2048: [b for b in (16, 256, 4096, 1 << 16, 1 << 20) if b <= 1 << args.max_log2], 3072: [1 << 14], 4096: [1 << 14]}
    if args.wbits:
        bits = 2048
        p, q = _native.keygen(bits, True, seed=4000 + bits)
        key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=bits)
        pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
        sk = PaillierPrivateKey(pk, p, q)
        h = pk.pubkey.handle
        rng = np.random.default_rng(1)
        edges = h.path_edges(2)
        most = max(1, min(edges)) if edges else 1
        for N in [max(1, b // (16 if args.quick else 1)) for b in (1 << 16, 1 << 20) if b <= 1 << args.max_log2]:
            m = torch.from_numpy(rng.integers(0, 2**31, (N, h.n_words), dtype=np.int64).astype(np.int32)).to(h.device)
            m[:, -1] = 0
            ct = pk.pubkey.encrypt_words(m, True, h.random_r(N))
            r = sk.prikey.recover_r_words(ct)
            e = torch.from_numpy(rng.integers(-2**31, 2**31, (N, 4), dtype=np.int64).astype(np.int32)).to(h.device)
            seg = -(-N // min(N, most))
            for w in (2, 1, 3, 4, 2):
                set_tune("open_wbits", w)
                lhs, rhs, flag = h.opening_fold(ct, m, r, e, 128, seg)              # (warm-up: the table scratch grows here)
                assert torch.equal(lhs, rhs) and int(flag.item()) == 0, "the fold refuses valid openings"
                engine.profile_enable(True)
                h.opening_fold(ct, m, r, e, 128, seg)
                kern = engine.profile_last()
                engine.profile_enable(False)
                emit({"what": "open_fold_wbits", "bits": bits, "N": N, "segment": seg, "open_wbits": w, "kernels_ms": kern})
            set_tune("open_wbits", None)
            del m, ct, r, e
            h.trim()
        return
    for bits in args.bits:
        batches = plan[bits]
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
        r_all = sk.prikey.recover_r_words(ct_all)
        torch.cuda.synchronize()
        routes = [("fused", False), ("composition", True)] if h.n_words * 32 <= 2048 else [("composition", False)]
        for N in [max(1, b // (16 if args.quick else 1)) for b in batches]:
            ct = ct_all[:N].contiguous()
            zeros = np.zeros(N, dtype=np.int32)
            x = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, ct), exponents=zeros, length=N)
            op = PaillierOpening(pk, m_all[:N].contiguous(), r_all[:N].contiguous(), zeros, N)
            for route, disabled in routes:
                set_disabled("open_fold", disabled)
                assert bool(pk.verify_opening(x, op).all()), "an opening does not verify"           # (warm-up of the single check)
                assert bool(pk.verify_openings(x, op).all()), "the batch check refuses valid openings"
                torch.cuda.synchronize()
                batch_ms, single_ms = [], []
                for _ in range(args.reps):
                    batch_ms.append(once(lambda: pk.verify_openings(x, op)))
                    single_ms.append(once(lambda: pk.verify_opening(x, op)))
                engine.profile_enable(True)
                pk.verify_openings(x, op)
                kern = engine.profile_last()
                pk.verify_opening(x, op)
                kern_single = engine.profile_last()
                engine.profile_enable(False)
                edges = h.path_edges(2)
                most = max(1, min(edges)) if edges else 1
                med_b, med_s = statistics.median(batch_ms), statistics.median(single_ms)
                emit({"what": "verify_openings", "bits": bits, "N": N, "route": route, "segment": -(-N // min(N, most)),
                      "batch_ms": med_b, "batch_spread_ms": max(batch_ms) - min(batch_ms), "single_ms": med_s,
                      "single_spread_ms": max(single_ms) - min(single_ms), "speedup": med_s / med_b,
                      "batch_kernels_ms": kern, "batch_kernels_sum_ms": sum(kern.values()), "single_kernels_ms": kern_single})
            set_disabled("open_fold", False)
        del m_all, ct_all, r_all
        h.trim()


if __name__ == "__main__":
    main()
