"""Times verifiable threshold decryption on device-resident batches.

  proof    PaillierKeyShare.partial_decrypt(x, prove=True)'s proof step and PaillierPublicKey.verify_partial against the
           partial decryption of the same batch (pai_partial_decrypt, share 1 of (3, 2)): 16 .. 2^16 rows at a 2048-bit key, 2^12 at
           3072- and 4096-bit keys, with the per-kernel milliseconds of one profiled prove and one profiled verify
  sha      k_sha256_rows over two limb matrices of a 2048-bit key's ciphertext width (1 KiB per row) against (a) a
           device-to-device copy of the same bytes and (b) a device-to-host copy plus hashlib.sha256 of them: 2^12 .. 2^20 rows
           (hashlib up to 2^18).  The host-only hashing is timed on its own, outside the alternating loop: the kernel that
           follows 0.1 s without device work is measured 0.1 ms slow.

Calls are timed ALTERNATING in one loop (one warm-up each, then `--reps` rounds), host clock around a device synchronise; the
spread is max - min over the rounds.  Every proof is verified before anything is timed.  One JSON line per measurement.

    python tools/threshold_proof_time.py [--out profiles/r23/threshold_proof_time.jsonl] [--reps 3] [--quick]
"""
from __future__ import annotations

import argparse
import hashlib
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="batches / 16 (plumbing check)")
    ap.add_argument("--only", choices=("proof", "sha"), default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from oracle import paillier_oracle as orc
    from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, _native, engine
    from pailliercryptolib_python_amd import threshold as th
    from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
    from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber

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

    def timed(fns):
        """({name: median ms}, {name: max - min}) of the calls `fns`, alternating"""
        for f in fns.values():
            once(f)
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                ms[k].append(once(f))
        return {k: statistics.median(v) for k, v in ms.items()}, {k: max(v) - min(v) for k, v in ms.items()}

    def kernels_of(fn):
        """{kernel: ms} summed over every engine call `fn` makes (the profile keeps the last call only: collected per call)"""
        total = {}
        real = _native.check

        def collecting(code):
            real(code)
            for k, v in engine.profile_last().items():                        # (every compute entry point starts its list afresh)
                total[k] = total.get(k, 0.0) + v

        engine.profile_enable(True)
        _native.check = collecting
        try:
            fn()
        finally:
            _native.check = real
            engine.profile_enable(False)
        return total

    scale = 16 if args.quick else 1
    if args.only != "sha":
        plan = [(2048, [16, 256, 4096, 16384, 65536]), (3072, [4096]), (4096, [4096])]
        for bits, batches in plan:
            p, q = _native.keygen(bits, True, seed=4000 + bits)
            key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=bits)
            pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
            sk = PaillierPrivateKey(pk, p, q)
            h = pk.pubkey.handle
            full = max(batches) // scale
            rng = np.random.default_rng(bits)
            m_all = torch.from_numpy(rng.integers(0, 2**31, (full, h.n_words), dtype=np.int64).astype(np.int32)).to(h.device)
            m_all[:, -1] = 0                                                   # residues below n
            ct_all = pk.pubkey.encrypt_words(m_all, True, h.random_r(full))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            shares = sk.share(3, 2, seed=bits, verifiable=True)
            deal_ms = (time.perf_counter() - t0) * 1e3
            vk = shares[0].verification_key
            sh = shares[0]
            hs = sh._native()
            for N in [max(1, b // scale) for b in batches]:
                ct = ct_all[:N].contiguous()
                x = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, ct), exponents=[0] * N, length=N)
                part = sh.partial_decrypt(x, prove=True)
                assert pk.verify_partial(x, part, vk), "an honest proof was rejected"
                pw = part.words(h.device)
                share_int = sh.exponent() // (2 * th.delta(3))
                fns = {"partial": lambda: hs.partial_decrypt(ct),
                       "prove": lambda: th._prove_device(h, vk, 1, share_int, ct, pw, None),
                       "verify": lambda: pk.verify_partial(x, part, vk)}
                med, spread = timed(fns)
                emit({"what": "proof", "bits": bits, "N": N, "deal_verifiable_ms": deal_ms, "partial_ms": med["partial"],
                      "partial_spread_ms": spread["partial"], "prove_ms": med["prove"], "prove_spread_ms": spread["prove"],
                      "verify_ms": med["verify"], "verify_spread_ms": spread["verify"], "prove_over_partial": med["prove"] / med["partial"],
                      "verify_over_partial": med["verify"] / med["partial"], "prove_kernels_ms": kernels_of(fns["prove"]),
                      "verify_kernels_ms": kernels_of(fns["verify"])})
            del m_all, ct_all
            h.trim()
    if args.only != "proof":
        bits = 2048
        p, q = _native.keygen(bits, True, seed=4000 + bits)
        key = orc.make_key(p, q, djn_x=0xABCDEF1234567, bits=bits)
        h = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits)).pubkey.handle
        W = h.ct_words
        for N in [max(1, b // scale) for b in (1 << 12, 1 << 16, 1 << 18, 1 << 20)]:
            a = torch.randint(-(2**31), 2**31, (N, W), dtype=torch.int64, device=h.device).to(torch.int32)
            b = torch.randint(-(2**31), 2**31, (N, W), dtype=torch.int64, device=h.device).to(torch.int32)
            a2, b2 = torch.empty_like(a), torch.empty_like(b)
            dig = torch.empty((N, 8), dtype=torch.int32, device=h.device)
            host = [torch.empty((N, W), dtype=torch.int32).pin_memory() for _ in range(2)]

            def sha():
                h.sha256_rows([a, b], out=dig)

            def d2d():
                a2.copy_(a)
                b2.copy_(b)

            def d2h():
                host[0].copy_(a)
                host[1].copy_(b)

            def hashed():
                ha, hb = host[0].numpy(), host[1].numpy()
                return b"".join(hashlib.sha256(ha[j].tobytes() + hb[j].tobytes()).digest() for j in range(N))

            sha()
            d2h()
            torch.cuda.synchronize()
            rec = {"what": "sha256_rows", "row_bytes": 8 * W, "N": N, "bytes": 8 * W * N}
            if N <= 1 << 18:
                t0 = time.perf_counter()
                want = hashed()
                rec["hashlib_ms"] = (time.perf_counter() - t0) * 1e3
                assert engine.to_host_words(dig).tobytes() == want, "wrong digests"
            med, spread = timed({"sha": sha, "d2d": d2d, "d2h": d2h})
            for k in med:
                rec[f"{k}_ms"], rec[f"{k}_spread_ms"] = med[k], spread[k]
            rec["sha_kernel_ms"] = statistics.median(kernels_of(sha)["k_sha256_rows"] for _ in range(max(3, args.reps)))
            rec["sha_GBps"] = 8 * W * N / rec["sha_kernel_ms"] / 1e6
            rec["d2d_GBps"] = 8 * W * N / med["d2d"] / 1e6
            emit(rec)
            del a, b, a2, b2, host


if __name__ == "__main__":
    main()
