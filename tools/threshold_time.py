"""Times threshold decryption on device-resident batches.

  partial   PaillierKeyShare's partial decryption (pai_partial_decrypt, share 1 of (3, 2)) against sk.decrypt on the same batch:
            16 .. 2^16 elements at a 2048-bit key, 2^12 at 3072- and 4096-bit keys; on digit-engine keys both routes (k_pow_padic
            forced with tpart_min = 0, the routes of pai_ct_mul with tpart_min out of reach) next to the default
  combine   pai_threshold_combine at t = 2, 3, 5 and 16 of 16 parties, 2^16 elements, 2048-bit key: k_tcomb_padic (tcomb_min = 0)
            against the composition route (PAI_DISABLE=tcombine), with the per-kernel milliseconds of a profiled call

Calls are timed ALTERNATING in one loop (one warm-up each, then `--reps` rounds), host clock around a device synchronise.  Every
batch is checked before it is timed: the combined residues must equal the plaintexts.  One JSON line per measurement.

    python tools/threshold_time.py [--out profiles/r21/threshold_time.jsonl] [--reps 3] [--quick]
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


def set_list(var: str, name: str, value) -> None:
    """name[=value] in the comma list `var` (PAI_TUNE / PAI_DISABLE); value None removes it, True adds the bare name"""
    cur = [kv for kv in os.environ.get(var, "").split(",") if kv and kv.split("=")[0] != name]
    if value is True:
        cur.append(name)
    elif value is not None:
        cur.append(f"{name}={value}")
    os.environ[var] = ",".join(cur)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="batches / 16 (plumbing check)")
    args = ap.parse_args()
    import numpy as np
    import torch

    from oracle import paillier_oracle as orc
    from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, _native, engine
    from pailliercryptolib_python_amd import threshold as th
    from pailliercryptolib_python_amd.bindings import ipclPublicKey

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
        """{name: median ms} of the calls `fns`, alternating"""
        for f in fns.values():
            once(f)
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                ms[k].append(once(f))
        return {k: statistics.median(v) for k, v in ms.items()}, {k: max(v) - min(v) for k, v in ms.items()}

    def profiled(fn):
        engine.profile_enable(True)
        fn()
        kern = engine.profile_last()
        engine.profile_enable(False)
        return kern

    scale = 16 if args.quick else 1
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
        m_all[:, -1] = 0                                                       # residues below n
        ct_all = pk.pubkey.encrypt_words(m_all, True, h.random_r(full))
        torch.cuda.synchronize()
        shares = sk.share(3, 2, seed=bits)
        hs = [s._native() for s in shares]
        for N in [max(1, b // scale) for b in batches]:
            ct = ct_all[:N].contiguous()
            parts = [hs[i].partial_decrypt(ct) for i in (0, 2)]
            mags, negs = th.lagrange([1, 3], 3)
            m, flag, _ = h.threshold_combine(parts, [2 * v for v in mags], negs, th.theta(pk.n, 3))
            assert int(flag.item()) == 0 and torch.equal(m, m_all[:N]), "the combined residues are not the plaintexts"
            fns = {"partial": lambda: hs[0].partial_decrypt(ct), "decrypt": lambda: sk.prikey.decrypt_words(ct)}
            med, spread = timed(fns)
            rec = {"what": "partial_decrypt", "bits": bits, "N": N, "exponent_bits": shares[0].exponent().bit_length(),
                   "partial_ms": med["partial"], "partial_spread_ms": spread["partial"], "decrypt_ms": med["decrypt"],
                   "decrypt_spread_ms": spread["decrypt"], "ratio": med["partial"] / med["decrypt"],
                   "partial_kernels_ms": profiled(fns["partial"])}
            if bits <= 2048:                                                   # both routes of a digit-engine key
                for name, v in (("pow_padic", 0), ("ct_mul", 1 << 40)):
                    set_list("PAI_TUNE", "tpart_min", v)
                    mm, _ = timed({"x": fns["partial"]})
                    rec[f"{name}_ms"] = mm["x"]
                set_list("PAI_TUNE", "tpart_min", None)
            emit(rec)
        if bits == 2048:
            N = 65536 // scale
            ct = ct_all[:N].contiguous()
            for t in (2, 3, 5, 16):
                dealt = sk.share(16, t, seed=100 + t)
                subset = list(range(1, t + 1))
                parts = [dealt[i - 1]._native().partial_decrypt(ct) for i in subset]
                mags, negs = th.lagrange(subset, 16)
                coeff, theta = [2 * v for v in mags], th.theta(pk.n, 16)
                call = lambda: h.threshold_combine(parts, coeff, negs, theta)     # noqa: E731
                rec = {"what": "combine", "bits": bits, "N": N, "t": t, "parties": 16, "coeff_bits": max(c.bit_length() for c in coeff)}
                for name, fused in (("fused", True), ("composition", False)):
                    set_list("PAI_DISABLE", "tcombine", None if fused else True)
                    set_list("PAI_TUNE", "tcomb_min", 0)
                    m, flag, _ = call()
                    assert int(flag.item()) == 0 and torch.equal(m, m_all[:N]), f"{name}: the combined residues are not the plaintexts"
                    med, spread = timed({"x": call})
                    rec[f"{name}_ms"], rec[f"{name}_spread_ms"], rec[f"{name}_kernels_ms"] = med["x"], spread["x"], profiled(call)
                set_list("PAI_DISABLE", "tcombine", None)
                set_list("PAI_TUNE", "tcomb_min", None)
                rec["fused_over_composition"] = rec["fused_ms"] / rec["composition_ms"]
                emit(rec)
                del parts
        del m_all, ct_all
        h.trim()


if __name__ == "__main__":
    main()
