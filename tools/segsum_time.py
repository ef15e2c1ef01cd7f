#!/usr/bin/env python3
"""Times PaillierEncryptedNumber.segment_sum (pai_ct_segment_prod) on the SecureBoost histogram shape: a 2048-bit key, N rows,
F features of K bins, integer gradients (all exponents equal) and np.random.randn floats (mixed exponents).  Next to it, in the
same run: the in-chain product rate (pai_ct_mont_mul over N) and, at F = 1, the route without a segment sum (per bin: gather
rows through .words[index], wrap, .sum()).  One JSON line per configuration.
usage: python tools/segsum_time.py [--bits 2048] [--n 1048576] [--k 32] [--reps 3] [--features 1,8]"""
import argparse, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import bench
from pailliercryptolib_python_amd import PaillierPublicKey, fixedpoint
from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber, _segment_plan

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=2048)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--features", default="1,8")
a = ap.parse_args()
key = bench.synthetic_key(a.bits)
pk = PaillierPublicKey(ipclPublicKey(key.n, a.bits, True, hs=key.hs, randbits=key.randbits))
h = pk.pubkey.handle
dev = h.device
N, K = a.n, a.k
g = torch.Generator(device=dev)
g.manual_seed(1)
ct = torch.randint(-(1 << 31), 1 << 31, (N, h.ct_words), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
ct[:, -1] &= 0x3FFFFFFF              # below n^2 for the fixture keys
ct = ct.contiguous()


def wall(f, reps):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


t_mul = wall(lambda: h.ct_mont_mul(ct, ct), a.reps)
rate = N / t_mul
print(json.dumps({"what": "in_chain_product", "bits": a.bits, "n": N, "ms": 1e3 * t_mul, "products_per_s": rate}), flush=True)
rng = np.random.default_rng(2)
for kind in ("int", "float"):
    expo = np.zeros(N, np.int32) if kind == "int" else fixedpoint.float64_mantissas(rng.standard_normal(N))[1].astype(np.int32)
    x = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, ct), expo, N)
    for F in [int(v) for v in a.features.split(",")]:
        ids = torch.randint(0, K, (N, F), device=dev, generator=g)
        t = wall(lambda: x.segment_sum(ids, K), a.reps)
        _, shift, offsets, _ = _segment_plan(ids, expo, K)
        M = int(offsets[-1])
        sh = shift[:M].to(torch.int64)
        lens = (offsets[1:] - offsets[:-1])
        products = (M - int((lens > 0).sum()) + int(sh.sum()) + int((sh > 0).sum()) + int((lens > 1).sum()))
        row = {"what": "segment_sum", "exponents": kind, "bits": a.bits, "n": N, "F": F, "K": K, "ms": 1e3 * t,
               "members_per_s": M / t, "implied_products": products, "ms_per_Mproduct": 1e3 * t / products * 1e6,
               "rate_vs_in_chain": (products / t) / rate}
        if F == 1:
            idx = [torch.nonzero(ids[:, 0] == b).reshape(-1) for b in range(K)]

            def today():
                outs = []
                for b in range(K):
                    sub = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, x.words[idx[b]].contiguous()), expo[idx[b].cpu().numpy()],
                                                  int(idx[b].numel()))
                    outs.append(sub.sum())
                return outs

            t_today = wall(today, 1)
            row.update({"gather_sum_ms": 1e3 * t_today, "speedup_vs_gather_sum": t_today / t})
        print(json.dumps(row), flush=True)
