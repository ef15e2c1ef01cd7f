#!/usr/bin/env python3
"""Times PaillierEncryptedNumber.cumsum (pai_ct_scan) on a 2048-bit key for the shapes (runs, L) = (3072, 32), (768, 256),
(8, 2^17), (1, 2^20), on integer inputs (all exponents equal) and np.random.randn floats (mixed exponents).  Next to it, in the same
run: the in-chain product rate (pai_ct_mont_mul over N: the roof) and the two routes that need no cumsum —
  ladder:  Hillis-Steele, log2(L) passes of aligned additions on shifted slices (gathered through .words, wrapped, `+`);
  sums:    x[a:i+1].sum() for every prefix, at L <= 256 only, on a few runs and scaled to all of them ("sums_scaled": true).
One JSON line per configuration.  implied_products counts the member products and domain conversions of the levels the dispatcher
takes (path_ranges.hpp: scan_chunk); squarings = sum(raise) + sum(step) of the plan, which a chunked level walks twice.
usage: python tools/cumsum_time.py [--bits 2048] [--reps 3] [--shapes 3072x32,768x256,8x131072,1x1048576] [--epb 64] [--no-ladder]"""
import argparse, json, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
import bench
from pailliercryptolib_python_amd import PaillierPublicKey, fixedpoint
from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber, _scan_plan

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=2048)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="3072x32,768x256,8x131072,1x1048576")
ap.add_argument("--epb", type=int, default=64, help="lane groups per workgroup of the key's geometry (2048-bit keys: 64)")
ap.add_argument("--no-ladder", action="store_true")
a = ap.parse_args()
key = bench.synthetic_key(a.bits)
pk = PaillierPublicKey(ipclPublicKey(key.n, a.bits, True, hs=key.hs, randbits=key.randbits))
h = pk.pubkey.handle
dev = h.device
ncu = torch.cuda.get_device_properties(dev).multi_processor_count
g = torch.Generator(device=dev)
g.manual_seed(1)


def wall(f, reps):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def wrap(words, expo):
    return PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, words), expo, words.shape[0])


def implied_products(N, L, tag):
    """member products and conversions over the dispatcher's levels"""
    want = ncu * a.epb * 2
    total, n, l, per = 0, N, L, 1 + (tag != 1)
    while True:
        c = l if n // l >= want else max(4, -(-n // want))
        if total:
            c = max(c, 2)
        if c >= l:
            return total + n * per - n // l
        cpr = -(-l // c)
        chains = n // l * cpr
        total += 2 * n * per - chains - n // l
        n, l, per = chains, cpr, 1


def ladder(x, L, hi_idx):
    """Hillis-Steele on runs of L: pass d adds element i - d to element i wherever i - d lies in the same run"""
    words, expo = x.words, np.asarray(x.exponent(), dtype=np.int32)
    d = 1
    for hi, hi_host in hi_idx:
        s = wrap(words[hi].contiguous(), expo[hi_host]) + wrap(words[hi - d].contiguous(), expo[hi_host - d])
        words = words.clone()
        words[hi] = s.words
        expo = expo.copy()
        expo[hi_host] = np.asarray(s.exponent(), dtype=np.int32)
        d *= 2
    return wrap(words, expo)


rng = np.random.default_rng(2)
for shape in a.shapes.split(","):
    runs, L = (int(v) for v in shape.split("x"))
    N = runs * L
    ct = torch.randint(-(1 << 31), 1 << 31, (N, h.ct_words), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    ct[:, -1] &= 0x3FFFFFFF              # below n^2 for the fixture keys
    ct = ct.contiguous()
    t_mul = wall(lambda: h.ct_mont_mul(ct, ct), a.reps)
    rate = N / t_mul
    pos = np.arange(N) % L
    hi_idx = []
    d = 1
    while d < L:
        hh = np.nonzero(pos >= d)[0]
        hi_idx.append((torch.from_numpy(hh).to(dev), hh))
        d *= 2
    for kind in ("int", "float"):
        expo = np.zeros(N, np.int32) if kind == "int" else fixedpoint.float64_mantissas(rng.standard_normal(N))[1].astype(np.int32)
        x = wrap(ct, expo)
        t = wall(lambda: x.cumsum(L), a.reps)
        raise_, step, _ = _scan_plan(expo, L, False)
        products = implied_products(N, L, 0)
        row = {"what": "cumsum", "exponents": kind, "bits": a.bits, "runs": runs, "L": L, "n": N, "ms": 1e3 * t,
               "implied_products": products, "squarings": 0 if raise_ is None else int(raise_.sum()) + int(step.sum()),
               "in_chain_products_per_s": rate, "roof_ms": 1e3 * products / rate, "time_vs_roof": t / (products / rate)}
        if not a.no_ladder:
            t_lad = wall(lambda: ladder(x, L, hi_idx), 1)
            row.update({"ladder_ms": 1e3 * t_lad, "ladder_passes": len(hi_idx), "speedup_vs_ladder": t_lad / t})
        if L <= 256:
            sub = min(runs, 2 if L > 32 else 8)

            def sums():
                return [x[r * L:r * L + i + 1].sum() for r in range(sub) for i in range(L)]

            t_sums = wall(sums, 1) * runs / sub
            row.update({"sums_ms": 1e3 * t_sums, "sums_scaled": True, "sums_runs_timed": sub, "speedup_vs_sums": t_sums / t})
        print(json.dumps(row), flush=True)
    del ct
