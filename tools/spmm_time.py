#!/usr/bin/env python3
"""Times the encrypted gradient of vertical federated regression, X.T @ [[d]] with a sparse plaintext X (N samples x F
features, randn values at the given density) and N randn-exponent ciphertexts, at one key size.  Two legs, interleaved in one
process, `--reps` runs each, median reported:
  (a) the sparse product (X.T @ enc: pai_ct_sparse_multiexp), with its split into tables / terms / combine (engine.profile_last)
      and the host time of its plan (paillier._sparse_terms + _sparse_plan);
  (b) the composite route with operations that exist without it: gather the term rows (.words[index]), ct * weights,
      segment_sum.
`--legs b` runs leg (b) alone (no sparse-product code is imported).  One JSON line per leg.
usage: python tools/spmm_time.py [--bits 2048] [--n 1048576] [--f 1024] [--density 0.01] [--reps 3] [--legs a,b]"""
import argparse, json, statistics, sys, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import scipy.sparse as sparse
import torch
import bench
from pailliercryptolib_python_amd import PaillierPublicKey, engine, fixedpoint
from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=2048)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--f", type=int, default=1024)
ap.add_argument("--density", type=float, default=0.01)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--legs", default="a,b")
a = ap.parse_args()
legs = a.legs.split(",")
key = bench.synthetic_key(a.bits)
pk = PaillierPublicKey(ipclPublicKey(key.n, a.bits, True, hs=key.hs, randbits=key.randbits))
h = pk.pubkey.handle
dev = h.device
N, F = a.n, a.f
g = torch.Generator(device=dev)
g.manual_seed(1)
ct = torch.randint(-(1 << 31), 1 << 31, (N, h.ct_words), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
ct[:, -1] &= 0x3FFFFFFF              # below n^2 for the fixture keys
ct = ct.contiguous()
rng = np.random.default_rng(2)
expo = fixedpoint.float64_mantissas(rng.standard_normal(N))[1].astype(np.int32)
enc = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, ct), expo, N)
X = sparse.random(N, F, density=a.density, format="csr", random_state=3, data_rvs=lambda k: rng.standard_normal(k))
Xt = X.T.tocsr()                     # F x N: row f holds the samples of feature f, in sample order
T = Xt.nnz
base_t = torch.from_numpy(Xt.indices.astype(np.int64)).to(dev)
seg_t = torch.from_numpy(np.repeat(np.arange(F), np.diff(Xt.indptr))).to(dev)
w_b = np.ascontiguousarray(Xt.data, dtype=np.float64)
e_b = expo[Xt.indices]


def leg_a():
    return X.T @ enc


def leg_b():
    terms = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, enc.words[base_t].contiguous()), e_b, T)
    return (terms * w_b).segment_sum(seg_t, F)


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


fns = {"a": leg_a, "b": leg_b}
for leg in legs:                     # warm-up (first-call setup, allocator)
    fns[leg]()
times = {leg: [] for leg in legs}
for _ in range(a.reps):
    for leg in legs:
        times[leg].append(timed(fns[leg]))
base = {"bits": a.bits, "n": N, "f": F, "density": a.density, "terms": T, "reps": a.reps}
med = {leg: statistics.median(times[leg]) for leg in legs}
if "a" in legs:
    from pailliercryptolib_python_amd import paillier as P
    engine.profile_enable(True)
    leg_a()
    prof = engine.profile_last()
    engine.profile_enable(False)
    ptr, idx, d, (m, n, k) = P._csr_args(Xt.indptr, Xt.indices, Xt.data, Xt.shape, N, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mant, pexpo = P._sparse_weights(d)
    b_, w_, s_, off_ = P._sparse_terms(ptr.to(dev), idx.to(dev), m, n, k, True)
    e_, ebits, _, _ = P._sparse_plan(b_, w_, s_, torch.from_numpy(mant).to(dev), torch.from_numpy(pexpo).to(dev),
                                     torch.from_numpy(expo.astype(np.int64)).to(dev), m * k)
    torch.cuda.synchronize()
    t_plan = time.perf_counter() - t0
    print(json.dumps({**base, "leg": "a_sparse", "ms": 1e3 * med["a"], "runs_ms": [1e3 * t for t in times["a"]],
                      "terms_per_s": T / med["a"], "kernels_ms": prof, "plan_host_ms": 1e3 * t_plan, "ebits": ebits,
                      "e_words": int(e_.shape[1])}), flush=True)
if "b" in legs:
    row = {**base, "leg": "b_composite", "ms": 1e3 * med["b"], "runs_ms": [1e3 * t for t in times["b"]], "terms_per_s": T / med["b"]}
    if "a" in legs:
        row["speedup_a_over_b"] = med["b"] / med["a"]
    print(json.dumps(row), flush=True)
