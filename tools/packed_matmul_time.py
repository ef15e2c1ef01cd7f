#!/usr/bin/env python3
"""Times the encrypted gradient X.T @ [[D]] of a linear model with k outputs on packed rows against the route with k plain
containers, on one device: 2048-bit key, G samples, F features, k slots of b bits, 16-bit integer weights of both signs.
  (a) the parent's route: k plain containers d_j (one residual column each), X.T @ d_j for each                  (k products)
      (a1) through the public API, `X.T.astype(float64) @ d_j`: the parent's multi-exponentiation serves float matrices only and
           encodes every weight by its 53-bit float mantissa at the weight's own exponent, so its exponents are about 53 bits
           wide (plus alignment) where (b)'s are 16 — what a user of the parent pays, NOT a like-for-like term cost;
      (a2) at (b)'s exponent width: the same 16-bit operands (pai_fp_quantize) through pai_ct_invert_flag + pai_ct_multiexp on
           each plain container — k calls of exactly what (b) runs once; (a2) / (b) is the packing gain alone.
      Both end with k F plain ciphertexts, not with (b)'s F packed rows of k slots: the `pack` that would bring them there (an
      interleave of the k results and one Horner chain per row) is left out, which favours (a).
  (b) X.T @ P on the packed rows P (row i = the k residuals of sample i)                                          (one product)
  (c) pai_fp_quantize alone against the torch construction of the same operands (the word loop of
      PaillierEncryptedNumber._matmul_multiexp_build): |w| words [G][F][ew] and signs [G][F] of the F x G weights
Medians of --reps interleaved runs (one of (a1), (a2), (b) in turn) with the spread (max - min) beside them, the ratios to (b),
and the kernels of the last (b) product from pai_profile_last.  Every route must decrypt to the same sums.
Every GPU step is a child process of its own under `timeout -k 10`; the first step that fails or runs over ends the run.
One JSON line per figure, also appended to --out (default profiles/r12/packed_matmul_time.jsonl).
usage: python tools/packed_matmul_time.py [--bits 2048] [--n 262144] [--features 64] [--slots 8] [--slot-bits 100] [--reps 5]"""
import argparse, json, statistics, subprocess, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=2048)
ap.add_argument("--n", type=int, default=1 << 18)
ap.add_argument("--features", type=int, default=64)
ap.add_argument("--slots", type=int, default=8)
ap.add_argument("--slot-bits", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=420)
ap.add_argument("--out", default=str(ROOT / "profiles" / "r12" / "packed_matmul_time.jsonl"))
ap.add_argument("--step", choices=("quantize", "products"), default=None, help="(internal) the step this child process runs")
a = ap.parse_args()

if a.step is None:
    # the driver: one child per GPU step, each under its own limit; nothing more is started after a step that did not end well
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for step in ("quantize", "products"):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--bits", str(a.bits), "--n", str(a.n),
               "--features", str(a.features), "--slots", str(a.slots), "--slot-bits", str(a.slot_bits), "--reps", str(a.reps),
               "--out", a.out, "--step", step]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"packed_matmul_time: step {step} ended with status {rc}; stopping", file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np
import torch
import bench
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, engine, packed
from pailliercryptolib_python_amd.bindings import ipclPublicKey

key = bench.synthetic_key(a.bits)
pk = PaillierPublicKey(ipclPublicKey(key.n, a.bits, True, hs=key.hs, randbits=key.randbits))
sk = PaillierPrivateKey(pk, key.p, key.q)
h = pk.pubkey.handle
G, F, k, B = a.n, a.features, a.slots, a.slot_bits
V = 40                                               # residual mantissas |m| < 2^40: 2^18 samples x 16-bit weights stay below 2^75
rng = np.random.default_rng(1)
D = rng.integers(-(1 << V) + 1, 1 << V, (G, k))
X = rng.integers(-(1 << 15), 1 << 15, (G, F))        # 16-bit weights, both signs
sink = open(a.out, "a")


def emit(row):
    line = json.dumps({"bits": a.bits, "n": G, "features": F, "slots": k, "slot_bits": B, **row})
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def once(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def spread(ts):
    return max(ts) - min(ts)


if a.step == "quantize":
    w = torch.from_numpy(np.ascontiguousarray(X.T)).to(h.device)          # [F][G] as rmatmul holds it; the kernel reads w.t()

    def with_torch():
        mag = w.t().abs().contiguous()
        e = (mag & 0xFFFFFFFF).to(torch.int32).reshape(G, F, 1)           # one word: the loop of _matmul_multiexp_build at ew = 1
        sign = (w.t() < 0).to(torch.uint8).contiguous()
        return e, sign, mag.sum(dim=0)

    def with_kernel():
        return h.fp_quantize(w.t(), 0, 16, 1)

    et, st, sumt = with_torch()
    ek, sk_, sumk, flag = with_kernel()
    assert int(flag.item()) == 0 and torch.equal(et, ek) and torch.equal(st, sk_) and torch.equal(sumt, sumk[:, 0])
    tt, tk = [], []
    for rep in range(a.reps + 1):
        t1, _ = once(with_torch)
        t2, _ = once(with_kernel)
        if rep:
            tt.append(t1)
            tk.append(t2)
    mt, mk = statistics.median(tt), statistics.median(tk)
    emit({"what": "quantize", "weights": G * F, "torch_ms": mt, "torch_spread_ms": spread(tt), "kernel_ms": mk,
          "kernel_spread_ms": spread(tk), "torch_over_kernel": mt / mk, "kernel_GBps": G * F * 13 / mk / 1e6})
    sys.exit(0)

# ---- the products: (a1) / (a2) k plain containers, (b) the packed rows ----------------------------------------------------------------
from pailliercryptolib_python_amd.bindings import ipclCipherText

Xt_i = np.ascontiguousarray(X.T)
Xt_f = Xt_i.astype(np.float64)
cols = [pk.encrypt(np.ascontiguousarray(D[:, j])) for j in range(k)]
P = pk.encrypt_packed(D.reshape(-1), exponent=0, value_bits=V, slot_bits=B, slots=k)
want = Xt_i.astype(object) @ D.astype(object)
w_dev = torch.from_numpy(Xt_i).to(h.device)


def route_a1():
    return [Xt_f @ c for c in cols]


def route_a2():
    outs = []
    for c in cols:
        e, sign, _, _ = h.fp_quantize(w_dev.t(), 0, 16, 1)
        ct = c.words
        flag = h.new_flag()
        outs.append(h.ct_multiexp(ct, h.ct_invert(ct, flag=flag), 1, G, F, e.reshape(1, G, F, 1), 16, sign))
    return outs


def route_b():
    return Xt_i @ P


routes = {"a1": route_a1, "a2": route_a2, "b": route_b}
ts = {r: [] for r in routes}
res = {}
for rep in range(a.reps + 1):                            # round 0 warms up
    for r, f in routes.items():
        t, res[r] = once(f)
        if rep:
            ts[r].append(t)
assert packed.PACKED_ROUTES["composite"] == 0            # (b) took the multi-exponentiation every time
assert (np.array(sk.decrypt_packed_mantissas(res["b"]), dtype=object).reshape(F, k) == want).all()
for j in range(k):
    wj = np.array([float(x) for x in want[:, j]])
    assert np.allclose(sk.decrypt_to_numpy(res["a1"][j]), wj, rtol=1e-12, atol=0)       # the plain containers, decrypted as they are
    one = packed.PaillierPackedNumber(pk, ipclCipherText(pk.pubkey, res["a2"][j]), slot_bits=B, slots=1, exponent=0, value_bits=B - 1,
                                      length=F)
    assert sk.decrypt_packed_mantissas(one) == [int(x) for x in want[:, j]]
med = {r: statistics.median(ts[r]) for r in routes}
emit({"what": "product", **{f"{r}_ms": med[r] for r in routes}, **{f"{r}_spread_ms": spread(ts[r]) for r in routes},
      "a1_over_b": med["a1"] / med["b"], "a2_over_b": med["a2"] / med["b"], "a_terms": k * G * F, "b_terms": G * F,
      "a1_exponent_bits": "53-bit mantissas + alignment", "a2_exponent_bits": 16, "b_exponent_bits": 16})
engine.profile_enable(True)
route_b()
emit({"what": "b_kernels_last_call", **{name: ms for name, ms in engine.profile_last().items()}})
engine.profile_enable(False)
