#!/usr/bin/env python3
"""Times the GH-packed histogram pipeline against the route with two plain containers, on one device, 2048-bit key, N samples
with a gradient g and a hessian h each, F features of K bins:
  (a) encrypt(g), encrypt(h) -> segment_sum and cumsum on each -> pack on each -> decrypt_packed        (two rows per sample)
  (b) encrypt_packed of the interleaved (g, h), slots=2 -> segment_sum -> cumsum -> repack -> decrypt_packed   (one row)
Per-stage medians of --reps interleaved runs (a stage of (a), then the same stage of (b)), the spread (max - min) beside them,
the (a) / (b) ratio per stage, and the in-chain product rate of the same run (pai_ct_mont_mul over N rows) beside the member
rate of the histogram stage.  Both routes must decrypt to the same cumulative histograms.
Every GPU step is a child process of its own under a time limit (--step-timeout); the first step that fails or runs over ends
the run.  One JSON line per figure, also appended to --out (default profiles/r11/gh_pack_time.jsonl).
usage: python tools/gh_pack_time.py [--bits 2048] [--n 1048576] [--features 8] [--bins 32] [--reps 5] [--out FILE]"""
import argparse, json, statistics, subprocess, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=2048)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--features", type=int, default=8)
ap.add_argument("--bins", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=420)
ap.add_argument("--out", default=str(ROOT / "profiles" / "r11" / "gh_pack_time.jsonl"))
ap.add_argument("--step", choices=("stages", "in_chain"), default=None, help="(internal) the step this child process runs")
a = ap.parse_args()

if a.step is None:
    # the driver: one child per GPU step, each under its own limit; nothing more is started after a step that did not end well
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    for step in ("stages", "in_chain"):
        cmd = [sys.executable, __file__, "--bits", str(a.bits), "--n", str(a.n), "--features", str(a.features), "--bins", str(a.bins),
               "--reps", str(a.reps), "--out", a.out, "--step", step]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"gh_pack_time: step {step} ended with status {rc}; stopping", file=sys.stderr)
            sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np
import torch
import bench
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey
from pailliercryptolib_python_amd.bindings import ipclPublicKey

key = bench.synthetic_key(a.bits)
pk = PaillierPublicKey(ipclPublicKey(key.n, a.bits, True, hs=key.hs, randbits=key.randbits))
sk = PaillierPrivateKey(pk, key.p, key.q)
h = pk.pubkey.handle
N, F, K = a.n, a.features, a.bins
E, B = 40, 100                                       # mantissas rint(x 2^40), |m| <= 2^40; 100-bit slots hold 2^20-member sums
rng = np.random.default_rng(1)
# values on the 2^-40 grid: both routes then carry exactly the same sums
g = np.ldexp(np.rint(np.ldexp(rng.uniform(-1, 1, N), E)), -E)
hs = np.ldexp(np.rint(np.ldexp(rng.uniform(0, 1, N), E)), -E)
gh = np.stack([g, hs], axis=1).reshape(-1)
ids = torch.from_numpy(rng.integers(0, K, (N, F))).to(h.device)
sink = open(a.out, "a")


def emit(row):
    line = json.dumps({"bits": a.bits, "n": N, "features": F, "bins": K, **row})
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def once(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


if a.step == "in_chain":
    ct = pk.encrypt_packed(gh, exponent=E, value_bits=E + 1, slot_bits=B, slots=2).ciphertext().words
    once(lambda: h.ct_mont_mul(ct, ct))
    ts = [once(lambda: h.ct_mont_mul(ct, ct))[0] for _ in range(a.reps)]
    med = statistics.median(ts)
    emit({"what": "in_chain_product", "rows": N, "ms": med, "spread_ms": max(ts) - min(ts), "products_per_ms": N / med})
    sys.exit(0)

# ---- the stages, (a) and (b) side by side: every stage consumes what the stage before it produced in the same round ---------------
STAGES = ("encrypt", "segment_sum", "cumsum", "pack", "decrypt")
# route (a) packs 128-bit slots: a float's own exponent reaches 53 + 40, and 2^20 aligned mantissas sum to 113 bits
route_a = {
    "encrypt": lambda _: (pk.encrypt(g), pk.encrypt(hs)),
    "segment_sum": lambda s: tuple(x.segment_sum(ids, K) for x in s),
    "cumsum": lambda s: tuple(x.cumsum(K) for x in s),
    "pack": lambda s: tuple(x.pack(slot_bits=128, value_bits=127) for x in s),
    "decrypt": lambda s: tuple(sk.decrypt_packed(x) for x in s),
}
route_b = {
    "encrypt": lambda _: pk.encrypt_packed(gh, exponent=E, value_bits=E + 1, slot_bits=B, slots=2),
    "segment_sum": lambda s: s.segment_sum(ids, K),
    "cumsum": lambda s: s.cumsum(K),
    "pack": lambda s: s.repack(),
    "decrypt": lambda s: sk.decrypt_packed(s),
}
ts = {(r, st): [] for r in "ab" for st in STAGES}
for rep in range(a.reps + 1):                            # round 0 warms up
    sa = sb = None
    for st in STAGES:
        ta, sa = once(lambda: route_a[st](sa))
        tb, sb = once(lambda: route_b[st](sb))
        if rep:
            ts[("a", st)].append(ta)
            ts[("b", st)].append(tb)
    got_b = sb.reshape(F * K, 2)
    assert np.allclose(sa[0], got_b[:, 0], rtol=1e-12, atol=0) and np.allclose(sa[1], got_b[:, 1], rtol=1e-12, atol=0)
idn = ids.cpu().numpy()
want = np.stack([[np.bincount(idn[:, f], weights=w, minlength=K) for f in range(F)] for w in (g, hs)], axis=-1).cumsum(axis=1)
assert np.allclose(got_b.reshape(F, K, 2), want, rtol=1e-9, atol=1e-6)      # (float64 sums of 2^20 terms on the reference side)
tot = {"a": 0.0, "b": 0.0}
for st in STAGES:
    ma, mb = statistics.median(ts[("a", st)]), statistics.median(ts[("b", st)])
    tot["a"] += ma
    tot["b"] += mb
    row = {"what": "stage", "stage": st, "a_ms": ma, "b_ms": mb, "a_over_b": ma / mb,
           "a_spread_ms": max(ts[("a", st)]) - min(ts[("a", st)]), "b_spread_ms": max(ts[("b", st)]) - min(ts[("b", st)])}
    if st == "segment_sum":                              # one product per member: N F members per container, two containers in (a)
        row.update({"a_members": 2 * N * F, "b_members": N * F, "a_members_per_ms": 2 * N * F / ma, "b_members_per_ms": N * F / mb})
    emit(row)
emit({"what": "total", "a_ms": tot["a"], "b_ms": tot["b"], "a_over_b": tot["a"] / tot["b"]})
