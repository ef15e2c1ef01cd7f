#!/usr/bin/env python3
"""Times packed ciphertexts against the route without them, on one device, 2048-bit key, N float values in [-1, 1):
  (a) encrypt + decrypt of N ciphertexts;
  (b) encrypt_packed + decrypt_packed at --slot-bits (default 64), with the codec kernels (pai_fp_pack / pai_fp_unpack) on
      their own and the bytes they move;
  (c) for N existing ciphertexts — equal exponents, and the exponents of np.random.randn floats as in tools/segsum_time.py —
      pack (pai_ct_pack on the default dispatch, on route A alone: PAI_DISABLE=pack_padic, and on route B alone: PAI_TUNE
      pack_padic_min=0) + decrypt_packed against decrypt of all N, beside the in-chain product time of the same run
      (pai_ct_mont_mul over N); then the chain alone on both routes over a sweep of batch sizes (where the hand-over belongs).
Medians of --reps interleaved runs, the spread (max - min) beside them.  One JSON line per figure, also appended to --out (default profiles/r09/pack_time.jsonl).
usage: python tools/pack_time.py [--bits 2048] [--n 1048576] [--slot-bits 64] [--reps 5] [--out FILE]"""
import argparse, json, os, statistics, sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch
import bench
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, fixedpoint, packed
from pailliercryptolib_python_amd.bindings import ipclCipherText, ipclPublicKey
from pailliercryptolib_python_amd.paillier import PaillierEncryptedNumber

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, default=2048)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--slot-bits", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=str(ROOT / "profiles" / "r09" / "pack_time.jsonl"))
a = ap.parse_args()
key = bench.synthetic_key(a.bits)
pk = PaillierPublicKey(ipclPublicKey(key.n, a.bits, True, hs=key.hs, randbits=key.randbits))
sk = PaillierPrivateKey(pk, key.p, key.q)
h = pk.pubkey.handle
dev = h.device
N, b = a.n, a.slot_bits
k = packed.max_slots(key.n.bit_length(), b)
G = (N + k - 1) // k
E, v = 40, 41                                        # mantissas rint(x 2^40), |m| <= 2^40
rng = np.random.default_rng(1)
x = rng.uniform(-1, 1, N)
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
sink = open(a.out, "a")


def emit(row):
    row = {"bits": a.bits, "n": N, "slot_bits": b, "slots": k, **row}
    line = json.dumps(row)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def once(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def medians(fns, reps):
    """{name: median ms} of `reps` interleaved rounds over the named callables (one warm-up round first)"""
    for f in fns.values():
        once(f)
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, f in fns.items():
            ts[name].append(once(f)[0])
    return {name: statistics.median(t) for name, t in ts.items()}, {name: max(t) - min(t) for name, t in ts.items()}


# ---- (a) / (b): from plaintext values ----------------------------------------------------------------------------------------
enc = pk.encrypt(x)
pkd = pk.encrypt_packed(x, exponent=E, value_bits=v, slot_bits=b)
xs = torch.from_numpy(x).to(dev)
rows, _ = h.fp_pack(xs, E, v, b, k)
med, spread = medians({
    "encrypt": lambda: pk.encrypt(x),
    "decrypt": lambda: sk.decrypt_to_numpy(enc),
    "encrypt_packed": lambda: pk.encrypt_packed(x, exponent=E, value_bits=v, slot_bits=b),
    "decrypt_packed": lambda: sk.decrypt_packed(pkd),
    "fp_pack": lambda: h.fp_pack(xs, E, v, b, k),
    "fp_unpack": lambda: h.fp_unpack(rows, b, k),
}, a.reps)
assert np.array_equal(sk.decrypt_packed(pkd), np.ldexp(np.rint(np.ldexp(x, E)), -E))
scale = (1 << 20) / N
emit({"what": "a_encrypt_decrypt", "encrypt_ms": med["encrypt"], "decrypt_ms": med["decrypt"],
      "ms_per_2p20": scale * (med["encrypt"] + med["decrypt"]), "spread_ms": spread["encrypt"] + spread["decrypt"]})
emit({"what": "b_encrypt_packed_decrypt_packed", "encrypt_packed_ms": med["encrypt_packed"], "decrypt_packed_ms": med["decrypt_packed"],
      "ms_per_2p20": scale * (med["encrypt_packed"] + med["decrypt_packed"]),
      "speedup_vs_a": (med["encrypt"] + med["decrypt"]) / (med["encrypt_packed"] + med["decrypt_packed"]),
      "spread_ms": spread["encrypt_packed"] + spread["decrypt_packed"]})
pack_bytes = 8 * N + 4 * h.n_words * G
unpack_bytes = 4 * h.n_words * G + 8 * G * k * (2 if b > 64 else 1) + 4 * G
emit({"what": "codec", "fp_pack_ms": med["fp_pack"], "fp_pack_bytes": pack_bytes, "fp_pack_GBps": pack_bytes / med["fp_pack"] / 1e6,
      "fp_unpack_ms": med["fp_unpack"], "fp_unpack_bytes": unpack_bytes, "fp_unpack_GBps": unpack_bytes / med["fp_unpack"] / 1e6})
del enc, pkd

# ---- (c): from existing ciphertexts --------------------------------------------------------------------------------------------
g = torch.Generator(device=dev)
g.manual_seed(1)
ct = torch.randint(-(1 << 31), 1 << 31, (N, h.ct_words), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
ct[:, -1] &= 0x3FFFFFFF              # below n^2 for the fixture keys
ct = ct.contiguous()
for kind in ("equal", "randn"):
    expo = np.zeros(N, np.int32) if kind == "equal" else fixedpoint.float64_mantissas(rng.standard_normal(N))[1].astype(np.int32)
    xe = PaillierEncryptedNumber(pk, ipclCipherText(pk.pubkey, ct), expo, N)
    bb = b if kind == "equal" else max(b, 100)       # randn: the aligned mantissas of N(0, 1) floats need wider slots
    kk = packed.max_slots(key.n.bit_length(), bb)

    def forced(route, f):
        """f under one forced route of pai_ct_pack ("a": the k_segprod levels, "b": digit pairs for every batch)"""
        def g():
            os.environ["PAI_DISABLE" if route == "a" else "PAI_TUNE"] = "pack_padic" if route == "a" else "pack_padic_min=0"
            try:
                return f()
            finally:
                os.environ.pop("PAI_DISABLE", None)
                os.environ.pop("PAI_TUNE", None)
        return g

    def decrypt_like_packed():
        """what decrypt_packed does (decrypt the rows, unpack on the device, flags and mantissas to the host), without its
        OverflowError: the plaintexts of random ciphertexts lie outside the packed range"""
        out, flag = h.fp_unpack(sk.prikey.decrypt_words(p.ciphertext().words), bb, kk)
        return flag.cpu(), out.cpu()

    do_pack = lambda: xe.pack(slot_bits=bb, value_bits=bb - 1)
    p = xe.pack(slot_bits=bb, value_bits=bb - 1)
    raised = xe.increase_exponent_to(xe.words, expo, int(expo.max()))
    med, spread = medians({
        "decrypt_all": lambda: sk.prikey.decrypt_words(ct),
        "pack": do_pack,
        "pack_route_a": forced("a", do_pack),
        "pack_route_b": forced("b", do_pack),
        "chain_route_a": forced("a", lambda: h.ct_pack(raised, bb, kk)),
        "chain_route_b": forced("b", lambda: h.ct_pack(raised, bb, kk)),
        "decrypt_rows": lambda: sk.prikey.decrypt_words(p.ciphertext().words),
        "decrypt_packed": decrypt_like_packed,
        "in_chain_product": lambda: h.ct_mont_mul(ct, ct),
    }, a.reps)
    emit({"what": "c_pack_existing", "exponents": kind, "slot_bits": bb, "slots": kk, "decrypt_all_ms": med["decrypt_all"],
          "pack_ms": med["pack"], "pack_route_a_ms": med["pack_route_a"], "pack_route_b_ms": med["pack_route_b"],
          "route_a_over_route_b": med["pack_route_a"] / med["pack_route_b"],
          "chain_route_a_ms": med["chain_route_a"], "chain_route_b_ms": med["chain_route_b"],
          "decrypt_rows_ms": med["decrypt_rows"], "decrypt_packed_ms": med["decrypt_packed"],
          "pack_plus_decrypt_packed_ms_per_2p20": scale * (med["pack"] + med["decrypt_packed"]),
          "decrypt_all_ms_per_2p20": scale * med["decrypt_all"],
          "speedup_vs_decrypt_all": med["decrypt_all"] / (med["pack"] + med["decrypt_packed"]),
          "in_chain_product_ms": med["in_chain_product"], "chain_products_route_a": N * (bb + 2),
          "route_a_chain_rate_vs_in_chain": (N * (bb + 2) / med["chain_route_a"]) / (N / med["in_chain_product"]),
          "spread_ms": {n_: round(s_, 3) for n_, s_ in spread.items()}})
    if kind == "equal":
        # the hand-over (csrc/path_ranges.hpp: pack_padic_min_rows): both routes over the number of output rows
        for rows_out in (2048, 4096, 8192, 12288, 16384, 24576):
            sub = raised[:rows_out * kk].contiguous()
            m2, s2 = medians({"a": forced("a", lambda: h.ct_pack(sub, bb, kk)), "b": forced("b", lambda: h.ct_pack(sub, bb, kk))}, a.reps)
            emit({"what": "route_sweep", "rows_out": rows_out, "slot_bits": bb, "slots": kk, "route_a_ms": m2["a"], "route_b_ms": m2["b"],
                  "spread_ms": {n_: round(s_, 3) for n_, s_ in s2.items()}})
