"""Generators and models of the differential fuzz for the extension entry points of the C ABI (tests/test_gpu_fuzz_ext.py,
tools/fuzz_ext_gpu.py; held to independent restatements in tests/test_fuzz_ext_cpu.py).  Pure Python: no device, no handle.

    case(family, key, seed, round) -> dict

is a function of its arguments and nothing else (the generator is random.Random seeded with their text).  `key` is anything with
the fields of oracle.paillier_oracle.OracleKey (n, p, q, nsq, bits, hs, randbits, max_int): a real key, or a toy key of a few
dozen bits in the CPU tests.  A case holds the family, the key bits, the round, `runs` — the knob settings the call is repeated
under, each {"tune": {name: value}, "disable": [names]} with the same expectation —, the operands as Python ints and numpy index
arrays in the wire form (the runner moves them to the case's domain tag), and the expected outputs.  `shape` names what the case
contains (tests/test_fuzz_ext_cpu.py asserts the classes by name over the schedule of the GPU tests).

Families: segprod (pai_ct_segment_prod), scan (pai_ct_scan), smexp (pai_ct_sparse_multiexp), pack (pai_ct_pack, pai_ct_pack_step),
open (pai_recover_r, pai_opening_fold), crtenc (pai_encrypt_crt, pai_obfuscate_crt), tpart (pai_keyshare_create,
pai_partial_decrypt), tcomb (pai_threshold_combine).  Operands are units modulo n (one row that shares a factor with n hides every
product behind it); the exceptions are placed on purpose and named in the case.

Rounds: round r is DIRTY when r % 8 == 1 (segprod, scan, smexp: rows, shifts, bases and offsets the calls must survive; the
status bit is expected and cleared).  The garbage on a chain's first shift / a run's first step is never applied; the header
documents that a NEGATIVE value there still sets the status bit, so the garbage is positive in the clean rounds (status 0) and
takes both signs in the dirty rounds and in the rounds with rnd % 4 == 2 (`first_negative`: the bit is expected, nothing else
changes)."""
from __future__ import annotations

import math
import random

import numpy as np

from tests._util import djn_encrypt_many, djn_obfuscate_many, pow_many

FAMILIES = ("segprod", "scan", "smexp", "pack", "open", "crtenc", "tpart", "tcomb")
KEY_CLASSES = {"digit36": (1024,), "digit72": (1408, 1536, 2048), "lanes": (2304, 2560, 3072), "wide": (3328, 3584, 4096)}
ROUNDS = {"digit36": 6, "digit72": 4, "lanes": 3, "wide": 2}          # per GPU test; a family may set its own (ROUNDS_FOR)
ROUNDS_FOR = {("tpart", "digit72"): 3}                                # (two full-length exponents over up to 513 rows per round)
for _cls in KEY_CLASSES:
    ROUNDS_FOR[("scan", _cls)] = 7                                     # cheap: every run length of SCAN_SEG in every class
    ROUNDS_FOR[("tcomb", _cls)] = max(ROUNDS[_cls], 4)                 # cheap: the four round kinds (signs, t) in every class
SEED = 20261020
SEGPROD_CHUNKS = (None, 1, 2, 3, 7)
SCAN_CHUNKS = (None, 1, 2, 3, 5)
SMEXP_CHUNKS = (None, 1, 2, 3)
OPEN_CHUNKS = (None, 1, 2, 3)
OPEN_WBITS = (None, 1, 2, 3, 4)
SCAN_SEG = (1, 2, 3, 5, 64, 65, "N")
SMEXP_EBITS = (1, 7, 53, 64, 100)
OPEN_EBITS = (1, 31, 32, 64, 128, 256)
OPEN_SEG = (1, 2, 7, 64, 65, "N", "N+3")
CRT_N = (1, 63, 64, 65, 255, 256, 257)
TPART_N = (1, 255, 256, 257, 513)
TPART_SMALL = (1, 2, 3, 63, 64)
FB_WBITS = 6                       # the window of the fixed-base tables in the crtenc family (small tables, built in milliseconds)


def rounds_for(family, cls):
    return ROUNDS_FOR.get((family, cls), ROUNDS[cls])


def key_bits_for(cls, rnd):
    sizes = KEY_CLASSES[cls]
    return sizes[rnd % len(sizes)]


def class_of(bits):
    """the key class a modulus of `bits` bits belongs to (toy keys: digit36, the class without row caps)"""
    for cls, sizes in KEY_CLASSES.items():
        if bits in sizes:
            return cls
    return "digit36" if bits < 2304 else ("lanes" if bits < 3328 else "wide")


def digit_served(n_bits):
    """csrc/padic_enc_kernels.hip: padic_enc_nl_for_n_bits — the moduli the base-n digit engine serves"""
    return 700 <= n_bits <= 1024 or 1400 <= n_bits <= 2068


def crt_served(key):
    """csrc/dispatch_encrypt_crt.hpp: crt_enc_nl — both primes on one instantiation of the digit engine"""
    a, b = key.p.bit_length(), key.q.bit_length()
    band = lambda v: 1 if 700 <= v <= 1024 else (2 if 1400 <= v <= 2068 else 0)
    return band(a) != 0 and band(a) == band(b)


def rng_for(family, key, seed, rnd):
    return random.Random(f"{family}/{key.bits}/{key.n % (1 << 64)}/{seed}/{rnd}")


def knobs(tune=None, disable=()):
    return {"tune": dict(tune or {}), "disable": list(disable)}


# ---- operands ------------------------------------------------------------------------------------------------------------------
def pattern(rng, M, count):
    """tools/fuzz_gpu.py: values next to 0 and M, runs of ones, ones on top, single bits, random"""
    bits = M.bit_length()
    out = []
    for _ in range(count):
        k = rng.randrange(8)
        if k == 0:
            v = rng.randrange(3)
        elif k == 1:
            v = M - 1 - rng.randrange(3)
        elif k == 2:
            v = (1 << rng.randrange(1, bits)) - 1
        elif k == 3:
            v = ((1 << bits) - 1) ^ ((1 << rng.randrange(1, bits)) - 1)
        elif k == 4:
            v = 1 << rng.randrange(bits)
        else:
            v = rng.getrandbits(bits + 64)
        out.append(v % M)
    return out


def units(rng, key, M, count):
    """pattern() with every value moved up to the next unit modulo n"""
    out = []
    for v in pattern(rng, M, count):
        while math.gcd(v, key.n) != 1:
            v = (v + 1) % M
        out.append(v)
    return out


def non_unit(rng, key):
    """a multiple of p that is neither 0 nor a multiple of q"""
    while True:
        v = key.p * rng.randrange(1, key.nsq // key.p) % key.nsq
        if v % key.q:
            return v


def exponents(rng, ebits, count):
    """`count` values below 2^ebits: 0 and all ones among them"""
    out = [rng.getrandbits(ebits) for _ in range(count)]
    if count >= 1:
        out[rng.randrange(count)] = (1 << ebits) - 1
    if count >= 2:
        out[rng.randrange(count)] = 0
    return out


def prod(vals, M):
    acc = 1
    for v in vals:
        acc = acc * v % M
    return acc


# ---- segment structure -----------------------------------------------------------------------------------------------------------
def segments(rng, rnd, cap):
    """member counts of the segments of one case, at most `cap` members in all.  Round kinds: rnd % 4 == 3 random small
    structure; other even rounds one segment of 257 / 256 members (in turn) holding more than half of all; other odd rounds
    segments of 64 and 65 members beside the majority segment (256 members where the cap allows).  (A cap below 280 members
    scales the long segments down.)  The structured kinds have 21 to 30 non-empty segments and three empty ones: at the front, in the middle, at the end."""
    if rnd % 4 == 3:
        S = rng.randrange(1, 31)
        lens = [rng.choice((1, 1, 2, 3, 5)) for _ in range(S)]
        if S >= 8:
            lens[rng.choice((0, S // 2, S - 1))] = 0
        while sum(lens) > cap:
            lens[lens.index(max(lens))] = 1
        if sum(lens) == 0:
            lens[0] = 1
        return lens
    nf = 21 if cap < 100 else (20 if cap <= 300 else rng.randrange(20, 28))
    fill = [1] * nf
    if rnd % 2 == 0:
        body = [(257 if rnd % 4 == 0 else 256) if cap >= 280 else cap * 3 // 5]
    elif cap >= 280:
        body = [64, 65, 256 if cap >= 600 else 129 + nf + 1 + rng.randrange(min(8, cap - (259 + 2 * nf)) + 1)]
    else:
        body = [cap // 2 + 1 + rng.randrange(3)]
    spare = min(cap - sum(body) - nf, max(body) - (sum(body) - max(body)) - nf - 1)
    assert spare >= 0, (cap, body, nf)
    for _ in range(min(spare, rng.randrange(0, 40))):
        fill[rng.randrange(nf)] += 1
    lens = body + fill
    rng.shuffle(lens)
    lens = [0] + lens[:len(lens) // 2] + [0] + lens[len(lens) // 2:] + [0]
    assert 2 * max(lens) > sum(lens) and sum(lens) <= cap and 8 * 3 <= len(lens)
    return lens


def seg_classes(lens):
    """the shape classes a list of member counts contains, by name"""
    out = set()
    S, total = len(lens), sum(lens)
    if S >= 2 and lens[0] == 0:
        out.add("empty_front")
    if S >= 2 and lens[-1] == 0:
        out.add("empty_end")
    if any(v == 0 for v in lens[1:-1]):
        out.add("empty_middle")
    if 1 in lens:
        out.add("single_member")
    if lens and 2 * max(lens) > total and S > 1:
        out.add("majority")
    for v in (64, 65, 256, 257):
        if v in lens:
            out.add(f"len{v}")
    return out


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- pai_ct_segment_prod ------------------------------------------------------------------------------------------------------------
def model_segprod(cts, N, rows, shift, offsets, M):
    """the chain of the header: acc <- acc^(2^shift_j) * ct[rows_j], the first member's shift ignored, an empty chain 1; a row
    >= N is skipped and a negative shift counts as 0"""
    out = []
    for s in range(len(offsets) - 1):
        acc = None
        for j in range(int(offsets[s]), int(offsets[s + 1])):
            r = j if rows is None else int(rows[j])
            if r >= N:
                continue
            sh = 0 if shift is None else max(0, int(shift[j]))
            acc = cts[r] if acc is None else pow(acc, 1 << sh, M) * cts[r] % M
        out.append(1 if acc is None else acc)
    return out


def case_segprod(key, seed, rnd):
    rng = rng_for("segprod", key, seed, rnd)
    M, cls = key.nsq, class_of(key.bits)
    dirty = rnd % 8 == 1
    lens = segments(rng, rnd, 600)
    offsets = offsets_of(lens)
    members = int(offsets[-1])
    ncap = 80 if cls == "wide" else 600
    gather = dirty or members > ncap or rng.randrange(2) == 1
    N = rng.randrange(1, min(ncap, members) + 1) if gather else members
    cts = units(rng, key, M, N)
    rows = np.array([rng.randrange(N) for _ in range(members)], dtype=np.uint32) if gather else None
    shift = None
    first_negative = dirty or rnd % 4 == 2
    if first_negative or rng.randrange(3):
        shift = np.array([rng.randrange(4) for _ in range(members)], dtype=np.int32)
        for s, ln in enumerate(lens):
            if ln:
                g = 1000 + rng.randrange(1 << 20)                            # a chain's first shift: garbage, never applied
                shift[offsets[s]] = -g if first_negative and rng.randrange(2) else g
    planted = None
    if not dirty and rng.randrange(2) and len(lens) >= 16:
        # a non-unit as the LAST member of one chain, on a row of its own (1 chain in >= 16)
        s = rng.choice([i for i, ln in enumerate(lens) if ln and 2 * ln <= members])
        j = int(offsets[s + 1]) - 1
        if gather:
            cts.append(non_unit(rng, key))
            N += 1
            rows[j] = N - 1
        else:
            cts[j] = non_unit(rng, key)
        planted = s
    if dirty:
        for j in rng.sample(range(members), min(members, 5)):
            rows[j] = N + rng.randrange(3) if rng.randrange(2) else 0xFFFFFFFF - rng.randrange(3)
        inner = [j for j in range(members) if j not in set(int(o) for o in offsets)]
        for j in rng.sample(inner, min(len(inner), 5)):
            shift[j] = -1 - rng.randrange(1 << 20)
    if first_negative:
        shift[offsets[lens.index(max(lens))]] = -7                            # (at least one, on the longest chain)
    return {"family": "segprod", "bits": key.bits, "round": rnd, "dirty": dirty, "first_negative": first_negative,
            "status_bit": 4 if first_negative else 0,
            "runs": [knobs({"segprod_chunk": c}) for c in SEGPROD_CHUNKS],
            "N": N, "tag": rng.randrange(-2, 3), "cts": cts, "rows": rows, "shift": shift, "offsets": offsets, "S": len(lens),
            "planted_non_unit": planted, "shape": seg_classes(lens) | {"gather" if gather else "rows_null", "shift" if shift is not None else "shift_null"} | ({"first_negative"} if first_negative else set()),
            "want": model_segprod(cts, N, rows, shift, offsets, M)}


# ---- pai_ct_scan ------------------------------------------------------------------------------------------------------------------------
def model_scan(cts, raise_, step, L, reverse, M):
    """acc_first = ct^(2^raise), acc_i = acc_prev^(2^step_i) * ct_i^(2^raise_i) along each run of L rows in scan order; a
    negative raise or step counts as 0 (tests/test_gpu_cumsum.py: want_chain, with the clamp)"""
    N = len(cts)
    out = [None] * N
    for base in range(0, N, L):
        acc = None
        for p in range(L):
            i = base + (L - 1 - p if reverse else p)
            v = pow(cts[i], 1 << (0 if raise_ is None else max(0, int(raise_[i]))), M)
            acc = v if p == 0 else pow(acc, 1 << (0 if step is None else max(0, int(step[i]))), M) * v % M
            out[i] = acc
    return out


def case_scan(key, seed, rnd):
    rng = rng_for("scan", key, seed, rnd)
    M, cls = key.nsq, class_of(key.bits)
    dirty = rnd % 8 == 1
    cap = 80 if cls == "wide" else 600
    pick = SCAN_SEG[rnd % len(SCAN_SEG)]
    if pick == "N":
        L = rng.randrange(1, cap + 1)
        runs = 1
    else:
        L = pick
        runs = rng.randrange(1, cap // L + 1)
    N = runs * L
    reverse = rnd % 2
    first_negative = dirty or rnd % 4 == 2
    cts = units(rng, key, M, N)
    arrays = {}
    for name in ("raise", "step"):
        arrays[name] = None
        if first_negative or rng.randrange(3):
            arrays[name] = np.array([rng.randrange(4) for _ in range(N)], dtype=np.int32)
    if arrays["step"] is not None:
        for base in range(0, N, L):
            g = 1000 + rng.randrange(1 << 20)                                # a run's first step: garbage, never applied
            arrays["step"][base + (L - 1 if reverse else 0)] = -g if first_negative and (base == 0 or rng.randrange(2)) else g
    if dirty:
        first = {base + (L - 1 if reverse else 0) for base in range(0, N, L)}
        for j in rng.sample(range(N), min(N, 4)):
            arrays["raise"][j] = -1 - rng.randrange(1 << 20)
        inner = [j for j in range(N) if j not in first]
        for j in rng.sample(inner, min(len(inner), 4)):
            arrays["step"][j] = -1 - rng.randrange(1 << 20)
    return {"family": "scan", "bits": key.bits, "round": rnd, "dirty": dirty, "first_negative": first_negative,
            "status_bit": 16 if first_negative else 0,
            "runs": [knobs({"scan_chunk": c}) for c in SCAN_CHUNKS],
            "N": N, "seg_len": L, "reverse": reverse, "tag": rng.randrange(-2, 3), "dom_out": rng.randrange(-2, 3), "cts": cts,
            "raise": arrays["raise"], "step": arrays["step"],
            "shape": {f"seg_len_{pick}", f"reverse_{reverse}", "raise" if arrays["raise"] is not None else "raise_null",
                      "step" if arrays["step"] is not None else "step_null"} | ({"first_negative"} if first_negative else set()),
            "want": model_scan(cts, arrays["raise"], arrays["step"], L, reverse, M)}


# ---- pai_ct_sparse_multiexp ---------------------------------------------------------------------------------------------------------------
def clean_offsets(offsets, T):
    """csrc/kernels_codec.hpp: k_smexp_offsets — the running maximum of the offsets clamped to [0, T]"""
    out, run = [], 0
    for v in offsets:
        run = max(run, min(max(int(v), 0), T))
        out.append(run)
    return out


def model_smexp(base, inv, N, bidx, e, sign, offsets, T, M):
    """out[s] = prod B_t^(e_t) over the terms of segment s, B_t = base or inverse by sign; a base outside [0, N) is skipped,
    offsets are cleaned as the kernel documents; the powers through pow_many"""
    ok = [0 <= int(b) < N for b in bidx]
    pw = pow_many([(inv if sign is not None and sign[t] else base)[int(bidx[t])] if ok[t] else 1 for t in range(T)], list(e), M)
    off = clean_offsets(offsets, T)
    return [prod([pw[t] for t in range(off[s], off[s + 1]) if ok[t]], M) for s in range(len(off) - 1)]


def case_smexp(key, seed, rnd):
    rng = rng_for("smexp", key, seed, rnd)
    M, cls = key.nsq, class_of(key.bits)
    dirty = rnd % 8 == 1
    lens = segments(rng, rnd, 60 if cls == "wide" else 300)
    offsets = offsets_of(lens)
    T = int(offsets[-1])
    N = rng.randrange(1, 41)
    base = units(rng, key, M, N)
    signed = rng.randrange(2) == 1
    inv = [pow(x, -1, M) for x in base] if signed else None
    ebits = SMEXP_EBITS[(rnd + key.bits // 128) % len(SMEXP_EBITS)]
    e = exponents(rng, ebits, T)
    bidx = np.array([rng.randrange(N) for _ in range(T)], dtype=np.int32)
    sign = np.array([rng.randrange(2) for _ in range(T)], dtype=np.uint8) if signed else None
    if dirty:
        for t in rng.sample(range(T), min(T, 5)):
            bidx[t] = N + rng.randrange(3) if rng.randrange(2) else -1 - rng.randrange(3)
        s = 1 + rng.choice([i for i, ln in enumerate(lens) if ln >= 10])
        offsets[s] = int(offsets[s]) - 3 - rng.randrange(5)                   # steps back (the long segment before it keeps terms)
        offsets[0] = -3                                                       # leaves [0, T] on either side
        offsets[len(offsets) - 2] = T + 7
    return {"family": "smexp", "bits": key.bits, "round": rnd, "dirty": dirty, "status_bit": 8 if dirty else 0,
            "runs": [knobs({"smexp_chunk": c}) for c in SMEXP_CHUNKS], "second_handle_padic_off": digit_served(key.n.bit_length()),
            "N": N, "T": T, "S": len(lens), "base": base, "inv": inv, "bidx": bidx, "e": e, "e_words": (ebits + 31) // 32, "ebits": ebits,
            "sign": sign, "offsets": offsets,
            "shape": seg_classes(lens) | {f"ebits_{ebits}", "signed" if signed else "unsigned", "e_ones"} | ({"e_zero"} if 0 in e else set()),
            "want": model_smexp(base, inv, N, bidx, e, sign, offsets, T, M)}


# ---- pai_ct_pack / pai_ct_pack_step -----------------------------------------------------------------------------------------------------------
def model_pack_step(cts, step, count, M):
    """out[g] = prod_(j < count) ct[g count + j]^(2^(step j)), a ragged last chain multiplying the rows it has (tests/
    test_gpu_packed.py: want_packed, tests/test_gpu_packed_rows.py: want_stepped)"""
    pw = pow_many(cts, [1 << (step * (i % count)) for i in range(len(cts))], M)
    return [prod(pw[g:g + count], M) for g in range(0, len(cts), count)]


def case_pack(key, seed, rnd):
    rng = rng_for("pack", key, seed, rnd)
    M, cls = key.nsq, class_of(key.bits)
    nb = key.n.bit_length()
    cap = 80 if cls == "wide" else (200 if cls == "lanes" else 600)

    def layout(lo, extreme):
        b = {0: min(128, nb - 2), 1: lo}.get(extreme, rng.randrange(lo, min(128, nb - 2) + 1))     # 128-bit slots with k = 1, 8-bit slots with the most
        kmax = (nb - 2) // b
        k = {0: 1, 1: kmax}.get(extreme, rng.randrange(1, kmax + 1))
        G = rng.randrange(1, max(1, min(70, cap // k)) + 1)
        n_rows = max(1, G * k - (rng.randrange(k) if k > 1 else 0))           # ragged against k
        return b, k, kmax, n_rows

    b, k, kmax, N = layout(8, rnd % 3)
    step, count, _, N2 = layout(8, 2)
    rows = units(rng, key, M, max(N, N2))
    return {"family": "pack", "bits": key.bits, "round": rnd,
            "runs": [knobs({"pack_padic_min": 0}), knobs(disable=["pack_padic"])],
            "tag": 0 if rnd % 2 == 0 else (-2, -1, 1, 2)[(rnd // 2 + key.bits // 128 % 5) % 4],    # (the digit route takes wire-form rows only)
            "cts": rows, "N": N, "slot_bits": b, "slots": k, "N_step": N2, "step_bits": step, "count": count,
            "shape": {"slots_1" if k == 1 else ("slots_max" if k == kmax else "slots_mid"), "ragged" if N % k else "full"},
            "want": model_pack_step(rows[:N], b, k, M), "want_step": model_pack_step(rows[:N2], step, count, M)}


# ---- pai_recover_r, pai_opening_fold --------------------------------------------------------------------------------------------------------------
def model_recover(key, c):
    """the header's arithmetic: r_s = (c mod s)^(n^-1 mod (s - 1)) mod s for s = p, q, Garner-lifted modulo n (r_s = 0 for a
    prime that divides c)"""
    p, q = (key.p, key.q) if key.p < key.q else (key.q, key.p)
    n = p * q
    rp = pow(c % p, pow(n % (p - 1), -1, p - 1), p)
    rq = pow(c % q, pow(n % (q - 1), -1, q - 1), q)
    return rp + p * ((rq - rp) * pow(p, -1, q) % q)


def model_fold(key, cts, ms, rs, es, L):
    """(lhs, rhs, flag) of pai_opening_fold: lhs[s] = prod ct^e, rhs[s] = (1 + n M_s) B_s^n, M_s = sum e m mod n, B_s = prod r^e
    mod n; one pow_many element per row (lhs, B) and per segment (B^n); flag bit 0: some B_s is no unit"""
    n, M = key.n, key.nsq
    pl = pow_many(cts, list(es), M)
    pb = pow_many(rs, list(es), n)
    Bs, Ms, lhs = [], [], []
    for s0 in range(0, len(cts), L):
        lhs.append(prod(pl[s0:s0 + L], M))
        Bs.append(prod(pb[s0:s0 + L], n))
        Ms.append(sum(e * m for e, m in zip(es[s0:s0 + L], ms[s0:s0 + L])) % n)
    Bn = pow_many(Bs, n, M)
    rhs = [(1 + n * m) % M * b % M for m, b in zip(Ms, Bn)]
    return lhs, rhs, int(any(math.gcd(b, n) != 1 for b in Bs))


def case_open(key, seed, rnd):
    rng = rng_for("open", key, seed, rnd)
    n, M, cls = key.n, key.nsq, class_of(key.bits)
    N = rng.randrange(2, {"digit36": 130, "digit72": 130, "lanes": 32, "wide": 16}[cls] + 1)
    ms = pattern(rng, n, N)
    rs = units(rng, key, n, N)
    rn = pow_many(rs, n, M)
    cts = [(1 + m * n) % M * v % M for m, v in zip(ms, rn)]
    want_r = list(rs)
    bad = rng.randrange(N)                                                    # the row that shares a factor with p
    cts[bad] = non_unit(rng, key)
    want_r[bad] = model_recover(key, cts[bad])
    # the fold on the same rows: half the rounds keep the bad row (its B is no unit), half enter it as the header's excluded row
    fold_ct, fold_m, fold_r = list(cts), list(ms), list(want_r)
    keep_bad = rnd % 2 == 0
    if not keep_bad:
        fold_ct[bad], fold_m[bad], fold_r[bad] = 1, 0, 1
    falsified = None
    if (rnd // 2) % 2 == 0:
        j = rng.choice([i for i in range(N) if i != bad] or [bad])
        if rng.randrange(2):
            fold_m[j] = (fold_m[j] + 1 + rng.randrange(n - 1)) % n
        else:
            fold_r[j] = (fold_r[j] * 2 + 1) % n or 1
        falsified = j
    ebits = OPEN_EBITS[(rnd + key.bits // 128) % len(OPEN_EBITS)]
    e_words = ((ebits + 31) // 32, 8, rng.randrange((ebits + 31) // 32, 9))[rnd % 3]
    es = exponents(rng, ebits, N)
    if falsified is not None and es[falsified] == 0:
        es[falsified] = 1
    pick = OPEN_SEG[(rnd + key.bits // 256) % len(OPEN_SEG)]
    L = N if pick == "N" else (N + 3 if pick == "N+3" else pick)
    c1, c2 = OPEN_CHUNKS[rnd % 4], OPEN_CHUNKS[(rnd + 2) % 4]
    lhs, rhs, flag = model_fold(key, fold_ct, fold_m, fold_r, es, L)
    return {"family": "open", "bits": key.bits, "round": rnd,
            "runs": [knobs({"open_chunk": c1, "open_wbits": OPEN_WBITS[rnd % 5]}), knobs({"open_chunk": c2}, ["open_fold"])],
            "N": N, "cts": cts, "want_r": want_r, "bad_row": bad, "fold_ct": fold_ct, "fold_m": fold_m, "fold_r": fold_r, "e": es,
            "e_words": e_words, "ebits": ebits, "seg_len": L, "falsified": falsified,
            "shape": {f"ebits_{ebits}", f"seg_len_{pick}", "falsified" if falsified is not None else "honest",
                      "bad_row_kept" if keep_bad else "bad_row_excluded", f"chunk_{c1}", f"chunk_{c2}", f"wbits_{OPEN_WBITS[rnd % 5]}"},
            "want_lhs": lhs, "want_rhs": rhs, "want_flag": flag}


# ---- pai_encrypt_crt / pai_obfuscate_crt --------------------------------------------------------------------------------------------------------------
def case_crtenc(key, seed, rnd):
    rng = rng_for("crtenc", key, seed, rnd)
    n, M, cls = key.n, key.nsq, class_of(key.bits)
    rb = key.randbits
    N = CRT_N[(rnd + key.bits // 128) % len(CRT_N)] if rnd % 3 or rnd == 0 else rng.randrange(1, 300)
    if not cls.startswith("digit"):
        N = min(N, 65 if cls == "lanes" else 33)
    rc = [0, 1, (1 << rb) - 1]
    for wb in (FB_WBITS, 18):
        windows = (rb + wb - 1) // wb
        ones = (1 << wb) - 1
        rc += [ones, ones << (wb * (windows // 2)), (ones << (wb * (windows - 1))) & ((1 << rb) - 1)]
    r = [rng.getrandbits(rb) for _ in range(N)]
    m = pattern(rng, n, N)
    o1, o2 = rng.randrange(N), rng.randrange(N)                               # (a batch shorter than the corners keeps the last ones)
    for i, v in enumerate(rc):
        r[(o1 + i) % N] = v
    for i, v in enumerate((0, n - 1, key.max_int)):
        m[(o2 + i) % N] = v
    corners = {name for name, v in (("r_zero", 0), ("r_one", 1), ("r_all_ones", (1 << rb) - 1)) if v in r}
    corners |= {"r_one_window"} if any(v in r for v in rc[3:]) else set()
    corners |= {name for name, v in (("m_zero", 0), ("m_n_minus_1", n - 1), ("m_max_int", key.max_int)) if v in m}
    cts = units(rng, key, M, N)
    served = crt_served(key)
    return {"family": "crtenc", "bits": key.bits, "round": rnd, "served": served,
            "runs": [knobs({"crtenc_min": 0, "fb_digit_wbits": FB_WBITS}), knobs({"fb_digit_wbits": FB_WBITS}, ["crtenc"])],
            "N": N, "m": m, "r": r, "cts": cts, "shape": {f"N_{N}" if N in CRT_N else "N_random"} | corners,
            "want_enc": djn_encrypt_many(key, m, r), "want_obf": djn_obfuscate_many(key, cts, r)}


# ---- pai_keyshare_create, pai_partial_decrypt ---------------------------------------------------------------------------------------------------------------
def tpart_exponents(rng, bits, rnd):
    """[(shape name, E)]: three of the small exponents and two of the four long shapes, in turn by round"""
    top = 2 * bits + 64
    out = [(f"E_{v}", v) for v in (TPART_SMALL[(3 * rnd + i) % 5] for i in range(3))]
    for kind in ((2 * rnd) % 4, (2 * rnd + 1) % 4):
        if kind == 0:
            k = top if rng.randrange(3) == 0 else rng.randrange(bits, top + 1)
            out.append(("E_pow2", 1 << k))
        elif kind == 1:
            k = top if rng.randrange(3) == 0 else rng.randrange(bits, top + 1)
            out.append(("E_pow2_minus_1", (1 << k) - 1))
        elif kind == 2:
            total = 2 * bits + 46
            run = min(rng.randrange(300, 2001), total - 40) if total >= 340 else total // 2
            low = rng.randrange(1, total - run - 20)
            hi = rng.getrandbits(total - run - low) | 1 | 1 << (total - run - low - 1)
            out.append(("E_zero_run", hi << (run + low) | rng.getrandbits(low) | 1 << (low - 1)))
        else:
            out.append(("E_random", rng.getrandbits(2 * bits + 46) | 1 << (2 * bits + 45)))
    return out


def case_tpart(key, seed, rnd):
    rng = rng_for("tpart", key, seed, rnd)
    M, cls = key.nsq, class_of(key.bits)
    N = TPART_N[(rnd + key.bits // 128) % 5] if cls.startswith("digit") else rng.randrange(1, 13 if cls == "wide" else 25)
    cts = units(rng, key, M, N)
    Es = tpart_exponents(rng, key.bits, rnd)
    tune = ({"tpart_min": 0}, {}, {"tpart_min": 0, "tpart_grid": 1})[rnd % 3]
    return {"family": "tpart", "bits": key.bits, "round": rnd, "runs": [knobs(tune)], "N": N, "cts": cts, "E": [e for _, e in Es],
            "digit_route": "tpart_min" in tune and digit_served(key.n.bit_length()),
            "shape": {name for name, _ in Es} | {f"N_{N}", "tpart_min_0" if tune else "tpart_min_unset", "tpart_grid_1" if "tpart_grid" in tune else "grid_unset"},
            "want": [pow_many(cts, e, M) for _, e in Es]}


# ---- pai_threshold_combine ---------------------------------------------------------------------------------------------------------------------------
def tcomb_magnitudes(rng, t, negs, rnd):
    """t magnitudes below 2^128: 1, 2^64, bit 127 set, random — and two or more members of one side with the same top bit"""
    shapes = ("one", "bit127", "two64", "random", "random64", "same_top", "same_top")
    mu, names = [], set()
    top = rng.randrange(2, 128)
    for j in range(t):
        s = shapes[(j + rnd) % len(shapes)]
        if s == "one":
            v = 1
        elif s == "two64":
            v = 1 << 64
        elif s == "bit127":
            v = 1 << 127 | rng.getrandbits(127)
        elif s == "random":
            v = rng.getrandbits(rng.randrange(1, 129)) or 1
        elif s == "random64":
            v = rng.getrandbits(64) or 1
        else:
            v = 1 << top | rng.getrandbits(top)
        mu.append(v)
        names.add(f"mu_{s}")
    names.discard("mu_same_top")
    for side in (False, True):
        tops = [mu[j].bit_length() for j in range(t) if bool(negs[j]) == side]
        if len(tops) != len(set(tops)):
            names.add("mu_same_top")
    return mu, names


def model_tcomb_direct(key, parts, mu, negs, theta, rows):
    """the header's definition on the given rows: x = prod parts_j^(+-mu_j) mod n^2, flagged when x != 1 mod n,
    m = ((x - 1) // n) theta mod n; {row: (flagged, m)}"""
    n, M = key.n, key.nsq
    out = {}
    for i in rows:
        x = 1
        for j, part in enumerate(parts):
            b = pow(part[i], -1, M) if negs[j] else part[i]
            x = x * pow(b, mu[j], M) % M
        out[i] = (x % n != 1, (x - 1) // n * theta % n)
    return out


def case_tcomb(key, seed, rnd):
    rng = rng_for("tcomb", key, seed, rnd)
    n, M, cls = key.n, key.nsq, class_of(key.bits)
    t = (rng.randrange(6, 16), 16, 1, rng.randrange(2, 6))[rnd % 4]
    if rnd % 4 == 0:
        negs = [0] * t
    elif rnd % 4 == 1:
        negs = [1] * t
    elif rnd % 4 == 3:
        negs = [0, 1] + [rng.randrange(2) for _ in range(t - 2)]              # both sides, t >= 2
        rng.shuffle(negs)
    else:
        negs = [rng.randrange(2) for _ in range(t)]
    mu, names = tcomb_magnitudes(rng, t, negs, rnd)
    fit = max(1, (max(mu).bit_length() + 31) // 32)
    mu_words = fit if rnd % 2 == 0 else 4
    N = rng.choice((5, 37, 256, 257) if cls == "digit36" else ((6, 65, 257) if cls == "digit72" else (4, 9, 37)))      # >= 4: every case has falsified rows
    theta = (rng.randrange(n), 1, n - 1)[rng.randrange(3)]
    sgn = [-1 if v else 1 for v in negs]
    # members paired (a, b): part_a = u^(mu_b) (1 + alpha n), part_b = u^(-s_a s_b mu_a) (1 + beta n): the powers of u cancel in
    # part_a^(s_a mu_a) part_b^(s_b mu_b); an unpaired member is 1 + alpha n
    order = list(range(t))
    rng.shuffle(order)
    alpha = [[rng.randrange(n) for _ in range(N)] for _ in range(t)]
    parts = [None] * t
    for a, b in zip(order[0::2], order[1::2]):
        u = units(rng, key, M, N)
        ui = [pow(x, -1, M) for x in u] if sgn[a] == sgn[b] else u
        pa, pb = pow_many(u, mu[b], M), pow_many(ui, mu[a], M)
        parts[a] = [x * (1 + al * n) % M for x, al in zip(pa, alpha[a])]
        parts[b] = [x * (1 + be * n) % M for x, be in zip(pb, alpha[b])]
    if t % 2:
        parts[order[-1]] = [(1 + al * n) % M for al in alpha[order[-1]]]
    want = [sum(sgn[j] * alpha[j][i] * mu[j] for j in range(t)) % n * theta % n for i in range(N)]
    # a few rows of one part replaced by unrelated units: flagged (decided by the direct definition), their m not compared
    corrupt = sorted(rng.sample(range(N), min(N // 4, rng.randrange(1, 4))))
    victim = rng.randrange(t)
    for i, v in zip(corrupt, units(rng, key, M, len(corrupt))):
        parts[victim][i] = v
    direct = model_tcomb_direct(key, parts, mu, negs, theta, corrupt)
    rowflag = [0] * N
    for i in corrupt:
        rowflag[i] = int(direct[i][0])
        want[i] = direct[i][1]                                                # (defined but meaningless: compared only when not flagged)
    # a second call per case with one row of a negative-side part replaced by a multiple of p: bit 1 (pai_ct_invert_flag leaves
    # the rows of that call undefined, so nothing else of it is compared)
    poison = None
    if any(negs) and rnd % 2 == 1:
        poison = (rng.choice([j for j in range(t) if negs[j]]), rng.randrange(N), non_unit(rng, key))
    grid = 1 if rng.randrange(2) else None
    names |= {"all_positive" if not any(negs) else ("all_negative" if all(negs) else "mixed_signs"), f"t_{t}", f"mu_words_{'4' if mu_words == 4 else 'fit'}",
              "theta_1" if theta == 1 else ("theta_n_minus_1" if theta == n - 1 else "theta_random"), "grid_1" if grid else "grid_unset"}
    if any(v >> 127 for v in mu):
        names.add("bit127")
    return {"family": "tcomb", "bits": key.bits, "round": rnd,
            "runs": [knobs({"tcomb_min": 0, "tcomb_grid": grid}), knobs({"tcomb_min": 0}, ["tcombine"])],
            "N": N, "t": t, "mu": mu, "mu_words": mu_words, "neg": negs, "theta": theta, "parts": parts, "corrupt": corrupt, "poison": poison,
            "shape": names, "want": want, "want_rowflag": rowflag}


CASES = {"segprod": case_segprod, "scan": case_scan, "smexp": case_smexp, "pack": case_pack, "open": case_open, "crtenc": case_crtenc,
         "tpart": case_tpart, "tcomb": case_tcomb}


def case(family, key, seed, rnd):
    return CASES[family](key, seed, rnd)


def reproducer(c, seed, run, what, row, got=None, want=None):
    """the one line a mismatch prints: family, key bits, seed, round, knobs, the first differing row"""
    def short(v):
        return "-" if v is None else (hex(v)[:18] + ".." if isinstance(v, int) and v > 1 << 64 else str(v))
    return (f"FUZZ-EXT MISMATCH family={c['family']} bits={c['bits']} seed={seed} round={c['round']} knobs={run} {what} first differing row={row} "
            f"got={short(got)} want={short(want)}  (python tools/fuzz_ext_gpu.py {c['round'] + 1} {seed} {c['family']} {class_of(c['bits'])})")
