"""CPU: the prime pairs of tests/golden/limit_keys.json (tests/golden/make_limit_keys.py) are what the fixture claims — primes of
equal width whose n^2 has exactly 29 NL - 2 bits, the widest modulus the Montgomery geometry of NL limbs admits (csrc/paillier_capi.hip:
geo_for_bits / geo_latency_for_bits, 29 NL >= bits + 2), with R / n^2 within 2^-200 of 4 (`hi`) or of 8 (`lo`), R = 2^(29 NL) —
and are sound Paillier keys under the oracle.  The kernels meet them in tests/test_gpu_aggregate_limits.py.

The most-significant-limb-first product (csrc/mont_msb.hpp, tools/msb_model.py) is held on these moduli wherever the model's
own admission conditions accept them; they accept none: at the limit of its own geometry n^2 has its top limb in limb NL - 1
(off = 0), and the latency limits on their lane-group geometries have 27 bits in the top limb (tb <= 26 is required) — the
same conditions csrc/paillier_capi.hip: build_msb_ctx refuses, so pai_ct_add takes the Montgomery products on every limit key."""
import importlib.util
import json
import math
from pathlib import Path

import pytest

from oracle import paillier_oracle as orc

RB = 29
LANE_GROUP_NL = (36, 72, 112, 144, 224, 288)
LATENCY_NL = (48, 96, 192)
MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
# lane-group geometries as (limbs per lane, lanes, rows per block): csrc/geo_36x1.hip ... geo_36x8.hip
LANE_GROUP_GEO = {36: (36, 1, 6), 72: (36, 2, 6), 112: (28, 4, 4), 144: (36, 4, 6), 224: (28, 8, 4), 288: (36, 8, 6)}


def load_limit_keys():
    """[(id, kind, nl, engine, prime_bits, p, q)] in the fixture's order (by limb count, `hi` before `lo`)."""
    fx = json.loads((Path(__file__).parent / "golden" / "limit_keys.json").read_text())
    return [(f"{e['kind']}-nl{e['nl']}", e["kind"], e["nl"], e["engine"], e["prime_bits"], int(e["p"], 16), int(e["q"], 16)) for e in fx]


ENTRIES = load_limit_keys()
IDS = [e[0] for e in ENTRIES]


def lane_group_nl(bits):
    """limbs of the lane-group geometry geo_for_bits gives a modulus of `bits` bits"""
    return next(nl for nl in LANE_GROUP_NL if RB * nl >= bits + 2)


def miller_rabin(n):
    if n < 2 or any(n % b == 0 for b in MR_BASES):
        return n in MR_BASES
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_fixture_covers_every_geometry():
    got = [(kind, nl, engine) for _, kind, nl, engine, _, _, _ in ENTRIES]
    want = sorted([("hi", nl, "lane_group") for nl in LANE_GROUP_NL] + [("lo", nl, "lane_group") for nl in LANE_GROUP_NL] +
                  [("hi", nl, "latency") for nl in LATENCY_NL], key=lambda t: (t[1], t[0]))
    assert got == want and len(ENTRIES) == 15
    assert [e[4] * 2 - 1 for e in ENTRIES if e[1] == "hi"] == [521, 695, 1043, 1391, 1623, 2087, 2783, 3247, 4175]      # bits of n


@pytest.mark.parametrize("ident,kind,nl,engine,pb,p,q", ENTRIES, ids=IDS)
def test_structure(ident, kind, nl, engine, pb, p, q):
    assert p != q and p.bit_length() == pb and q.bit_length() == pb
    assert miller_rabin(p) and miller_rabin(q)
    n = p * q
    M, R = n * n, 1 << (RB * nl)
    assert math.gcd(n, (p - 1) * (q - 1)) == 1 and n.bit_length() > 16 and n & 1
    assert M.bit_length() == RB * nl - 2
    if kind == "hi":                                                # 4 < R / M < 4 + 2^-200
        assert 4 * M < R and (R - 4 * M) << 200 < M
    else:                                                           # 8 - 2^-200 < R / M < 8
        assert R < 8 * M and (8 * M - R) << 200 < M
    if engine == "lane_group":
        assert lane_group_nl(M.bit_length()) == nl                  # the geometry n^2 itself lives on, nothing to spare
    else:
        assert next(l for l in (48, 96, 192, 288) if RB * l >= M.bit_length() + 2) == nl
        assert lane_group_nl(M.bit_length()) > nl                   # the chain kernels run these keys with room above n^2


@pytest.mark.parametrize("ident,kind,nl,engine,pb,p,q", ENTRIES, ids=IDS)
def test_oracle_roundtrip(ident, kind, nl, engine, pb, p, q, monkeypatch):
    key = orc.make_key(p, q, djn_x=0x1234567, bits=2 * pb)
    n = key.n
    consts = orc.crt_constants(key)                       # (decrypt_crt derives them at every call: half of its time at the wide keys)
    monkeypatch.setattr(orc, "crt_constants", lambda k: consts)
    cts = {m: orc.encrypt(key, m, 0xFEDCBA9876543211 + m % 7) for m in (0, 1, n - 1, n // 2)}
    for m, c in cts.items():
        assert orc.decrypt_crt(key, c) == m
    assert orc.decrypt_lambda(key, cts[n // 2]) == n // 2


def test_msb_first_product_model_admits_no_limit_modulus():
    """tools/msb_model.py on n^2 of every limit key, on the lane-group geometry that serves it: the product is checked wherever the
    model's admission conditions (Params.ok: 3 .. 26 bits in the top limb, the modulus shifted up by at least one limb) hold.
    They hold for none of the fifteen — which is the hand-down tests/test_gpu_aggregate_limits.py sees (k_modmul, never
    k_modmul_msb) — and the reason is asserted per key."""
    spec = importlib.util.spec_from_file_location("msb_model", Path(__file__).resolve().parent.parent / "tools" / "msb_model.py")
    mm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mm)
    admitted = []
    for ident, kind, nl, engine, pb, p, q in ENTRIES:
        M = (p * q) ** 2
        g = lane_group_nl(M.bit_length())
        if g == 36:
            continue                                                # one lane per integer: no most-significant-limb-first kernel (csrc/geo_inst.hpp)
        par = mm.Params(M, *LANE_GROUP_GEO[g])
        if par.ok:
            admitted.append(ident)
            full = (1 << (M.bit_length() + 2)) - 1                  # the widest row build_msb_ctx admits: < 8 M
            stats = {}
            for a, b in ((M - 1, M - 1), (1, 1), (0, 5), (full, full), (full, M - 1), (M - 1, p * q)):
                assert mm.msb_mul(par, a, b, stats) == a * b % M
            assert stats["qmax"] <= 2 * mm.B + 8
        elif engine == "lane_group":
            assert par.off == 0, ident                              # n^2 fills its geometry: no limb to shift the modulus up by
        else:
            assert par.off >= 1 and par.tb == 27, ident             # 29 NL - 2 bits: 27 of them in the top limb
    assert admitted == []
