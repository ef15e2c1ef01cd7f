"""CPU: the inputs of tests/test_gpu_codec_keys.py, tests/test_gpu_standard_scheme.py and test_ct_invert_direct_inputs
(tests/test_gpu_paillier_abi.py) do what they are for, on all 42 keys of tests/golden/extreme_keys.json and limit_keys.json,
without a GPU:

  * codec_inputs(key) is deterministic, its expected values are the oracle's, and orc.fp_decode inverts orc.fp_encode on every
    encoder input;
  * on the families `ones`, `zeros` and `half` n mod 2^64 is below 2^26 and at least 8 zero words follow word 1 (the minimum is at
    half-512), so that n - m of every negative float mantissa borrows across that whole run: counted on the expected encodings;
  * the `mbits + d = bits(n) - 2` block of pai_fp_encode_at moves every non-zero mantissa to its target and the block one further
    keeps the element's own exponent;
  * every unpack row carries the model flag its place in the list claims: 0 for packed rows and (-B) mod n, 1 for 2^(k b) - B and
    n - B - 1, 2 for rows >= n;
  * n of the `ones`, `zeros`, `ones_zeros` and `half` keys at 512- and 1024-bit primes has a run of more than 255 zero bits, and the
    sliding-window schedule of such an n (a restatement of csrc/paillier_capi.hip: compile_sliding_schedule) holds "no
    multiplication" entries — the case k_pow_padic must skip the table for;
  * the extended-GCD inputs are at least 40 distinct units below n^2 on every key of that test."""
import numpy as np
import pytest

from oracle import paillier_oracle as orc
from tests._util import limbs_to_ints, model_unpack
from tests.test_gpu_codec_keys import ALL_KEYS, IDS, M32, codec_inputs, zero_words_above_word_1
from tests.test_gpu_paillier_abi import INVERT_DIRECT_KEYS, invert_direct_inputs, invert_direct_key
from tests.test_gpu_standard_scheme import digit_served, longest_zero_run

BORROW_FAMILIES = ("ones", "zeros", "half")
SLIDE_BITS = 6                       # csrc/geo_ops.hpp: PADIC_SLIDE_BITS


def std_key(b, p, q):
    return orc.make_key(p, q, djn_x=None, bits=2 * b)


def test_all_42_keys_are_listed():
    assert len(ALL_KEYS) == 42 and len(set(IDS)) == 42
    assert sorted({(e[3] * e[4]).bit_length() for e in ALL_KEYS if e[1] in ("hi", "lo")}) == [521, 695, 1043, 1391, 1623, 2087, 2783, 3247, 4175]


@pytest.mark.parametrize("ident,family,b,p,q", ALL_KEYS, ids=IDS)
def test_codec_inputs(ident, family, b, p, q):
    key = std_key(b, p, q)
    n, max_int = key.n, key.n // 3 - 1
    ci, again = codec_inputs(key), codec_inputs(key)
    nw, z = ci["nw"], ci["z"]
    # deterministic
    assert np.array_equal(ci["xf"], again["xf"]) and np.array_equal(ci["xi"], again["xi"]) and ci["dec_rows"] == again["dec_rows"]
    assert ci["want_f"] == again["want_f"] and ci["want_i"] == again["want_i"]
    for t in ("at_f", "at_i"):
        assert np.array_equal(ci[t]["targets"], again[t]["targets"]) and np.array_equal(ci[t]["want_r"], again[t]["want_r"])
    assert [[c["unpack"] for c in ci["pack"]]] == [[c["unpack"] for c in again["pack"]]]
    # the codec inverts itself on every encoder input (tiny floats and -2^63 encode as 0)
    for v, (enc, ex) in zip(ci["xf"], ci["want_f"]):
        v = float(v)
        assert orc.fp_decode(enc, ex, n, max_int) == (0 if abs(v) < 1e-200 else v)
    for v, (enc, ex) in zip(ci["xi"], ci["want_i"]):
        assert ex == 0 and orc.fp_decode(enc, ex, n, max_int) == (0 if int(v) == -(2**63) else int(v))
    neg_f = [enc for v, (enc, _) in zip(ci["xf"], ci["want_f"]) if v < 0 and abs(v) >= 1e-200]
    assert len(neg_f) >= 100
    L = n % (1 << 64)
    if L < 1 << 63:                  # the integer inputs stand on both sides of the first borrow
        got = {int(v) for v in ci["xi"]}
        assert {-(L - 1), -L, -(L + 1)} <= got
    # decoder rows: both flags occur, rows >= n and the rows n - 2^(32 j) are flagged
    flags = [f for f, _ in ci["dec_want"]]
    assert flags[:8] == [0] * 8 and flags[8:] == [1] * (len(flags) - 8)
    assert sum(1 for r in ci["dec_rows"] if r >= n) >= 3 and n - (1 << (32 * z)) in ci["dec_rows"]
    # encode_at: the block at the bound moves every non-zero mantissa to its target, the block one past it keeps the exponent
    for t in ("at_f", "at_i"):
        at = ci[t]
        Lx, blk = at["L"], at["bound_block"]
        nz = np.array([m != 0 for m in at["mags"]])
        assert nz.sum() >= 200
        sl, sl1 = slice(blk * Lx, (blk + 1) * Lx), slice((blk + 1) * Lx, (blk + 2) * Lx)
        assert np.array_equal(at["want_e"][sl][nz], at["targets"][sl][nz])
        assert np.array_equal(at["want_e"][sl1][nz], at["ex0"][nz]) and (at["targets"][sl1][nz] > at["ex0"][nz]).all()
        moved = limbs_to_ints(at["want_r"][sl][nz])
        assert all(min(r, n - r).bit_length() == n.bit_length() - 2 for r in moved)                # |mantissa| 2^d fills bits(n) - 2 bits
        last = (len(at["targets"]) // Lx - 1) * Lx                                                  # d = -5: nothing moves
        assert np.array_equal(at["want_e"][last:], at["ex0"])
        assert at["bcast"][1][1][nz].tolist() == at["ex0"][nz].tolist() and (at["bcast"][1][1][~nz] == 2**31 - 1).all()
    # unpack rows: the flag each place in the list claims
    for case in ci["pack"]:
        bb, k = case["b"], case["k"]
        assert k * bb <= n.bit_length() - 2
        claimed = [f for _, f in case["unpack"]]
        assert [model_unpack(r, bb, k, n)[0] for r, _ in case["unpack"]] == claimed, (ident, bb, k)
        assert {0, 1, 2} <= set(claimed)
    assert {c["k"] for c in ci["pack"] if c["b"] == 8} >= {1, 2, (n.bit_length() - 2) // 8}
    if family in BORROW_FAMILIES:
        assert L < 1 << 26 and zero_words_above_word_1(n) >= 8, (ident, L.bit_length(), zero_words_above_word_1(n))
        for enc in neg_f:            # n - m borrowed across the whole zero run: all-ones words from word 2 up to the first non-zero word of n
            ones = 0
            while (enc >> (32 * (2 + ones))) & M32 == M32:
                ones += 1
            assert ones == z - 2 >= 8 and (enc >> (32 * z)) & M32 == ((n >> (32 * z)) & M32) - 1, (ident, ones, z)


def sliding_schedule(e):
    """csrc/paillier_capi.hip: compile_sliding_schedule — entries (squarings, table index); index 0xFF = no multiplication"""
    bit = lambda i: i >= 0 and (e >> i) & 1
    ops, i, pending, first = [], e.bit_length() - 1, 0, True
    while i >= 0:
        if not bit(i):
            pending += 1
            i -= 1
            continue
        l = min(SLIDE_BITS, i + 1)
        while not bit(i - l + 1):
            l -= 1
        val = 0
        for k in range(l):
            val = (val << 1) | bit(i - k)
        nsq = 0 if first else pending + l
        while nsq > 255:
            ops.append((255, 0xFF))
            nsq -= 255
        ops.append((nsq, val >> 1))
        first, pending = False, 0
        i -= l
    while pending > 0:
        c = min(pending, 255)
        ops.append((c, 0xFF))
        pending -= c
    return ops


def schedule_value(ops):
    """the exponent a schedule stands for"""
    e = 0
    for nsq, idx in ops:
        e <<= nsq
        if idx != 0xFF:
            e += 2 * idx + 1
    return e


@pytest.mark.parametrize("ident,family,b,p,q", [e for e in ALL_KEYS if e[2] in (512, 1024) and e[1] in ("ones", "zeros", "ones_zeros", "half")],
                         ids=[e[0] for e in ALL_KEYS if e[2] in (512, 1024) and e[1] in ("ones", "zeros", "ones_zeros", "half")])
def test_schedule_corner_of_the_digit_engine_route(ident, family, b, p, q):
    n = p * q
    assert digit_served(n.bit_length())
    assert 255 < longest_zero_run(n) <= n.bit_length()
    ops = sliding_schedule(n)
    assert schedule_value(ops) == n
    assert any(idx == 0xFF for _, idx in ops) and all(idx < 1 << (SLIDE_BITS - 1) or idx == 0xFF for _, idx in ops)
    print(f"{ident}: zero run of {longest_zero_run(n)} bits, {sum(1 for _, i in ops if i == 0xFF)} entries without a multiplication")


def test_schedule_corner_keys_are_eight():
    got = sorted(e[0] for e in ALL_KEYS if e[2] in (512, 1024) and e[1] in ("ones", "zeros", "ones_zeros", "half"))
    assert len(got) == 8
    runs = [longest_zero_run(e[3] * e[4]) for e in ALL_KEYS if e[0] in got]
    assert 330 <= min(runs) and max(runs) <= 1012, runs


@pytest.mark.parametrize("ident", INVERT_DIRECT_KEYS)
def test_extended_gcd_inputs(ident):
    key = invert_direct_key(ident)
    vals = invert_direct_inputs(key)              # asserts units below n^2 and at least 40 distinct values
    M = key.nsq
    mb = M.bit_length()
    assert {1, M - 1, 1 << (mb - 1), 1 << (mb - 2), (1 << (mb - 1)) - 1} <= set(vals)
    assert all(pow(v, -1, M) * v % M == 1 for v in vals[:12])
    cw = 2 * ((key.bits + 31) // 32)
    assert {"seeded-1024": 64, "bench-2048": 128, "seeded-3072": 192, "seeded-4096": 256, "ones-676": 86, "ones-2068": 260}.get(ident, cw) == cw
