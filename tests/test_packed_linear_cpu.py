"""CPU: linear maps of packed rows (PaillierPackedNumber.scale_rows / rmatmul / csr_rmatmul) — the headroom rule of weighted sums,
a pure-Python model of the weight quantiser (what tests/test_gpu_packed_linear.py holds pai_fp_quantize to), and every argument
check, on host containers that never touch a device.  The expectations come from Python ints and fractions.Fraction, never from
the code under test."""
from fractions import Fraction
import itertools
import json
import math
from pathlib import Path
import struct

import numpy as np
import pytest
import torch

from pailliercryptolib_python_amd import PaillierPackedNumber, PaillierPublicKey, _native, packed
from pailliercryptolib_python_amd.bindings import ipclCipherText

ROOT = Path(__file__).resolve().parents[1]
KEYS = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())


def host_key(bits=1024):
    """a public key object that never touches a device (standard scheme: nothing to precompute)"""
    return PaillierPublicKey(int(KEYS[str(bits)]["p"], 16) * int(KEYS[str(bits)]["q"], 16), bits, False)


def host_packed(pk, rows, b, k, E=10, v=20):
    return PaillierPackedNumber(pk, ipclCipherText(pk.pubkey, [1] * rows), slot_bits=b, slots=k, exponent=E, value_bits=v, length=rows * k)


def no_device(pk):
    return "_home_handle" not in vars(pk.pubkey) and not pk.pubkey._handles


# ---- the model of the quantiser (integer arithmetic on the bits of the double; no floating-point operation) ----------------------
def quantize_one(x, exponent):
    """w = rint(x 2^exponent), ties to even, for a finite Python float / numpy float64, or x << exponent for an int"""
    if isinstance(x, (int, np.integer)):
        return int(x) << exponent
    bits = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    e, frac, neg = (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1), bits >> 63
    assert e != 0x7FF, "finite values only"
    mag = frac | (1 << 52) if e else frac
    q = (e if e else 1) - 1075 + exponent                 # the value is +-mag 2^q
    if q >= 0:
        w = mag << q
    else:
        fl, rem, half = mag >> -q, mag & ((1 << -q) - 1), 1 << (-q - 1)
        w = fl + (1 if rem > half or (rem == half and fl & 1) else 0)
    return -w if neg else w


def quantize_model(x, exponent, e_words, offsets=None):
    """(words uint32 [K, M, e_words], signs uint8 [K, M], sums: Python ints per column — or per segment of `offsets`, x then [K])
    of a float64 / int64 array x [K, M] or [K]: what pai_fp_quantize must write"""
    x = np.asarray(x)
    flat = [quantize_one(v, exponent) for v in x.reshape(-1).tolist()] if x.dtype.kind == "f" else \
        [quantize_one(int(v), exponent) for v in x.reshape(-1)]
    w = np.array(flat, dtype=object).reshape(x.shape)
    words = np.zeros(x.shape + (e_words,), dtype=np.uint32)
    for pos, v in np.ndenumerate(w):
        for i in range(e_words):
            words[pos + (i,)] = (abs(v) >> (32 * i)) & 0xFFFFFFFF
    sign = (w < 0).astype(np.uint8)
    if offsets is None:
        sums = [int(sum(abs(v) for v in w[:, j])) for j in range(x.shape[1])]
    else:
        sums = [int(sum(abs(v) for v in w[offsets[s]:offsets[s + 1]])) for s in range(len(offsets) - 1)]
    return words, sign, sums


def test_quantiser_model_rounds_like_fractions_at_ties_subnormals_and_zeros():
    ulp = 2.0 ** -52
    cases = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.25, -0.75, 1.0 + ulp, 1.0 - ulp / 2, 3.0, -7.0, 1e-3, -123.456,
             5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 2.0 ** 52 + 0.5, 2.0 ** 53, -(2.0 ** 62)]
    # ties half an ulp and one and a half ulps above a representable integer grid point, at several exponents
    for E in (0, 1, 3, 10, 52, 60):
        for k in (1, 2, 3, 1 << 20 | 1):
            cases += [math.ldexp(2 * k + 1, -E - 1), -math.ldexp(2 * k + 1, -E - 1), math.ldexp(4 * k + 3, -E - 2)]
    for x in cases:
        for E in (-70, -3, -1, 0, 1, 3, 10, 52, 60, 64, 1074, 1100):
            want = round(Fraction(x) * Fraction(2) ** E)   # Python rounds fractions half to even
            assert quantize_one(x, E) == want, (x, E)
    assert quantize_one(0.5, 0) == 0 and quantize_one(1.5, 0) == 2 and quantize_one(2.5, 0) == 2 and quantize_one(-0.5, 0) == 0
    assert quantize_one(-1.5, 0) == -2 and quantize_one(5e-324, 1074) == 1 and quantize_one(5e-324, 1073) == 0
    assert quantize_one(1.5e-323, 1073) == 2              # 3 subnormal units at half a unit each: the tie goes to even


def test_quantiser_model_shifts_integers_exactly_and_lays_words_out():
    for x, E in itertools.product((0, 1, -1, 12345, -(1 << 62), (1 << 63) - 1, -(1 << 63)), (0, 1, 31, 62)):
        assert quantize_one(np.int64(x), E) == x * (1 << E)
    x = np.array([[3, -4], [0, (1 << 40) + 5], [-(1 << 63), 1]], dtype=np.int64)
    words, sign, sums = quantize_model(x, 1, 3)
    assert words.shape == (3, 2, 3) and sign.tolist() == [[0, 1], [0, 0], [1, 0]]
    assert words[1, 1].tolist() == [10, 1 << 9, 0] and words[2, 0].tolist() == [0, 0, 1] and words[0, 1].tolist() == [8, 0, 0]
    assert sums == [6 + (1 << 64), 8 + (1 << 41) + 10 + 2]
    words, sign, sums = quantize_model(np.array([0.5, 1.5, -2.5, 3.0]), 0, 1, offsets=[0, 0, 3, 4])
    assert words[:, 0].tolist() == [0, 2, 2, 3] and sign.tolist() == [0, 0, 1, 0] and sums == [0, 4, 3]


# ---- the headroom rule --------------------------------------------------------------------------------------------------------------
def test_weighted_sum_value_bits_bounds_the_extreme_sum_exhaustively():
    for v, S in itertools.product(range(1, 9), range(0, 300)):
        bound = packed.weighted_sum_value_bits(v, S, 128)
        assert bound == v + S.bit_length()
        top = ((1 << v) - 1) * S                           # every member at its extreme, every weight's sign aligned
        assert top < 1 << bound and -top > -(1 << bound), (v, S)
        if S:
            assert (1 << v) * S >= 1 << (bound - 1), (v, S)     # ... and not loose by more than one bit
    assert packed.weighted_sum_value_bits(20, 0, 32) == 20 and packed.weighted_sum_value_bits(20, 1, 32) == 21
    # every weighted sum of three members at v = 2 under every sign pattern of the weights (2, 3, 1): S = 6
    bound = packed.weighted_sum_value_bits(2, 6, 64)
    for ms in itertools.product(range(-3, 4), repeat=3):
        for ws in itertools.product((2, -2), (3, -3), (1, -1)):
            assert abs(sum(w * m for w, m in zip(ws, ms))) < 1 << bound


def test_weighted_sum_value_bits_overflow_edge():
    assert packed.weighted_sum_value_bits(20, (1 << 11) - 1, 32) == 31        # exactly the b - 1 bits a 32-bit slot holds
    with pytest.raises(OverflowError):
        packed.weighted_sum_value_bits(20, 1 << 11, 32)
    with pytest.raises(OverflowError):
        packed.weighted_sum_value_bits(31, 1, 32)
    assert packed.weighted_sum_value_bits(31, 0, 32) == 31
    assert packed.weighted_sum_value_bits(1, (1 << 126) - 1, 128) == 127
    with pytest.raises(OverflowError):
        packed.weighted_sum_value_bits(1, (1 << 128) - 1, 128)                # a saturated device sum always overflows


# ---- argument checks come before the device ------------------------------------------------------------------------------------------
def test_scale_rows_argument_checks():
    pk = host_key()
    p = host_packed(pk, 6, 64, 3)
    for c in (np.ones(6), torch.ones(6), np.ones(6, dtype=bool), torch.ones(6, dtype=torch.bool), [1.0] * 6, [True] * 6):
        with pytest.raises(TypeError):
            p.scale_rows(c)
    for c in (np.ones(5, dtype=np.int64), np.ones(7, dtype=np.int32), np.ones((6, 1), dtype=np.int64), torch.ones(3, dtype=torch.int64), []):
        with pytest.raises(ValueError):
            p.scale_rows(c)
    with pytest.raises(OverflowError):
        host_packed(pk, 2, 32, 3, v=20).scale_rows(np.array([1, 1 << 11]))    # 20 + 12 bits > 31
    with pytest.raises(ValueError):
        p.scale_rows(np.array([1 << 63] * 6, dtype=np.uint64))
    empty = host_packed(pk, 0, 64, 3).scale_rows(np.zeros(0, dtype=np.int64))
    assert empty.rows == 0 and empty.slots == 3
    assert no_device(pk)


def test_rmatmul_argument_checks():
    pk = host_key()
    p = host_packed(pk, 6, 64, 3)
    for W in (np.ones((2, 6), dtype=bool), np.ones((2, 6), dtype=complex), np.array([[None] * 6]), torch.ones((2, 6), dtype=torch.bool)):
        with pytest.raises(TypeError):
            p.rmatmul(W)
        with pytest.raises(TypeError):
            W @ p
    for W in (np.ones((2, 5)), np.ones(7, dtype=np.int64), np.ones((6, 2)), np.ones((1, 2, 6)), torch.ones((6, 5))):
        with pytest.raises(ValueError):
            p.rmatmul(W)
    for we in (1.0, np.float64(2), True, "3", None):
        with pytest.raises(TypeError):
            p.rmatmul(np.ones((2, 6)), weight_exponent=we)
        with pytest.raises(TypeError):
            p.csr_rmatmul([0, 1], [0], [1.0], (1, 6), weight_exponent=we)
    with pytest.raises(ValueError):
        p.rmatmul(np.ones((2, 6), dtype=np.int64), weight_exponent=-1)        # integers cannot be shifted right
    with pytest.raises(ValueError):
        p.rmatmul(np.full((2, 6), 1 << 63, dtype=np.uint64))
    assert no_device(pk)


def test_matmul_with_the_matrix_on_the_right_is_rejected():
    pk = host_key()
    p = host_packed(pk, 6, 64, 3)
    for W in (np.ones((6, 2)), np.ones(6), [[1] * 2] * 6, torch.ones((6, 2)), np.ones((18, 2))):
        with pytest.raises(TypeError, match="split rows"):
            p @ W
    assert no_device(pk)


def test_csr_rmatmul_argument_checks_are_those_of_csr_args():
    pk = host_key()
    p = host_packed(pk, 6, 64, 3)
    ptr, idx, dat = np.array([0, 2, 2, 3]), np.array([0, 5, 1]), np.array([1.0, -2.0, 3.0])
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr, idx, dat, (3, 5))               # 6 rows are no multiple of 5 columns
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr, idx, dat, (3, 3))               # ... and a divisor of 6 is not enough: one column per row
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr, idx, dat, (3, 2))
    with pytest.raises(NotImplementedError):
        p.csr_rmatmul(ptr, idx, dat, (3, 6, 1))
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr[:-1], idx, dat, (3, 6))          # indptr too short
    with pytest.raises(ValueError):
        p.csr_rmatmul(np.array([0, 2, 1, 3]), idx, dat, (3, 6))     # indptr steps back
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr, np.array([0, 6, 1]), dat, (3, 6))        # column out of range
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr, idx, dat[:-1], (3, 6))
    with pytest.raises(ValueError):
        p.csr_rmatmul(np.array([0]), idx[:0], dat[:0], (0, 6))      # no output rows
    with pytest.raises(TypeError):
        p.csr_rmatmul(ptr, idx, np.array([True, False, True]), (3, 6))
    with pytest.raises(TypeError):
        p.csr_rmatmul(ptr.astype(np.float64), idx, dat, (3, 6))
    with pytest.raises(ValueError):
        p.csr_rmatmul(ptr, idx, np.array([1, 2, 3]), (3, 6), weight_exponent=-2)
    assert no_device(pk)


def test_zero_row_container_gives_zero_rows_without_a_device():
    pk = host_key()
    p = host_packed(pk, 0, 100, 2, v=30)
    for W, we in ((np.zeros((4, 0)), 0), (np.zeros((4, 0), dtype=np.int64), 3), (np.zeros(0), 0), (torch.zeros((2, 0)), 5)):
        q = p.rmatmul(W, weight_exponent=we)
        assert isinstance(q, PaillierPackedNumber) and q.rows == 0 and len(q) == 0
        assert (q.slot_bits, q.slots, q.exponent, q.value_bits) == (100, 2, p.exponent + we, 30)
    assert (np.zeros((4, 0)) @ p).rows == 0
    with pytest.raises(ValueError):
        p.rmatmul(np.zeros((4, 1)))
    assert no_device(pk)


# ---- the entry point and the surface ----------------------------------------------------------------------------------------------
def test_pai_fp_quantize_is_declared_bound_and_exported():
    import re

    name = "pai_fp_quantize"
    assert name in _native.PROTOTYPES and len(_native.PROTOTYPES[name][1]) == 17
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m and re.search(r"long\s+long\s+stride_k\s*,\s*long\s+long\s+stride_m", m.group(1))
    assert len(m.group(1).split(",")) == 17
    assert hasattr(_native.load(), name)


def test_python_surface():
    from pailliercryptolib_python_amd import engine

    assert callable(getattr(engine.PublicKeyHandle, "fp_quantize", None))
    for meth in ("scale_rows", "rmatmul", "csr_rmatmul", "__rmatmul__"):
        assert callable(getattr(PaillierPackedNumber, meth, None)), meth
        assert "apply_obfuscator" in getattr(PaillierPackedNumber, meth).__doc__ or meth == "__rmatmul__"
    assert packed.PACKED_ROUTES.keys() == {"fast", "composite"}
    for meth in ("scale_rows", "rmatmul", "csr_rmatmul"):
        assert meth in packed.__doc__
