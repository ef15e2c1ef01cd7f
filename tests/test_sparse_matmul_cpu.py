"""CPU: the plan behind PaillierEncryptedNumber.csr_rmatmul / csr_matmul (paillier._sparse_terms / _sparse_plan), checked in the
additive domain with Python ints — the product of the terms' powers ct_b^(w) is the sum of w * m_b over its terms — against the
direct formula of the sparse product; the argument checks of paillier._csr_args; and the C ABI symbol."""
from pathlib import Path
import ctypes as C
import re

import numpy as np
import pytest
import torch

from pailliercryptolib_python_amd import _native
from pailliercryptolib_python_amd import paillier as P

ROOT = Path(__file__).resolve().parents[1]


def direct(indptr, indices, data, shape, expo, rhs, length, mvals):
    """Output element s = i k + j: sum over its terms of mant(v) m_b 2^(E_s - e_b - p_v) and E_s = max(e_b + p_v) (an element
    without terms: 0 at the smallest term exponent, 0 without terms), written out with Python loops over the stored entries."""
    mant, pexpo = P._sparse_weights(np.asarray(data))
    if rhs:
        m, n = shape
        k = length // n
    else:
        n, k = shape
        m = length // n
    terms = {s: [] for s in range(m * k)}
    for r in range(len(indptr) - 1):
        for p in range(indptr[r], indptr[r + 1]):
            c = int(indices[p])
            if rhs:                                   # A[r, c]: output (r, j) takes base c k + j
                for j in range(k):
                    terms[r * k + j].append((c * k + j, p))
            else:                                     # B[r, c]: output (i, c) takes base i n + r
                for i in range(m):
                    terms[i * k + c].append((i * n + r, p))
    tot = [int(expo[b]) + int(pexpo[p]) for s in terms for b, p in terms[s]]
    lo = min(tot) if tot else 0
    vals, exps = [], []
    for s in range(m * k):
        if not terms[s]:
            vals.append(0)
            exps.append(lo)
            continue
        E = max(int(expo[b]) + int(pexpo[p]) for b, p in terms[s])
        vals.append(sum(int(mant[p]) * mvals[b] << (E - int(expo[b]) - int(pexpo[p])) for b, p in terms[s]))
        exps.append(E)
    return vals, exps


def check(indptr, indices, data, shape, expo, rhs, want_ew=None, seed=0):
    rng = np.random.default_rng(seed)
    length = len(expo)
    mvals = [int(v) for v in rng.integers(1, 1 << 40, length)]
    ptr, idx, d, (m, n, k) = P._csr_args(np.asarray(indptr), np.asarray(indices), np.asarray(data), shape, length, rhs)
    base, widx, seg, offsets = P._sparse_terms(ptr, idx, m, n, k, rhs)
    mant, pexpo = P._sparse_weights(d)
    e, ebits, sign, seg_expo = P._sparse_plan(base, widx, seg, torch.from_numpy(mant), torch.from_numpy(pexpo),
                                              torch.from_numpy(np.asarray(expo, dtype=np.int64)), m * k)
    assert e is not None and e.dtype == torch.int32 and sign.dtype == torch.uint8
    if want_ew is not None:
        assert e.shape[1] == want_ew, (e.shape, ebits)
    assert 32 * (e.shape[1] - 1) < ebits <= 32 * e.shape[1]
    off = offsets.tolist()
    T = base.shape[0]
    assert off[0] == 0 and off[-1] == T and all(a <= b for a, b in zip(off, off[1:]))
    assert all(0 <= b < length for b in base.tolist())
    assert seg.tolist() == [s for s in range(m * k) for _ in range(off[s], off[s + 1])]
    words = e.numpy().view(np.uint32)
    sg = sign.tolist()
    bl = base.tolist()
    got = []
    for s in range(m * k):
        acc = 0
        for t in range(off[s], off[s + 1]):
            w = int.from_bytes(words[t].tobytes(), "little")
            assert w.bit_length() <= ebits
            acc += (-1 if sg[t] else 1) * w * mvals[bl[t]]
        got.append(acc)
    want, want_e = direct(indptr, indices, data, shape, expo, rhs, length, mvals)
    assert got == want
    assert seg_expo.tolist() == want_e
    return e.shape[1]


def random_csr(rng, rows, cols, density, data_fn, empty_rows=(), dup=False, zeros=False):
    indptr, indices, data = [0], [], []
    for r in range(rows):
        if r not in empty_rows:
            c = sorted(rng.choice(cols, size=max(1, int(rng.binomial(cols, density))), replace=dup).tolist())
            indices += c
        indptr.append(len(indices))
    data = data_fn(len(indices))
    if zeros and len(data):
        data[::4] = 0
    return np.asarray(indptr), np.asarray(indices, dtype=np.int64), data


@pytest.mark.parametrize("rhs", [True, False])
@pytest.mark.parametrize("k", [1, 3])
def test_plan_float_weights_both_signs_with_zeros_and_empty_rows(rhs, k):
    rng = np.random.default_rng(11 + k + 7 * rhs)
    rows, cols = (5, 9) if rhs else (9, k)
    indptr, indices, data = random_csr(rng, rows, cols, 0.4, lambda c: rng.standard_normal(c), empty_rows=(1,), zeros=True)
    length = cols * k if rhs else 4 * rows
    expo = np.full(length, 10)
    check(indptr, indices, data, (rows, cols), expo, rhs, want_ew=2, seed=k)


@pytest.mark.parametrize("rhs", [True, False])
def test_plan_empty_columns_duplicates_and_explicit_zeros(rhs):
    # column 2 never stored (an empty output column for self @ B), duplicates in row 0, explicit zeros
    indptr = [0, 4, 4, 6, 8]
    indices = [0, 0, 3, 3, 1, 4, 0, 4]
    data = np.array([1.5, -2.0, 0.0, 3.25, -0.0, 7.0, 0.0, -1e-3])
    expo = np.arange(20) % 5 if rhs else np.arange(12) % 3
    shape = (4, 5) if rhs else (4, 5)
    length = 5 * 4 if rhs else 3 * 4
    check(indptr, indices, data, shape, expo[:length], rhs, seed=3)


@pytest.mark.parametrize("rhs", [True, False])
def test_plan_integer_weights_one_word(rhs):
    rng = np.random.default_rng(5)
    indptr, indices, data = random_csr(rng, 6, 7, 0.5, lambda c: rng.integers(-3, 4, c).astype(np.int8), empty_rows=(2,))
    length = 7 * 2 if rhs else 6 * 3
    assert check(indptr, indices, data, (6, 7), np.zeros(length, np.int64), rhs) == 1


def test_plan_int64_extremes():
    # int64 -2^63 encodes as 0 (exponent 0); 2^63 - 1 and -(2^63 - 1) keep all 63 bits; uint64 below 2^63 are plain values
    indptr = [0, 3, 5]
    indices = [0, 1, 2, 0, 2]
    data = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -np.iinfo(np.int64).max, -5, 1 << 40], dtype=np.int64)
    mant, pexpo = P._sparse_weights(data)
    assert mant[0] == 0 and pexpo.tolist() == [0] * 5
    check(indptr, indices, data, (2, 3), np.array([0, 3, 1]), True)
    check(indptr, indices, data.astype(np.uint64) % (1 << 62), (2, 3), np.array([0, 3, 1]), True)
    check(indptr, indices, data, (2, 3), np.array([4, 0, 2, 1, 1, 7]), False)


@pytest.mark.parametrize("spread,ew", [(0, 1), (20, 2), (50, 3), (80, 4)])
def test_plan_mixed_exponents_word_counts(spread, ew):
    # 20-bit weights; row 0 holds columns 0 and 1, whose bases (j = 0) sit at exponents 0 and `spread`: 20 + spread aligned bits
    rng = np.random.default_rng(spread)
    indptr, indices, data = random_csr(rng, 4, 12, 0.5, lambda c: ((1 << 19) + rng.integers(0, 1 << 19, c)) * rng.choice([-1, 1], c))
    indptr = np.concatenate([[0], indptr + 3])
    indices = np.concatenate([[0, 1, 5], indices])
    data = np.concatenate([[1 << 19, -(1 << 19) - 7, 3], data])
    expo = rng.integers(0, spread + 1, 12 * 2)
    expo[0], expo[2] = 0, spread
    assert check(indptr, indices, data, (5, 12), expo, True, seed=spread) == ew
    expo_b = rng.integers(0, spread + 1, 3 * 5)
    expo_b[0], expo_b[1] = 0, spread                                    # self @ B: row 0 of self, B rows 0 and 1 (column 0 and 1)
    check(indptr, indices, data, (5, 12), expo_b, False, seed=spread)


def test_plan_spread_above_cap_is_refused():
    # 1e-30 and 1e30 in one row: 252 aligned bits — the fast route declines (the composite route serves)
    ptr, idx, d, (m, n, k) = P._csr_args(np.array([0, 2]), np.array([0, 1]), np.array([1e-30, 1e30]), (1, 2), 2, True)
    base, widx, seg, offsets = P._sparse_terms(ptr, idx, m, n, k, True)
    mant, pexpo = P._sparse_weights(d)
    e, ebits, _, _ = P._sparse_plan(base, widx, seg, torch.from_numpy(mant), torch.from_numpy(pexpo), torch.zeros(2, dtype=torch.int64), 1)
    assert e is None and ebits == 252


def test_plan_no_terms():
    ptr, idx, d, (m, n, k) = P._csr_args(np.zeros(4, np.int64), np.zeros(0, np.int64), np.zeros(0), (3, 2), 4, True)
    base, widx, seg, offsets = P._sparse_terms(ptr, idx, m, n, k, True)
    e, ebits, sign, seg_expo = P._sparse_plan(base, widx, seg, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                                              torch.arange(4, dtype=torch.int64), m * k)
    assert base.numel() == 0 and offsets.tolist() == [0] * 7 and seg_expo.tolist() == [0] * 6


def test_argument_errors():
    ip, ix, d = np.array([0, 1, 2]), np.array([0, 1]), np.array([1.0, 2.0])
    P._csr_args(ip, ix, d, (2, 2), 4, True)
    P._csr_args(torch.from_numpy(ip), torch.from_numpy(ix), torch.from_numpy(d), (2, 2), 4, False)
    with pytest.raises(ValueError, match="matrix multiplysize mismatch"):
        P._csr_args(ip, ix, d, (2, 3), 4, True)                  # n = 3 does not divide len(self)
    with pytest.raises(ValueError, match="matrix multiply size mismatch"):
        P._csr_args(ip, ix, d, (3, 2), 4, False)
    with pytest.raises(ValueError):
        P._csr_args(np.array([0, 2, 1]), ix, d, (2, 2), 4, True)   # not monotone
    with pytest.raises(ValueError):
        P._csr_args(np.array([0, 1, 1]), ix, d, (2, 2), 4, True)   # does not end at len(indices)
    with pytest.raises(ValueError):
        P._csr_args(np.array([1, 1, 2]), ix, d, (2, 2), 4, True)   # does not start at 0
    with pytest.raises(ValueError):
        P._csr_args(np.array([0, 2]), ix, d, (2, 2), 4, True)      # wrong length
    with pytest.raises(ValueError):
        P._csr_args(ip, np.array([0, 2]), d, (2, 2), 4, True)      # index out of range
    with pytest.raises(ValueError):
        P._csr_args(ip, np.array([0, -1]), d, (2, 2), 4, False)
    with pytest.raises(ValueError):
        P._csr_args(ip, ix, np.array([1.0]), (2, 2), 4, True)      # data / indices lengths
    with pytest.raises(NotImplementedError):
        P._csr_args(ip, ix, d, (2,), 4, True)
    with pytest.raises(NotImplementedError):
        P._csr_args(ip, ix, d, (2, 2, 1), 4, False)
    with pytest.raises(ValueError):
        P._csr_args(np.array([0]), np.zeros(0, np.int64), np.zeros(0), (0, 2), 4, True)       # m = 0
    with pytest.raises(ValueError):
        P._csr_args(np.array([0, 0, 0]), np.zeros(0, np.int64), np.zeros(0), (2, 0), 4, False)  # k = 0
    with pytest.raises(ValueError):
        P._csr_args(ip, ix, d, (2, 2), 0, True)                    # k = len(self) / n = 0
    for bad in (np.array([True, False]), np.array([1 + 2j, 3j]), np.array([1.0, "x"], dtype=object)):
        with pytest.raises(TypeError):
            P._csr_args(ip, ix, bad, (2, 2), 4, True)
    for bad in (torch.tensor([True, False]), torch.tensor([1 + 2j, 3j])):
        with pytest.raises(TypeError):
            P._csr_args(ip, ix, bad, (2, 2), 4, True)
    for bad in (np.array([np.nan, 1.0]), np.array([np.inf, 1.0])):
        ptr, idx, dd, _ = P._csr_args(ip, ix, bad, (2, 2), 4, True)      # the weight errors of ct * data, before any launch
        with pytest.raises((ValueError, OverflowError)):
            P._sparse_weights(dd)


def test_sparse_multiexp_is_declared_bound_and_rejects_null_key():
    assert "pai_ct_sparse_multiexp" in _native.PROTOTYPES
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    assert re.search(r"\bpai_ct_sparse_multiexp\s*\(", header)
    assert "bit 3" in header
    lib = _native.load()
    assert hasattr(lib, "pai_ct_sparse_multiexp")
    off = (C.c_int64 * 2)(0, 0)
    out = (C.c_uint32 * 64)()
    rc = lib.pai_ct_sparse_multiexp(None, None, None, 0, None, None, 1, 1, None, 0, C.cast(off, C.c_void_p), 1,
                                    C.cast(out, C.c_void_p), None)
    assert rc == _native.PAI_E_INVALID
    from pailliercryptolib_python_amd import engine

    assert callable(getattr(engine.PublicKeyHandle, "ct_sparse_multiexp", None))
    for name in ("csr_rmatmul", "csr_matmul", "__array__"):
        assert callable(getattr(P.PaillierEncryptedNumber, name, None))
