"""CPU: the plan behind PaillierEncryptedNumber.cumsum (paillier._scan_plan) and its argument checks (paillier._cumsum_args),
checked in the additive domain with Python ints — a ciphertext product acc^(2^s) * ct^(2^r) is acc 2^s + m 2^r on the plaintexts —
against the direct formula sum_j m_j 2^(E_i - e_j), and a model of pai_ct_scan's three-phase chunked evaluation (chunk totals, the
scan of the totals level by level, seeded chunks) against the unchunked chain."""
from pathlib import Path
import re

import numpy as np
import pytest

from pailliercryptolib_python_amd import _native
from pailliercryptolib_python_amd import paillier as P

ROOT = Path(__file__).resolve().parents[1]


def order(L, reverse):
    """run-local element offsets in scan order"""
    return list(range(L - 1, -1, -1)) if reverse else list(range(L))


def scan_chain(m, raise_, step, L, reverse):
    """The unchunked chains of pai_ct_scan: per run, acc_first = m 2^raise, acc_i = acc_prev 2^step_i + m_i 2^raise_i."""
    N = len(m)
    out = [None] * N
    for base in range(0, N, L):
        acc = None
        for p, o in enumerate(order(L, reverse)):
            i = base + o
            v = m[i] << int(raise_[i])
            acc = v if p == 0 else (acc << int(step[i])) + v
            out[i] = acc
    return out


def scan_chunked(m, raise_, step, L, reverse, C, level=0):
    """The dispatcher's levels.  Phase 1: the total of every chunk of C scan positions (unseeded, the first member's step not
    applied) and the sum of the chunk's steps (the first member's included unless it starts a run).  Phase 2: the inclusive scan of
    the totals per run with those sums as steps — this function again, forward, chunks of max(C, 2) — until a run is one chunk.
    Phase 3: every chunk again, seeded with the scanned total of the chunk before it."""
    N = len(m)
    c = C if level == 0 else max(C, 2)
    if c >= L:
        return scan_chain(m, raise_, step, L, reverse)
    cpr = -(-L // c)
    ords = order(L, reverse)
    totals, ssum = [], []
    for base in range(0, N, L):
        for k in range(cpr):
            acc, ss = None, 0
            for p in range(k * c, min(L, (k + 1) * c)):
                i = base + ords[p]
                s = int(step[i]) if p > 0 else 0
                ss += s
                v = m[i] << int(raise_[i])
                acc = v if acc is None else (acc << s) + v
            totals.append(acc)
            ssum.append(ss)
    carry = scan_chunked(totals, [0] * len(totals), ssum, cpr, False, C, level + 1)
    out = [None] * N
    for r, base in enumerate(range(0, N, L)):
        for k in range(cpr):
            acc = carry[r * cpr + k - 1] if k else None
            for p in range(k * c, min(L, (k + 1) * c)):
                i = base + ords[p]
                v = m[i] << int(raise_[i])
                acc = v if acc is None else (acc << (int(step[i]) if p > 0 else 0)) + v
                out[i] = acc
    return out


def expected(m, expo, L, reverse):
    N = len(m)
    vals, exps = [], []
    for i in range(N):
        a = i - i % L
        mem = range(i, a + L) if reverse else range(a, i + 1)
        E = max(int(expo[j]) for j in mem)
        vals.append(sum(m[j] << (E - int(expo[j])) for j in mem))
        exps.append(E)
    return vals, exps


def check(expo, L, seed=0):
    rng = np.random.default_rng(seed)
    expo = np.asarray(expo)
    N = len(expo)
    m = [int(v) for v in rng.integers(1, 1 << 40, N)]
    for reverse in (False, True):
        raise_, step, out_expo = P._scan_plan(expo, L, reverse)
        want, want_e = expected(m, expo, L, reverse)
        assert out_expo.dtype == np.int32 and out_expo.tolist() == want_e
        if raise_ is None:
            assert step is None and len(set(expo.tolist())) <= 1
            raise_ = step = np.zeros(N, np.int32)
        else:
            assert raise_.dtype == np.int32 and step.dtype == np.int32 and raise_.shape == (N,) and step.shape == (N,)
            assert (raise_ >= 0).all() and (step >= 0).all()
            assert not ((raise_ != 0) & (step != 0)).any()              # an element is raised, or steps the accumulator: never both
            first = np.arange(N) % L == (L - 1 if reverse else 0)
            assert not step[first].any()
            assert (raise_ == out_expo - expo).all()
        assert scan_chain(m, raise_, step, L, reverse) == want
        for C in (1, 2, 3, 5, L):
            assert scan_chunked(m, raise_, step, L, reverse, C) == want, (C, reverse)


@pytest.mark.parametrize("L", [1, 2, 7, 84])
def test_plan_random_exponents(L):
    rng = np.random.default_rng(L)
    check(rng.integers(-20, 20, 84), L, seed=L)


@pytest.mark.parametrize("L", [1, 2, 7, 42])
def test_plan_all_equal_exponents(L):
    raise_, step, out_expo = P._scan_plan(np.full(42, -7), L, False)
    assert raise_ is None and step is None and out_expo.tolist() == [-7] * 42
    check(np.full(42, -7), L, seed=1)


@pytest.mark.parametrize("L", [1, 2, 7, 56])
def test_plan_strictly_rising_and_falling_exponents(L):
    up = np.arange(56) - 30
    check(up, L, seed=2)
    check(up[::-1].copy(), L, seed=3)
    # rising along the scan: every element steps the accumulator and none is raised; falling: the reverse
    raise_, step, _ = P._scan_plan(up, 56, False)
    assert not raise_.any() and step.tolist() == [0] + [1] * 55
    raise_, step, _ = P._scan_plan(up, 56, True)
    assert not step.any() and raise_.tolist() == list(range(55, -1, -1))


def test_plan_exponent_spread_above_64():
    rng = np.random.default_rng(4)
    expo = rng.integers(0, 3, 60)
    expo[::7] = 150
    check(expo, 20, seed=4)


def test_model_accepts_raise_and_step_on_one_element():
    """the C ABI takes both counts non-zero on one element: the chunked evaluation equals the chain for arbitrary counts"""
    rng = np.random.default_rng(5)
    N, L = 90, 30
    m = [int(v) for v in rng.integers(1, 1 << 40, N)]
    raise_, step = rng.integers(0, 4, N), rng.integers(0, 4, N)
    for reverse in (False, True):
        want = scan_chain(m, raise_, step, L, reverse)
        for C in (1, 2, 3, 5, L):
            assert scan_chunked(m, raise_, step, L, reverse, C) == want


def test_plan_empty_input():
    raise_, step, out_expo = P._scan_plan(np.zeros(0, np.int32), 0, False)
    assert raise_ is None and step is None and out_expo.shape == (0,)


def test_argument_errors():
    assert P._cumsum_args(None, 12) == 12
    assert P._cumsum_args(None, 0) == 0
    assert P._cumsum_args(4, 12) == 4
    assert P._cumsum_args(np.int64(12), 12) == 12
    assert P._cumsum_args(3, 0) == 3
    for bad in (2.0, "4", True, np.bool_(True), [4]):
        with pytest.raises(TypeError):
            P._cumsum_args(bad, 12)
    for bad in (0, -4, 5, 24):
        with pytest.raises(ValueError):
            P._cumsum_args(bad, 12)


def test_scan_is_declared_bound_and_exported():
    assert "pai_ct_scan" in _native.PROTOTYPES
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    assert re.search(r"\bpai_ct_scan\s*\(", header)
    assert hasattr(_native.load(), "pai_ct_scan")
    from pailliercryptolib_python_amd import engine

    assert callable(getattr(engine.PublicKeyHandle, "ct_scan", None))
    assert callable(getattr(P.PaillierEncryptedNumber, "cumsum", None))
