"""CPU: the plan behind PaillierEncryptedNumber.segment_sum (paillier._segment_plan), checked in the additive domain with Python
ints — a ciphertext product ct^(2^k) * ct' is the sum m 2^k + m' of its plaintexts — against the direct formula, and the chunked
evaluation of pai_ct_segment_prod (partials per chunk, combined with their summed shifts) against the unchunked chain."""
from pathlib import Path
import re

import numpy as np
import pytest
import torch

from pailliercryptolib_python_amd import _native
from pailliercryptolib_python_amd import paillier as P

ROOT = Path(__file__).resolve().parents[1]


def chain(rows, shift, m, lo, hi):
    """The Horner chain acc <- acc * 2^shift_j + m[row_j] over members lo .. hi-1 (the first member's shift ignored), and the
    sum of the members' shifts (the exponent step the partial carries)."""
    acc, ssum = 0, 0
    for j in range(lo, hi):
        s = int(shift[j])
        ssum += s
        acc = (acc << s if j > lo else 0) + m[int(rows[j])]
    return acc, ssum


def chunked(rows, shift, offsets, m, C):
    """The dispatcher's levels: cut every segment into chunks of <= C members, one chain per chunk, then the partials of a
    segment form its next member list (row = chunk index, shift = the chunk's summed shifts), until one chain per segment."""
    S = len(offsets) - 1
    vals = list(m)
    rows, shift, offsets = list(rows), list(shift), list(offsets)
    c = C
    while max((offsets[s + 1] - offsets[s] for s in range(S)), default=0) > c:
        parts, psh, poff = [], [], [0]
        for s in range(S):
            for a in range(offsets[s], offsets[s + 1], c):
                v, ss = chain(rows, shift, vals, a, min(a + c, offsets[s + 1]))
                parts.append(v)
                psh.append(ss)
            poff.append(len(parts))
        vals, rows, shift, offsets = parts, list(range(len(parts))), psh, poff
        c = max(2, min(C, 4))
    return [chain(rows, shift, vals, offsets[s], offsets[s + 1])[0] for s in range(S)]


def expected(ids, expo, m, K):
    """Direct formula: segment f K + b sums m_i 2^(E - e_i) over rows with ids[i, f] == b; E = max member exponent (empty:
    the smallest exponent of the input, 0 without input)."""
    ids = np.asarray(ids).reshape(len(expo), -1)
    N, F = ids.shape
    emin = int(min(expo)) if N else 0
    vals, exps = [], []
    for f in range(F):
        for b in range(K):
            mem = [i for i in range(N) if ids[i, f] == b]
            if not mem:
                vals.append(0)
                exps.append(emin)
                continue
            E = max(int(expo[i]) for i in mem)
            vals.append(sum(m[i] << (E - int(expo[i])) for i in mem))
            exps.append(E)
    return vals, exps


def check(ids, expo, K, seed=0):
    rng = np.random.default_rng(seed)
    N = len(expo)
    m = [int(v) for v in rng.integers(1, 1 << 40, N)]
    t = torch.from_numpy(np.asarray(ids, dtype=np.int64).reshape(N, -1))
    rows, shift, offsets, seg_expo = P._segment_plan(t, np.asarray(expo), K)
    assert rows.dtype == torch.int32 and shift.dtype == torch.int32 and offsets.dtype == torch.int64
    off = offsets.tolist()
    S = t.shape[1] * K
    assert len(off) == S + 1 and off[0] == 0 and all(a <= b for a, b in zip(off, off[1:]))
    assert off[S] == int((t >= 0).sum())
    r, sh = rows.tolist(), shift.tolist()
    assert all(0 <= x < N for x in r[:off[S]]) and all(x >= 0 for x in sh[:off[S]])
    want, want_e = expected(ids, expo, m, K)
    got = [chain(r, sh, m, off[s], off[s + 1])[0] for s in range(S)]
    assert got == want
    assert seg_expo.tolist() == want_e
    # squarings of a segment's chain = its exponent spread (Horner order), not the sum of the members' raises
    for s in range(S):
        if off[s + 1] > off[s]:
            es = [int(expo[r[j]]) for j in range(off[s], off[s + 1])]
            assert sum(sh[off[s] + 1:off[s + 1]]) == max(es) - min(es)
            assert sh[off[s]] == 0
    for C in range(1, 6):
        assert chunked(r, sh, off, m, C) == want, C


def test_plan_random_ids_and_exponents():
    rng = np.random.default_rng(1)
    N, K = 300, 7
    check(rng.integers(0, K, N), rng.integers(-20, 20, N), K, seed=1)


def test_plan_two_dimensional_ids_with_negatives_and_empty_segments():
    rng = np.random.default_rng(2)
    N, F, K = 200, 3, 9
    ids = rng.integers(-2, K - 3, (N, F))           # ids K-3 .. K-1 never occur: empty segments; negatives drop pairs
    check(ids, rng.integers(0, 12, N), K, seed=2)


def test_plan_all_equal_exponents():
    rng = np.random.default_rng(3)
    N, K = 150, 4
    ids = rng.integers(0, K, N)
    t = torch.from_numpy(ids.astype(np.int64)).reshape(N, 1)
    _, shift, offsets, _ = P._segment_plan(t, np.full(N, 5), K)
    assert not shift[:int(offsets[-1])].any()
    check(ids, np.full(N, 5), K, seed=3)


def test_plan_exponent_spread_above_64():
    rng = np.random.default_rng(4)
    N, K = 60, 3
    expo = rng.integers(0, 3, N)
    expo[::7] = 150                                 # spreads of 150 inside a segment
    check(rng.integers(0, K, N), expo, K, seed=4)


def test_plan_one_segment_holding_most_rows():
    rng = np.random.default_rng(5)
    N, K = 400, 5
    ids = np.where(rng.random(N) < 0.9, 2, rng.integers(0, K, N))
    check(ids, rng.integers(40, 60, N), K, seed=5)


def test_plan_empty_input():
    rows, shift, offsets, seg_expo = P._segment_plan(torch.zeros((0, 2), dtype=torch.int64), np.zeros(0, np.int32), 3)
    assert offsets.tolist() == [0] * 7 and seg_expo.tolist() == [0] * 6
    assert rows.numel() == 0 and shift.numel() == 0


def test_plan_only_dropped_pairs():
    check(np.full(10, -1), np.arange(10), 2)


def test_argument_errors():
    ok = np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError):
        P._segment_ids(ok, 4, 0)
    with pytest.raises(ValueError):
        P._segment_ids(ok, 4, -3)
    with pytest.raises(TypeError):
        P._segment_ids(ok, 4, 2.0)
    with pytest.raises(TypeError):
        P._segment_ids(ok.astype(np.float64), 4, 2)
    with pytest.raises(TypeError):
        P._segment_ids(torch.zeros(4), 4, 2)
    with pytest.raises(TypeError):
        P._segment_ids(torch.zeros(4, dtype=torch.bool), 4, 2)
    with pytest.raises(TypeError):
        P._segment_ids([0, 1, 0, 1], 4, 2)
    with pytest.raises(ValueError):
        P._segment_ids(np.zeros(5, dtype=np.int64), 4, 2)         # wrong length
    with pytest.raises(ValueError):
        P._segment_ids(np.zeros((4, 2, 2), dtype=np.int64), 4, 2)  # wrong rank
    with pytest.raises(ValueError):
        P._segment_ids(np.array([0, 1, 2, 0]), 4, 2)              # id >= num_segments
    big = np.array([0, 1, 1 << 63, 0], dtype=np.uint64)           # ids >= 2^63: the same error for numpy and torch ids
    with pytest.raises(ValueError):
        P._segment_ids(big, 4, 2)
    if hasattr(torch, "uint64"):
        with pytest.raises(ValueError):
            P._segment_ids(torch.from_numpy(big.view(np.int64)).view(torch.uint64), 4, 2)
        ok_u = P._segment_ids(torch.tensor([0, 1, 1, 0], dtype=torch.int64).view(torch.uint64), 4, 2)
        assert ok_u.dtype == torch.int64 and ok_u.reshape(-1).tolist() == [0, 1, 1, 0]
    ids = P._segment_ids(torch.tensor([0, -1, 1, 1], dtype=torch.int32), 4, 2)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (4, 1)
    assert tuple(P._segment_ids(np.zeros((4, 3), dtype=np.uint8), 4, 1).shape) == (4, 3)
    assert tuple(P._segment_ids(np.zeros((0, 2), dtype=np.int64), 0, 3).shape) == (0, 2)
    assert tuple(P._segment_ids(np.zeros(0, dtype=np.int64), 0, 3).shape) == (0, 1)


def test_segment_prod_is_declared_bound_and_exported():
    assert "pai_ct_segment_prod" in _native.PROTOTYPES
    header = (ROOT / "include" / "paillier_hip.h").read_text()
    assert re.search(r"\bpai_ct_segment_prod\s*\(", header)
    assert hasattr(_native.load(), "pai_ct_segment_prod")
    from pailliercryptolib_python_amd import engine

    assert callable(getattr(engine.PublicKeyHandle, "ct_segment_prod", None))
    assert callable(getattr(P.PaillierEncryptedNumber, "segment_sum", None))
