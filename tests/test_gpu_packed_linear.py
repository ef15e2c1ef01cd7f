"""GPU: linear maps of packed rows — pai_fp_quantize through the engine, PaillierPackedNumber.scale_rows / rmatmul / csr_rmatmul,
every check exact.

The expectations are CPython integers only: the ciphertext bits of output row f are prod_i pow(ct_i, w_fi, n^2) of the input's
getTexts() (Python's pow takes negative exponents modulo n^2), the mantissas object-dtype numpy sums, the quantised weights the
pure-Python model of tests/test_packed_linear_cpu.py — never the code under test.  Both routes are forced with
PAI_MEXP_MIN_TERMS, the chunking of the multi-exponentiation with PAI_TUNE, and the kernels that ran are read from
pai_profile_last after every engine call."""
import json
from pathlib import Path
import pickle

import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, _native, engine, packed
from pailliercryptolib_python_amd.bindings import ipclPublicKey

from ._util import tune
from .test_packed_linear_cpu import quantize_model, quantize_one

pytestmark = pytest.mark.gpu

_KEYS = {}


def keypair(bits):
    if bits not in _KEYS:
        fx = json.loads((Path(__file__).parent / "golden" / "fixture_keys.json").read_text())[str(bits)]
        key = orc.make_key(int(fx["p"], 16), int(fx["q"], 16), djn_x=(1 << 70) + 12345, bits=bits)
        pk = PaillierPublicKey(ipclPublicKey(key.n, bits, True, hs=key.hs, randbits=key.randbits))
        _KEYS[bits] = (key, pk, PaillierPrivateKey(pk, key.p, key.q))
    return _KEYS[bits]


def texts(p):
    return [int(c) for c in p.ciphertext().getTexts()]


def packed_ints(pk, rng, G, b, k, v, extremes=False):
    """(container of G full rows of integers |x| < 2^v at exponent 0 — raw encryptions, the chains do not care; its mantissas as
    an int64 [G, k] matrix); extremes: only the mantissas +-(2^v - 1)"""
    m = rng.integers(-(1 << v) + 1, 1 << v, (G, k))
    if extremes:
        m = np.where(rng.random((G, k)) < 0.5, (1 << v) - 1, -(1 << v) + 1)
    p = pk.encrypt_packed(m.reshape(-1).astype(np.int64), exponent=0, value_bits=v, slot_bits=b, slots=k, apply_obfuscator=False)
    return p, m.astype(np.int64)


def mant(sk, p, k):
    return np.array(sk.decrypt_packed_mantissas(p), dtype=object).reshape(-1, k)


def want_rows(ct, W, nsq):
    """prod_i pow(ct_i, w_fi, n^2) per row f of the integer matrix W (zero weights skipped: pow(c, 0) = 1)"""
    out = []
    for row in W:
        acc = 1
        for c, w in zip(ct, row):
            if int(w):
                acc = acc * pow(c, int(w), nsq) % nsq
        out.append(acc)
    return out


def sums_of(t):
    a = t.cpu().numpy().view(np.uint64)
    return [(int(hi) << 64) + int(lo) for lo, hi in a]


@pytest.fixture
def kernels(monkeypatch):
    """the kernel names of every engine call made while the fixture lives, in order (pai_profile_last after each call)"""
    seen = []

    def spy(name):
        fn = getattr(engine.PublicKeyHandle, name)

        def wrapped(self, *a, **kw):
            try:
                return fn(self, *a, **kw)
            finally:
                seen.append((name, sorted(engine.profile_last())))
        monkeypatch.setattr(engine.PublicKeyHandle, name, wrapped)

    for name in ("fp_quantize", "ct_invert", "ct_multiexp", "ct_sparse_multiexp", "ct_mul", "ct_segment_prod"):
        spy(name)
    engine.profile_enable(True)
    yield seen
    engine.profile_enable(False)


# ---- pai_fp_quantize ----------------------------------------------------------------------------------------------------------------
def quant_weights(rng, K, M, wb, E, is_f64):
    """[K, M] weights whose quantised values include 0, +-1, +-(2^wb - 1), ties (floats) and an all-zero column"""
    w = rng.integers(-(1 << wb) + 1, 1 << wb, (K, M)).astype(np.int64)
    w[0, 0], w[1, 0], w[2, 0], w[5, 0], w[6, 0] = (1 << wb) - 1, -(1 << wb) + 1, 0, 1, -1
    if M > 2:
        w[:, 2] = 0
    if not is_f64:
        return w                                           # exponent 0 for integers: every value is its own weight
    x = np.ldexp(w.astype(np.float64), -E)                 # exact: wb <= 53
    half = 2.0 ** -(E + 1)
    for i, base in enumerate((5, 6, -5, -6, 0, -1)):       # ties half way between grid points, either parity, both signs
        x[10 + i, 1 % M] = np.ldexp(float(base), -E) + half
    x[16, 1 % M] = -0.0
    return x


@pytest.mark.parametrize("is_f64", [True, False])
@pytest.mark.parametrize("ew", [1, 2])
def test_quantize_words_signs_and_sums_equal_the_model(is_f64, ew):
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(10 * ew + is_f64)
    wb, E = (20, 3) if ew == 1 else (40, 3)
    if not is_f64:
        E = 0
    for K, M in ((67, 5), (70, 130)):                      # 8 columns per workgroup and two row blocks; 64 columns and three column blocks
        x = quant_weights(rng, K, M, wb, E, is_f64)
        words, sign, sums = quantize_model(x, E, ew)
        assert max(sums) >= (1 << wb) - 1 and sums[2] == 0                          # the all-zero column
        c_order = torch.from_numpy(x).to(h.device)                                  # [K][M], the unit stride along the columns
        t_view = torch.from_numpy(np.ascontiguousarray(x.T)).to(h.device).t()       # the transposed view of an [M][K] array
        assert c_order.stride() == (M, 1) and t_view.stride() == (1, K)
        for xt in (c_order, t_view):
            e, s, tot, flag = h.fp_quantize(xt, E, wb, ew)
            assert int(flag.item()) == 0
            assert (e.cpu().numpy().view(np.uint32) == words).all(), (K, M, xt.stride())
            assert (s.cpu().numpy() == sign).all()
            assert sums_of(tot) == sums
    # segments: the first column as a term list, S = 4 with an empty segment; then a list that spans workgroups
    for K, offsets in ((67, [0, 10, 10, 40, 67]), (600, [0, 1, 300, 300, 600])):
        x = quant_weights(rng, K, 1, wb, E, is_f64)[:, 0].copy()
        words, sign, sums = quantize_model(x, E, ew, offsets=offsets)
        e, s, tot, flag = h.fp_quantize(torch.from_numpy(x).to(h.device), E, wb, ew, torch.tensor(offsets, device=h.device))
        assert int(flag.item()) == 0 and tuple(tot.shape) == (4, 2)
        assert (e.cpu().numpy().view(np.uint32) == words).all() and (s.cpu().numpy() == sign).all()
        assert sums_of(tot) == sums and sums[1 if K == 67 else 2] == 0


@pytest.mark.parametrize("is_f64", [True, False])
def test_quantize_one_workgroup_walks_many_tiles(is_f64, monkeypatch):
    """PAI_TUNE quantize_blocks=1: a single workgroup per column block takes every row tile in turn — ten tiles of 64 rows (the
    LDS tile is loaded, read and reused; the column sums are carried in registers from tile to tile) and three passes of 256
    rows in segment mode, with segments that cross the passes"""
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(77 + is_f64)
    tune(monkeypatch, "quantize_blocks", 1)
    wb, E, ew = 40, (3 if is_f64 else 0), 2
    for K, M in ((600, 5), (300, 130)):
        x = quant_weights(rng, K, M, wb, E, is_f64)
        words, sign, sums = quantize_model(x, E, ew)
        for xt in (torch.from_numpy(x).to(h.device), torch.from_numpy(np.ascontiguousarray(x.T)).to(h.device).t()):
            e, s, tot, flag = h.fp_quantize(xt, E, wb, ew)
            assert int(flag.item()) == 0
            assert (e.cpu().numpy().view(np.uint32) == words).all(), (K, M, xt.stride())
            assert (s.cpu().numpy() == sign).all() and sums_of(tot) == sums
    offsets = [0, 100, 100, 520, 600]
    x = quant_weights(rng, 600, 1, wb, E, is_f64)[:, 0].copy()
    words, sign, sums = quantize_model(x, E, ew, offsets=offsets)
    e, s, tot, flag = h.fp_quantize(torch.from_numpy(x).to(h.device), E, wb, ew, torch.tensor(offsets, device=h.device))
    assert int(flag.item()) == 0 and (e.cpu().numpy().view(np.uint32) == words).all() and (s.cpu().numpy() == sign).all()
    assert sums_of(tot) == sums
    # no segments at all: the operands are still written
    e, s, tot, flag = h.fp_quantize(torch.from_numpy(x).to(h.device), E, wb, ew, torch.tensor([0], device=h.device))
    assert tuple(tot.shape) == (0, 2) and (e.cpu().numpy().view(np.uint32) == words).all() and (s.cpu().numpy() == sign).all()


def test_quantize_shifts_integers():
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    x = np.random.default_rng(3).integers(-(1 << 30), 1 << 30, (67, 5))
    words, sign, sums = quantize_model(x, 5, 2)
    e, s, tot, flag = h.fp_quantize(torch.from_numpy(x).to(h.device), 5, 36, 2)
    assert int(flag.item()) == 0 and (e.cpu().numpy().view(np.uint32) == words).all() and (s.cpu().numpy() == sign).all()
    assert sums_of(tot) == sums


def test_quantize_flags_and_wide_sums():
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    x = np.zeros((67, 5))
    x[40, 3] = float(1 << 20)
    assert int(h.fp_quantize(torch.from_numpy(x).to(h.device), 0, 20, 1)[3].item()) == 1        # one |w| = 2^weight_bits
    assert int(h.fp_quantize(torch.from_numpy(x).to(h.device), 0, 21, 1)[3].item()) == 0
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[66, 4] = bad
        assert int(h.fp_quantize(torch.from_numpy(y).to(h.device), 0, 21, 1)[3].item()) == 2
    # 67 weights of 2^62: the sum needs the high word
    big = np.full((67, 1), 1 << 62, dtype=np.int64)
    e, s, tot, flag = h.fp_quantize(torch.from_numpy(big).to(h.device), 0, 63, 2)
    assert int(flag.item()) == 0 and sums_of(tot) == [67 << 62] and 67 << 62 >= 1 << 64
    tot = h.fp_quantize(torch.from_numpy(big[:, 0].copy()).to(h.device), 0, 63, 2, torch.tensor([0, 67], device=h.device))[2]
    assert sums_of(tot) == [67 << 62]


def test_quantize_rejects_invalid_widths():
    _, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    x = torch.zeros((67, 5), dtype=torch.float64, device=h.device)
    for wb, ew in ((0, 1), (33, 1), (65, 2), (127, 4), (8, 0), (8, 5), (-1, 2)):
        with pytest.raises(_native.NativeError) as exc:
            h.fp_quantize(x, 0, wb, ew)
        assert exc.value.code == _native.PAI_E_INVALID
    h.fp_quantize(x, 0, 126, 4)


# ---- scale_rows -----------------------------------------------------------------------------------------------------------------------
def test_scale_rows_raises_every_row_to_its_multiplier():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(21)
    G, b, k, v = 9, 64, 3, 20
    p, m = packed_ints(pk, rng, G, b, k, v)
    c = np.array([0, 1, -1, (1 << 29) + 123, -(1 << 29) - 77, 5, -7, 3, 1000], dtype=np.int64)
    ct = texts(p)
    for arg in (c, torch.from_numpy(c), c.tolist()):
        out = p.scale_rows(arg)
        assert len(out.ciphertext()._taint) == 1           # the inversion's outcome word travels with the result
        assert (out.rows, len(out), out.slot_bits, out.slots, out.exponent) == (G, G * k, b, k, 0)
        assert out.value_bits == v + 30
        got = texts(out)
        assert got == [pow(x, int(e), key.nsq) for x, e in zip(ct, c)] and got[0] == 1 and got[1] == ct[1]
        assert (mant(sk, out, k) == m.astype(object) * c.astype(object)[:, None]).all()
    # multipliers of 33 to 63 bits: two exponent words
    wide, mw = packed_ints(pk, rng, 5, 128, 3, v)
    cw = np.array([(1 << 40) + 9, -(1 << 62) - 5, 1 << 32, -3, 0], dtype=np.int64)
    out = wide.scale_rows(cw)
    assert out.value_bits == v + 63
    assert texts(out) == [pow(x, int(e), key.nsq) for x, e in zip(texts(wide), cw)]
    assert (mant(sk, out, 3) == mw.astype(object) * cw.astype(object)[:, None]).all()
    plain = p.scale_rows(np.abs(c))
    assert plain.ciphertext()._taint == () and texts(plain) == [pow(x, int(abs(e)), key.nsq) for x, e in zip(ct, c)]


# ---- dense W @ P ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [2048, 3072])
def test_dense_product_rows_are_the_products_of_powers(bits, monkeypatch, kernels):
    key, pk, sk = keypair(bits)
    rng = np.random.default_rng(bits)
    G, F, b, k, v = 67, 5, 64, 3, 20
    p, m = packed_ints(pk, rng, G, b, k, v)
    W = rng.integers(-(1 << 12) + 1, 1 << 12, (F, G)).astype(np.int64)
    W[2, :] = 0                                            # an output row without terms: the ciphertext 1
    W[:, 7] = 0                                            # a member no output uses
    ct = texts(p)
    want = want_rows(ct, W, key.nsq)
    wm = W.astype(object) @ m.astype(object)
    S = int(np.abs(W).sum(axis=1).max())
    assert want[2] == 1
    monkeypatch.setenv("PAI_MEXP_MIN_TERMS", "0")
    for lanes in (None, 335, 50, 1):                       # chunks of the default size, 1, 7 and 67 members
        for wbits in (None, 1):
            tune(monkeypatch, "mexp_lanes", lanes)
            tune(monkeypatch, "mexp_wbits", wbits)
            before = dict(packed.PACKED_ROUTES)
            out = (W @ p) if lanes is None else p.rmatmul(torch.from_numpy(W))
            assert packed.PACKED_ROUTES == {"fast": before["fast"] + 1, "composite": before["composite"]}
            assert (out.rows, len(out), out.slot_bits, out.slots, out.exponent) == (F, F * k, b, k, 0)
            assert out.value_bits == v + S.bit_length()
            assert len(out.ciphertext()._taint) == 1
            assert texts(out) == want, (lanes, wbits)
            assert (mant(sk, out, k) == wm).all(), (lanes, wbits)
    tune(monkeypatch, "mexp_lanes", None)
    tune(monkeypatch, "mexp_wbits", None)
    assert any(name == "ct_invert" and "k_invert" in ks for name, ks in kernels)
    # one output row from a vector
    one = p.rmatmul(W[0])
    assert one.rows == 1 and texts(one) == want[:1]
    # the defining route: the same bits
    monkeypatch.setenv("PAI_MEXP_MIN_TERMS", str(1 << 40))
    before = dict(packed.PACKED_ROUTES)
    out = W @ p
    assert packed.PACKED_ROUTES == {"fast": before["fast"], "composite": before["composite"] + 1}
    assert texts(out) == want and out.value_bits == v + S.bit_length()
    # non-negative weights: no inversion on either route, no taint
    Wp = np.abs(W)
    wantp = want_rows(ct, Wp, key.nsq)
    for min_terms in ("0", str(1 << 40)):
        monkeypatch.setenv("PAI_MEXP_MIN_TERMS", min_terms)
        del kernels[:]
        out = Wp @ p
        assert out.ciphertext()._taint == () and texts(out) == wantp
        assert [name for name, _ in kernels][0] == "fp_quantize" and "k_fp_quantize" in kernels[0][1]
        assert not any(name == "ct_invert" or "k_invert" in ks for name, ks in kernels), kernels


def test_float_weights_are_rounded_to_the_common_grid(monkeypatch):
    monkeypatch.delenv("PAI_MEXP_MIN_TERMS", raising=False)
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(31)
    G, F, b, k, v, E = 67, 5, 64, 3, 20, 4
    m = rng.integers(-(1 << v) + 1, 1 << v, (G, k))
    p = pk.encrypt_packed(np.ldexp(m.reshape(-1).astype(np.float64), -E), exponent=E, value_bits=v, slot_bits=b, slots=k,
                          apply_obfuscator=False)
    W = rng.normal(0, 3, (F, G))
    W[0, :4] = [0.5 / 1024, 1.5 / 1024, -2.5 / 1024, 1.0]   # ties at weight_exponent 10
    Wq = np.array([[quantize_one(x, 10) for x in row] for row in W.tolist()], dtype=object)
    assert Wq[0, :4].tolist() == [0, 2, -2, 1024]
    before = dict(packed.PACKED_ROUTES)
    out = p.rmatmul(W, weight_exponent=10)
    assert packed.PACKED_ROUTES["composite"] == before["composite"] + 1      # 335 weights: below the default threshold
    assert out.exponent == E + 10
    S = max(int(sum(abs(x) for x in row)) for row in Wq)
    assert out.value_bits == v + S.bit_length()
    wm = Wq @ m.astype(object)
    assert texts(out) == want_rows(texts(p), Wq, key.nsq)
    assert (mant(sk, out, k) == wm).all()
    got = sk.decrypt_packed(out).reshape(F, k)
    assert (got == np.array([[float(x) for x in row] for row in wm]) * 2.0 ** -(E + 10)).all()   # |sums| < 2^53: exact doubles
    for bad in (np.nan, np.inf):
        W[1, 3] = bad
        with pytest.raises(ValueError):
            p.rmatmul(W, weight_exponent=10)


def test_headroom_is_settled_before_any_paillier_kernel(monkeypatch, kernels):
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(41)
    G, F, b, k = 67, 2, 32, 3
    W = np.ones((F, G), dtype=np.int64)
    W[0, ::2] = -1
    W[1] = 3
    W[1, 60:] = -1                                         # S = max(67, 60 * 3 + 7) = 187: 8 bits
    S = 187
    assert int(np.abs(W).sum(axis=1).max()) == S
    v = b - 1 - S.bit_length()                             # v + bit_length(S) = b - 1: the last value that fits
    p, m = packed_ints(pk, rng, G, b, k, v, extremes=True)
    wm = W.astype(object) @ m.astype(object)
    for min_terms in ("0", str(1 << 40)):
        monkeypatch.setenv("PAI_MEXP_MIN_TERMS", min_terms)
        out = W @ p
        assert out.value_bits == b - 1
        assert (mant(sk, out, k) == wm).all()
    W[1, 0] = 3 + (256 - S)                                # S = 256: one more bit
    for min_terms in ("0", str(1 << 40)):
        monkeypatch.setenv("PAI_MEXP_MIN_TERMS", min_terms)
        del kernels[:]
        with pytest.raises(OverflowError):
            W @ p
        assert [name for name, _ in kernels] == ["fp_quantize"]
        assert list(engine.profile_last()) == ["k_fp_quantize"]       # nothing ran after the quantiser
    with pytest.raises(OverflowError):
        p.rmatmul(np.full((1, G), 2.0 ** 100), weight_exponent=26)     # |w| = 2^126
    assert list(engine.profile_last()) == ["k_fp_quantize"]           # (still the last call's: not even the quantiser ran)


# ---- csr_rmatmul ----------------------------------------------------------------------------------------------------------------------
def csr_case(rng, G):
    """m = 6 rows over G columns: row 1 empty, row 2 with a duplicate entry, a stored zero in row 3, mixed signs"""
    cols = [rng.choice(G, 9, replace=False).tolist(), [], [4, 11, 4, 30], [0, 66, 17], rng.choice(G, 40, replace=False).tolist(), [66]]
    data = [rng.integers(-4000, 4000, len(c)).tolist() for c in cols]
    data[3][1] = 0
    data[5] = [-(1 << 14)]
    indptr = np.cumsum([0] + [len(c) for c in cols])
    return indptr, np.array(sum(cols, []), dtype=np.int32), np.array(sum(data, []), dtype=np.int64), cols, data


@pytest.mark.parametrize("bits", [2048, 3072])
def test_csr_product_over_the_stored_entries(bits, monkeypatch):
    key, pk, sk = keypair(bits)
    rng = np.random.default_rng(50 + bits)
    G, b, k, v = 67, 64, 3, 20
    p, m = packed_ints(pk, rng, G, b, k, v)
    indptr, indices, data, cols, vals = csr_case(rng, G)
    ct = texts(p)
    want, wm = [], []
    for c, d in zip(cols, vals):
        acc, accm = 1, np.zeros(k, dtype=object)
        for l, w in zip(c, d):
            acc = acc * pow(ct[l], int(w), key.nsq) % key.nsq
            accm = accm + int(w) * m[l].astype(object)
        want.append(acc)
        wm.append(accm)
    S = max(sum(abs(w) for w in d) for d in vals)
    assert want[1] == 1
    for min_terms, route in (("0", "fast"), (str(1 << 40), "composite")):
        monkeypatch.setenv("PAI_MEXP_MIN_TERMS", min_terms)
        for chunk in ((2, None) if route == "fast" else (None,)):
            tune(monkeypatch, "smexp_chunk", chunk)
            before = packed.PACKED_ROUTES[route]
            out = p.csr_rmatmul(indptr, torch.from_numpy(indices), data, (6, G))
            assert packed.PACKED_ROUTES[route] == before + 1
            assert (out.rows, len(out), out.slot_bits, out.slots, out.exponent) == (6, 6 * k, b, k, 0)
            assert out.value_bits == v + S.bit_length()    # the largest per-row sum, not the sum of everything
            assert texts(out) == want, (route, chunk)
            assert (mant(sk, out, k) == np.array(wm, dtype=object)).all()
    tune(monkeypatch, "smexp_chunk", None)
    # float data on the grid of weight_exponent 1
    out = p.csr_rmatmul(indptr, indices, data / 2.0, (6, G), weight_exponent=1)
    assert out.exponent == 1 and texts(out) == want
    # no stored entry at all
    none = p.csr_rmatmul(np.zeros(4, dtype=np.int64), indices[:0], data[:0], (3, G))
    assert texts(none) == [1, 1, 1] and none.value_bits == v


def test_csr_product_from_a_scipy_matrix(monkeypatch):
    sp = pytest.importorskip("scipy.sparse")
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(61)
    G, b, k, v = 67, 64, 3, 20
    p, m = packed_ints(pk, rng, G, b, k, v)
    A = sp.random(6, G, density=0.2, random_state=5, data_rvs=lambda n: rng.integers(-500, 500, n)).astype(np.int64).tocsr()
    dense = np.asarray(A.todense()).astype(np.int64)
    monkeypatch.setenv("PAI_MEXP_MIN_TERMS", "0")
    for mat in (A, A.tocoo(), A.tocsc()):
        out = mat @ p
        assert texts(out) == want_rows(texts(p), dense, key.nsq)
        assert (mant(sk, out, k) == dense.astype(object) @ m.astype(object)).all()


# ---- the pipeline and the empty container ----------------------------------------------------------------------------------------------
def test_gradient_pipeline_and_pickle():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(71)
    G, F, k, b, v = 67, 5, 3, 64, 24
    D = rng.integers(-(1 << 20), 1 << 20, (G, k))         # residuals: k outputs per sample
    X = rng.integers(-100, 100, (G, F))
    P = pk.encrypt_packed(D.reshape(-1).astype(np.int64), exponent=0, value_bits=v, slot_bits=b, slots=k)
    grad = X.T @ P
    assert grad.rows == F and grad.slots == k
    flat = grad.repack()
    assert flat.rows == 1 and len(flat) == F * k
    assert (np.array(sk.decrypt_packed_mantissas(flat), dtype=object).reshape(F, k) == X.T.astype(object) @ D.astype(object)).all()
    assert (sk.decrypt_packed(flat).reshape(F, k) == (X.T @ D).astype(np.float64)).all()
    back = pickle.loads(pickle.dumps(grad))
    assert texts(back) == texts(grad) and (back.rows, back.slots, back.value_bits, back.exponent) == (F, k, grad.value_bits, 0)


def test_container_without_rows_launches_nothing(kernels):
    key, pk, sk = keypair(2048)
    p = pk.encrypt_packed(np.zeros(0), exponent=3, value_bits=20, slot_bits=64, slots=3)
    del kernels[:]
    out = np.zeros((5, 0)) @ p
    assert out.rows == 0 and len(out) == 0 and out.exponent == 3 and out.value_bits == 20
    assert p.scale_rows(np.zeros(0, dtype=np.int64)).rows == 0
    assert kernels == []
