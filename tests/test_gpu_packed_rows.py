"""GPU: the row operations of packed ciphertexts — PaillierPackedNumber.segment_sum / cumsum / sum / take / repack and the
pai_ct_pack_step entry point, every check exact.

The expectations are CPython products and powers modulo n^2 of the input rows' getTexts() (tests/_util.pow_many for the wide
powers), numpy integer sums of the mantissas, and float64 sums with the rounding bound of rint(x 2^E) — never the code under
test.  The chunk levels of the chain runners are crossed with PAI_TUNE segprod_chunk / scan_chunk, both routes of the stepped
pack chain are forced (PAI_DISABLE=pack_padic / PAI_TUNE pack_padic_min=0) and the kernels that ran are read from
pai_profile_last, as tests/test_gpu_packed.py does."""
import ctypes
import json
from pathlib import Path
import pickle

import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import PaillierPrivateKey, PaillierPublicKey, _native, engine, packed
from pailliercryptolib_python_amd.bindings import ipclPublicKey

from ._util import disable, pow_many, rand_below, tune

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


def rows_of(t):
    return engine.words_to_ints(engine.to_host_words(t))


def call_status(h):
    """the handle's sticky status word (pai_pubkey_status), left in place"""
    v = ctypes.c_int(-1)
    _native.check(h.lib.pai_pubkey_status(h.h, ctypes.byref(v), 0, None))
    return v.value


def prod(vals, nsq):
    acc = 1
    for v in vals:
        acc = acc * v % nsq
    return acc


def packed_ints(pk, rng, G, b, k, v, E=0):
    """(container of G full rows of integers |x| < 2^v at exponent E, so value_bits v + E; its mantissas as an int64 [G, k]
    matrix): raw encryptions — the chains under test do not care"""
    m = rng.integers(-(1 << v) + 1, 1 << v, (G, k))
    p = pk.encrypt_packed(m.reshape(-1), exponent=E, value_bits=v + E, slot_bits=b, slots=k, apply_obfuscator=False)
    return p, m.astype(np.int64) << E


def mant(sk, p, k):
    return np.array(sk.decrypt_packed_mantissas(p), dtype=object).reshape(-1, k)


def shape_of(p):
    return (p.rows, len(p), p.slot_bits, p.slots, p.exponent)


# ---- segment_sum -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3])
def test_segment_sum_rows_are_the_products_of_their_members(F, monkeypatch):
    key, pk, sk = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(100 + F)
    G, K, b, k, v = 700, 9, 64, 2, 30
    p, m = packed_ints(pk, rng, G, b, k, v, E=3)
    ids = rng.integers(0, K - 1, (G, F))                   # bin K - 1 stays empty
    ids[rng.random((G, F)) < 0.1] = -1                     # dropped pairs
    ids[rng.random(G) < 0.6, 0] = 2                        # one dominant bin: longer than a chunk
    ct = texts(p)
    want = [prod([ct[i] for i in range(G) if ids[i, f] == s], key.nsq) for f in range(F) for s in range(K)]
    cmax = max(int((ids[:, f] == s).sum()) for f in range(F) for s in range(K))
    wm = np.array([[int(m[ids[:, f] == s, j].sum()) for j in range(k)] for f in range(F) for s in range(K)], dtype=object)
    for chunk, arg in ((None, ids if F > 1 else ids[:, 0]), (3, torch.from_numpy(ids)), (16, ids.astype(np.int32))):
        tune(monkeypatch, "segprod_chunk", chunk)
        out = p.segment_sum(arg, K)
        assert shape_of(out) == (F * K, F * K * k, b, k, 3), chunk
        assert out.value_bits == v + 3 + (cmax - 1).bit_length()
        assert texts(out) == want, chunk
        assert want[K - 1] == 1                            # the empty segment
        assert (mant(sk, out, k) == wm).all(), chunk
    tune(monkeypatch, "segprod_chunk", None)
    assert call_status(h) == 0


# ---- cumsum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
def test_cumsum_rows_are_prefix_products(reverse, monkeypatch):
    key, pk, sk = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(200 + reverse)
    b, k, v = 100, 2, 40
    for G, L, chunks in ((96, 16, (None, 5, 64)), (60, None, (7,)), (60, 1, (None,))):
        p, m = packed_ints(pk, rng, G, b, k, v)
        ct = texts(p)
        run = G if L is None else L
        want, wm = [], []
        for r0 in range(0, G, run):
            idx = list(range(r0, r0 + run))
            if reverse:
                idx.reverse()
            acc, row, accm, rowm = 1, {}, np.zeros(k, dtype=object), {}
            for i in idx:
                acc = acc * ct[i] % key.nsq
                accm = accm + m[i].astype(object)
                row[i], rowm[i] = acc, accm
            want += [row[i] for i in range(r0, r0 + run)]
            wm += [rowm[i] for i in range(r0, r0 + run)]
        mm = m.reshape(-1, run, k)
        np_cum = (np.cumsum(mm[:, ::-1], axis=1)[:, ::-1] if reverse else np.cumsum(mm, axis=1)).reshape(G, k)
        assert (np.array(wm, dtype=object) == np_cum).all()
        for chunk in chunks:                               # runs shorter and longer than one chunk of scan positions
            tune(monkeypatch, "scan_chunk", chunk)
            out = p.cumsum(L, reverse=reverse)
            assert shape_of(out) == (G, G * k, b, k, 0) and out.value_bits == v + (run - 1).bit_length()
            assert texts(out) == want, (G, L, chunk)        # the wire form, wherever the rows rested
            assert (mant(sk, out, k) == np_cum).all(), (G, L, chunk)
        tune(monkeypatch, "scan_chunk", None)
    assert call_status(h) == 0


# ---- sum and take ----------------------------------------------------------------------------------------------------------------
def test_sum_and_take():
    key, pk, sk = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(300)
    G, b, k, v = 37, 32, 5, 20
    p, m = packed_ints(pk, rng, G, b, k, v)
    ct = texts(p)
    s = p.sum()
    assert shape_of(s) == (1, k, b, k, 0) and s.value_bits == v + (G - 1).bit_length()
    assert texts(s) == [prod(ct, key.nsq)]
    assert (mant(sk, s, k) == m.sum(axis=0)).all()
    one = p.take([4]).sum()                                # one row: the row itself
    assert texts(one) == [ct[4]] and one.value_bits == v
    perm = rng.permutation(G)
    for rows in (perm, torch.from_numpy(perm), [3, 3, 0, 3, G - 1, -1, -G], slice(5, 30, 4), slice(None, None, -1),
                 np.array([], dtype=np.int64)):
        idx = list(range(G))[rows] if isinstance(rows, slice) else [int(i) % G for i in np.asarray(rows).tolist()]
        t = p.take(rows)
        assert shape_of(t) == (len(idx), len(idx) * k, b, k, 0) and t.value_bits == v
        assert texts(t) == [ct[i] for i in idx]
        if idx:
            assert (mant(sk, t, k) == m[idx]).all()
    # a cumulative histogram's rows rest at a Montgomery tag: take and sum still give the wire form
    c = p.take(slice(0, 36)).cumsum(6)
    picked = texts(c.take([5, 11, 35]))                    # (before c itself is read: the gather runs on the tagged rows)
    cw = texts(c)
    assert picked == [cw[5], cw[11], cw[35]]
    assert texts(p.take(slice(0, 36)).cumsum(6).sum()) == [prod(cw, key.nsq)]
    with pytest.raises(IndexError):
        p.take([G])
    assert call_status(h) == 0


# ---- pai_ct_pack_step and repack --------------------------------------------------------------------------------------------------
def want_stepped(cts, step, count, nsq):
    """prod_(j<count) ct_(g count + j)^(2^(step j)) mod n^2 per output row, the powers through tests/_util.pow_many"""
    pw = pow_many(cts, [1 << (step * (i % count)) for i in range(len(cts))], nsq)
    return [prod(pw[g:g + count], nsq) for g in range(0, len(cts), count)]


def step_rows_and_kernels(h, t, step, count, tag=0):
    engine.profile_enable(True)
    try:
        rows = rows_of(h.ct_pack_step(t, step, count, tag=tag))
        return rows, set(engine.profile_last())
    finally:
        engine.profile_enable(False)


@pytest.mark.parametrize("bits,step,count,N", [(2048, 200, 10, 43), (2048, 1023, 2, 7), (2048, 682, 3, 4), (1024, 129, 7, 30),
                                               (2048, 8, 255, 300), (3072, 1535, 2, 5), (4096, 1000, 4, 9)])
def test_ct_pack_step_equals_the_product_of_powers_on_both_routes(bits, step, count, N, monkeypatch):
    key, pk, _ = keypair(bits)
    h = pk.pubkey.handle
    assert count * step <= key.n.bit_length() - 2 and N % count       # a ragged last chain
    rng = np.random.default_rng(bits + step)
    cts = rand_below(rng, key.nsq, N)
    t = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
    want = want_stepped(cts, step, count, key.nsq)
    assert rows_of(h.ct_pack_step(t, step, count)) == want             # the default dispatch
    disable(monkeypatch, "pack_padic")
    rows_a, kern_a = step_rows_and_kernels(h, t, step, count)
    assert rows_a == want
    assert "k_segprod" in kern_a and "k_ct_pack_padic" not in kern_a, kern_a
    for chunk in (1, 2, 3):                                # chunk joins at shift step * (chunk length), levels deep
        tune(monkeypatch, "segprod_chunk", chunk)
        assert rows_of(h.ct_pack_step(t, step, count)) == want, chunk
    tune(monkeypatch, "segprod_chunk", None)
    for tag in (1, -1):                                    # rows at a lazy domain tag in, the wire form out
        assert rows_of(h.ct_pack_step(h.ct_retag(t, 0, tag), step, count, tag=tag)) == want, tag
    disable(monkeypatch, "pack_padic", False)
    tune(monkeypatch, "pack_padic_min", 0)
    rows_b, kern_b = step_rows_and_kernels(h, t, step, count)
    tune(monkeypatch, "pack_padic_min", None)
    assert rows_b == want
    if bits <= 2048:                                       # the digit engine serves keys up to 2048 bits; above, route A alone
        assert "k_ct_pack_padic" in kern_b and "k_segprod" not in kern_b, kern_b
    else:
        assert "k_segprod" in kern_b and "k_ct_pack_padic" not in kern_b, kern_b
    assert call_status(h) == 0


@pytest.mark.parametrize("bits,b,k,N", [(2048, 64, 31, 100), (2048, 128, 3, 10), (1024, 8, 127, 300), (3072, 100, 7, 20)])
def test_ct_pack_and_ct_pack_step_give_identical_bits(bits, b, k, N, monkeypatch):
    key, pk, _ = keypair(bits)
    h = pk.pubkey.handle
    cts = rand_below(np.random.default_rng(bits + b), key.nsq, N)
    t = engine.to_device_words(engine.ints_to_words(cts, h.ct_words), h.device)
    for route in ("a", "b"):
        disable(monkeypatch, "pack_padic", route == "a")
        tune(monkeypatch, "pack_padic_min", 0 if route == "b" else None)
        assert torch.equal(h.ct_pack(t, b, k), h.ct_pack_step(t, b, k)), route
    assert call_status(h) == 0


def test_ct_pack_step_invalid_steps_launch_nothing():
    key, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    ct = h.empty_ct(8)
    engine.profile_enable(True)
    try:
        h.ct_pack_step(ct.zero_() + 1, 64, 2)              # something for the profile list to hold
        before = engine.profile_last()
        assert before
        for step, count in ((7, 1), (0, 1), (-8, 2), (8, 256), (1024, 2), (2047, 1), (682, 4), (64, 0), (64, -1), (1 << 30, 4)):
            out = h.empty_ct(8)
            rc = h.lib.pai_ct_pack_step(h.h, ct.data_ptr(), 8, 0, step, count, out.data_ptr(), None)
            assert rc == _native.PAI_E_INVALID, (step, count)
        with pytest.raises(_native.NativeError) as e:
            h.ct_pack_step(ct, 1023, 3)
        assert e.value.code == _native.PAI_E_INVALID
        assert engine.profile_last() == before             # no call got as far as clearing the list, let alone a launch
    finally:
        engine.profile_enable(False)
    # the edges that fit: 2046 = bits(n) - 2
    assert h.ct_pack_step(ct, 2046, 1).shape[0] == 8 and h.ct_pack_step(ct, 1023, 2).shape[0] == 4
    assert call_status(h) == 0


@pytest.mark.parametrize("route", ["a", "b"])
def test_repack_rows_and_elements(route, monkeypatch):
    key, pk, sk = keypair(2048)
    h = pk.pubkey.handle
    disable(monkeypatch, "pack_padic", route == "a")
    tune(monkeypatch, "pack_padic_min", 0 if route == "b" else None)
    rng = np.random.default_rng(400)
    b, k, v, E = 100, 2, 60, 7
    N = 2 * 47 - 1                                         # 47 rows, the last one half full; 10 rows fit one: a ragged last chain
    x = rng.integers(-(1 << 50), 1 << 50, N)
    p = pk.encrypt_packed(x, exponent=E, value_bits=v, slot_bits=b, slots=k)
    ct = texts(p)
    for f, fa in ((10, None), (10, 10), (3, 3), (1, 1)):
        engine.profile_enable(True)
        try:
            q = p.repack(factor=fa)
            kern = set(engine.profile_last())
        finally:
            engine.profile_enable(False)
        assert shape_of(q) == (-(-47 // f), N, b, k * f, E) and q.value_bits == v
        assert texts(q) == (want_stepped(ct, k * b, f, key.nsq) if f > 1 else ct), f
        if f > 1:
            assert ("k_segprod" in kern) == (route == "a") and ("k_ct_pack_padic" in kern) == (route == "b"), kern
        assert sk.decrypt_packed_mantissas(q) == [int(t) << E for t in x], f
        assert np.array_equal(sk.decrypt_packed(q), x.astype(np.float64))
    q = p.repack(factor=1)
    assert q.ciphertext().words.data_ptr() != p.ciphertext().words.data_ptr()      # a copy
    with pytest.raises(ValueError):
        p.repack(factor=11)
    # rows that rest at the scan's Montgomery tag go in as they are
    c = p.take(slice(0, 40)).cumsum(8)
    assert texts(c.repack(factor=4)) == want_stepped(texts(c), k * b, 4, key.nsq)
    assert call_status(h) == 0


# ---- end to end: GH packing --------------------------------------------------------------------------------------------------------
def test_gh_packed_histogram_pipeline():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(500)
    N, F, K, b, E = 1500, 4, 16, 100, 40
    g = rng.uniform(-1, 1, N)
    hs = rng.uniform(0, 1, N)
    gh = np.stack([g, hs], axis=1).reshape(-1)             # (g_i, h_i) share plaintext i
    ids = rng.integers(0, K, (N, F))
    p = pk.encrypt_packed(gh, exponent=E, value_bits=E + 1, slot_bits=b, slots=2)
    assert p.rows == N
    hist = p.segment_sum(ids, K)
    cum = hist.cumsum(K)
    out = cum.repack()
    assert (hist.rows, cum.rows, out.rows, out.slots, len(out)) == (F * K, F * K, -(-F * K // 10), 20, F * K * 2)
    m = np.rint(np.ldexp(gh, E)).astype(np.int64).reshape(N, 2)            # exact: |x 2^E| < 2^41
    want = np.zeros((F, K, 2), dtype=np.int64)
    wantf = np.zeros((F, K, 2))
    count = np.zeros((F, K), dtype=np.int64)
    for f in range(F):
        for s in range(K):
            sel = ids[:, f] == s
            want[f, s] = m[sel].sum(axis=0)
            wantf[f, s] = [np.sum(g[sel]), np.sum(hs[sel])]                 # float64 sums of the inputs themselves
            count[f, s] = sel.sum()
    want, wantf, count = np.cumsum(want, axis=1), np.cumsum(wantf, axis=1), np.cumsum(count, axis=1)
    assert sk.decrypt_packed_mantissas(out) == [int(t) for t in want.reshape(-1)]
    got = sk.decrypt_packed(out).reshape(F, K, 2)
    # rint(x 2^E) moves every element by at most 2^-(E+1): a prefix of c samples is within c 2^-(E+1) of the float64 sum
    err = np.abs(got - wantf)
    tol = np.broadcast_to(count[:, :, None] * 2.0 ** -(E + 1), err.shape)
    print("gh pipeline: largest |error| / (c 2^-(E+1)) =", float((err[tol > 0] / tol[tol > 0]).max()))
    assert (err <= tol).all()


# ---- headroom, taint, pickling ---------------------------------------------------------------------------------------------------
def test_overflow_is_raised_before_any_paillier_kernel():
    key, pk, _ = keypair(2048)
    h = pk.pubkey.handle
    rng = np.random.default_rng(600)
    p, _ = packed_ints(pk, rng, 40, 32, 3, 27)             # 4 spare bits: sums of up to 16 rows
    h.check_status(force=True)
    engine.profile_enable(True)
    try:
        ok = p.take(slice(0, 16)).sum()
        assert ok.value_bits == 31
        before = engine.profile_last()
        assert before
        with pytest.raises(OverflowError):
            p.sum()
        with pytest.raises(OverflowError):
            p.cumsum()
        with pytest.raises(OverflowError):
            p.cumsum(20, reverse=True)
        with pytest.raises(OverflowError):
            p.segment_sum(np.zeros(40, dtype=np.int64), 2)             # 40 members in one segment
        with pytest.raises(OverflowError):
            p.segment_sum(np.array([0] * 17 + [1] * 23).reshape(40, 1), 2)
        with pytest.raises(OverflowError):
            ok.take([0, 0]).sum()                          # full slots: nothing more fits
        assert engine.profile_last() == before             # no library call cleared the list: nothing was launched
        assert p.segment_sum(np.arange(40) % 3, 3).value_bits == 27 + 4  # 14 members: passes
        assert p.cumsum(8).value_bits == 30
    finally:
        engine.profile_enable(False)
    assert call_status(h) == 0


def test_taint_travels_with_every_result():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(700)
    p, m = packed_ints(pk, rng, 12, 64, 2, 30)
    q = p * -1
    assert len(q.ciphertext()._taint) == 1
    flag = q.ciphertext()._taint[0]
    outs = {"segment_sum": q.segment_sum(np.arange(12) % 3, 3), "cumsum": q.cumsum(4), "sum": q.sum(), "take": q.take([1, 0]),
            "repack": q.repack(factor=3), "copy": q.repack(factor=1)}
    for name, r in outs.items():
        assert any(f is flag for f in r.ciphertext()._taint), name
    assert (mant(sk, outs["sum"], 2) == -m.sum(axis=0)).all()
    assert sk.decrypt_packed_mantissas(outs["repack"]) == [-int(t) for t in m.reshape(-1)]
    assert texts(outs["take"]) == [texts(q)[1], texts(q)[0]]              # a clean outcome: the rows leave the device


def test_results_pickle_round_trip():
    key, pk, sk = keypair(2048)
    rng = np.random.default_rng(800)
    p, m = packed_ints(pk, rng, 24, 64, 2, 30, E=5)
    for r in (p.segment_sum(np.arange(24) % 4, 4), p.cumsum(6), p.sum(), p.take([5, 2]), p.cumsum(6).repack(factor=5)):
        q = pickle.loads(pickle.dumps(r))
        assert shape_of(q) == shape_of(r) and q.value_bits == r.value_bits
        assert texts(q) == texts(r)
        assert sk.decrypt_packed_mantissas(q) == sk.decrypt_packed_mantissas(r)
    assert isinstance(packed.sum_value_bits(1, 1, 8), int)
