"""GPU: the aggregation kernels against CPython integers on the limit keys of tests/golden/limit_keys.json and the structured
keys of tests/golden/extreme_keys.json, with corner operands.

Every kernel that works modulo M = n^2 on the lane-group Montgomery engine keeps lazy residues in [0, 2M) between products; that
is sound because R = 2^(29 NL) >= 4M (csrc/paillier_capi.hip: geo_for_bits).  k_addn, k_segprod, k_segscan and k_smexp / k_mexp
run arbitrarily many products on one accumulator, move it between powers of R through the key's table (|m| <= RPOW_SPAN) and
call cond_sub once, at the end.  The limit keys put n^2 at 29 NL - 2 bits of each geometry, R/M just above 4 (`hi`) and just below
8 (`lo`) — every other key of the suite has R/M >= 16 — and the latency limits (NL = 48 / 96 / 192) do the same to the
integer-per-wavefront products of the small-batch paths (tests/test_limit_keys_cpu.py holds the fixture).

Keys: the 15 limit keys and the 27 structured keys, one module-scoped pair of raw-ABI handles each (test_gpu_extreme_keys.Key: DJN,
fixed x); any status but PAI_OK at creation fails.  Operands: test_gpu_extreme_keys.ciphertexts() — the 10 corners (0, 1, 2,
n - 1, n, n + 1, M - 1, M - 2, M - n, (n - 1) n), the 49 cells of the p^2 / q^2 CRT grid and a pattern tail (runs of ones, single
bits, values next to 0 and M).  Batches are one full and one ragged workgroup tile: 70 chains or elements at 64 per tile, 37 at 32
(keys of 4000 bits and more; their 74 operands go in two batches).  Every comparison is bit-exact against CPython integers (bulk
powers through tests/_util.pow_many).

Not vacuous: a row that is 0, or two rows that are multiples of n, annihilate a chain and hide what follows.  Rows that are no
units (4 of the 70, plus a 0 the pattern tail may add) are placed as the LAST member of a chain, in chains of their own, or — in
the element-wise calls — in the operand that is not squared; every expectation passes live(): at most 1 in 8 outputs of a call is 0.

What ran is read back per call (pai_profile_last / pai_profile_last_path) and printed as COVERAGE lines by the last test, which
requires k_addn, k_segprod and k_segscan on every lane-group geometry (36 x 1 ... 36 x 8) at a limit key of that geometry, and on
every latency limit key (these kernels have no latency form: a latency limit key runs them on the lane-group geometry above
it, with room to spare; its own limit is met by the k_modmul:lat / k_add_aligned:lat / k_pow2:lat products of test_limit_ct_add_family).

Documented hand-downs (asserted, and printed as HANDDOWN lines):
  * pai_ct_pack / pai_ct_pack_step above the hand-over run one chain per lane on digit pairs (k_ct_pack_padic) only where the base-n
    digit engine serves n (csrc/padic_enc_kernels.hip: padic_enc_nl_for_n_bits — 700 .. 1024 and 1400 .. 2068 bits) and the rows are
    in the wire form; every other key, and every tagged input, takes the k_segprod levels on both sides.
  * pai_ct_sparse_multiexp runs k_smexp on digit pairs on those same keys and on lane groups elsewhere; the digit-served keys run
    a second time on a handle created with PAI_DISABLE=padic.  Of the limit keys only hi-nl112 / lo-nl112 (n of 1623 bits) are digit-served.
  * pai_ct_add on a limit key never takes the most-significant-limb-first product: build_msb_ctx refuses a modulus whose top limb
    is the geometry's (off = 0) or holds 27 bits; the Montgomery products (k_modmul) serve, which test_ct_add_family reports."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from pailliercryptolib_python_amd import _native
from tests import test_gpu_extreme_keys as xkeys
from tests._util import DevArray, ints_to_limbs, limbs_to_ints, pow_many, tune
from tests._util import disable as knob_disable
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_cumsum import want_chain
from tests.test_gpu_extreme_keys import Key, ciphertexts, plain
from tests.test_gpu_packed import want_packed
from tests.test_gpu_packed_rows import want_stepped
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels
from tests.test_limit_keys_cpu import LANE_GROUP_NL, LATENCY_NL, load_limit_keys

pytestmark = pytest.mark.gpu

LIMIT = [("limit",) + e for e in load_limit_keys()]
EXTREME = [("extreme",) + e for e in load_extreme_keys()]
PARAMS = LIMIT + EXTREME
IDS = [e[1] for e in PARAMS]
RB = 29
RPOW_SPAN = 48                       # csrc/kernels_paillier.hpp
COV = {}                             # (operation, lane-group limbs of the key's handle) -> {"kernel:path"}
LIMIT_RAN = {}                       # (kernel, engine, fixture limbs) -> limbs of the geometry it ran on
XSEEN = {}                           # what the bodies of test_gpu_extreme_keys.py record on the limit keys
HANDDOWN = set()
VISITED = set()


@pytest.fixture(scope="module", params=PARAMS, ids=IDS)
def ak(request):
    lib = _native.load()
    _native.check(lib.pai_profile_enable(1))
    e = request.param
    if e[0] == "limit":
        _, ident, kind, nl, engine, pb, p, q = e
        k = Key(ident, kind, pb, p, q)
        k.limit = (engine, nl)
    else:
        k = Key(*e[1:])
        k.limit = None
    rb = C.c_int(0)
    _native.check(lib.pai_pubkey_mont_bits(k.nk.pk, C.byref(rb)))
    assert rb.value % RB == 0 and rb.value >= k.key.nsq.bit_length() + 2
    k.NL = rb.value // RB
    if k.limit and k.limit[0] == "lane_group":
        assert k.NL == k.limit[1], "a limit key must sit on the geometry it is the limit of"
    k.R = pow(2, rb.value, k.key.nsq)
    k.digit = 700 <= k.key.n.bit_length() <= 1024 or 1400 <= k.key.n.bit_length() <= 2068
    VISITED.add(k.ident)
    yield k
    _native.check(lib.pai_profile_enable(0))


limit_only = pytest.mark.parametrize("ak", LIMIT, indirect=True, ids=IDS[:len(LIMIT)])


def ran(k, op):
    """the kernels of the last library call as "name:path", recorded per operation and geometry"""
    lib = k.nk.lib
    names = _last_kernels(lib)
    buf = C.create_string_buffer(64)
    out = []
    for i, nm in enumerate(names):
        _native.check(lib.pai_profile_last_path(i, buf, 64))
        out.append(f"{nm}:{buf.value.decode()}")
        if k.limit:
            LIMIT_RAN[(nm,) + k.limit] = k.NL
    COV.setdefault((op, k.NL), set()).update(out)
    return out


def rpow(k, m):
    return pow(k.R, m, k.key.nsq)


def tagged(k, vals, tag):
    f = rpow(k, tag)
    return [v * f % k.key.nsq for v in vals]


def dev(k, vals):
    return DevArray(ints_to_limbs(vals, k.nk.cw))


def at(d, rows, k):
    return C.c_void_p(d.ptr.value + 4 * k.nk.cw * rows)


def live(want):
    """the condition on the oracle values: at most 1 in 8 expected outputs of a call is 0"""
    assert 8 * sum(1 for w in want if w == 0) <= len(want), "vacuous: too many expected outputs are 0"
    return want


def split(k, pool):
    """(indices of the rows that are no units modulo n, the units in pool order)"""
    bad = [i for i, c in enumerate(pool) if math.gcd(c, k.key.n) != 1]
    assert 4 <= len(bad) <= 7 and pool[0] == 0 and pool[4] == k.key.n
    return bad, [c for i, c in enumerate(pool) if i not in bad]


def unit_rows(k, seed, rot=0):
    u = ciphertexts(k, k.T, seed, units=True)
    assert all(math.gcd(c, k.key.n) == 1 for c in u)
    return u[rot % k.T:] + u[:rot % k.T]


def tile(k):
    return 64 if k.N == 70 else 32


# ---- pai_ct_addn ----------------------------------------------------------------------------------------------------------------
def test_addn(ak):
    """k in {2, 5, 16} x (tag0, tag) in {(0,0), (1,1), (0,1), (-2,3)} x dom_out in {0, 1, the natural tag}, without raise arrays and
    with per-element raises in 0..3: one operand random, one with an all-zero full tile and a single raised element in the ragged
    tile, one all zero, the others NULL; operand 0 is raised where the call allows it (tag0 == tag).  Operand 0 is the corner set
    itself, operands 1..15 its units rotated by 5 j rows, so that every corner meets different corners."""
    k, nk = ak, ak.nk
    M, N, W = k.key.nsq, k.N, k.nk.cw
    pool = ciphertexts(k, k.T, 31)
    bad, _ = split(k, pool)
    ops = [pool] + [unit_rows(k, 32 + j, 5 * j) for j in range(1, 16)]
    d0 = {t: dev(k, tagged(k, pool, t)) for t in (0, 1, -2)}
    dj = {t: [None] + [dev(k, tagged(k, ops[j], t)) for j in range(1, 16)] for t in (0, 1, 3)}
    out = DevArray(shape=(N, W))
    rng = np.random.default_rng(k.b)
    for off in k.offs:
        r0 = rng.integers(0, 4, N).astype(np.int32)
        for i in bad:                                                  # a squared multiple of n is 0
            if off <= i < off + N:
                r0[i - off] = 0
        r_rand, r_rand2 = rng.integers(0, 4, N).astype(np.int32), rng.integers(0, 4, N).astype(np.int32)
        r_single, r_zero = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        r_single[N - 2] = 3
        assert N - 2 >= tile(k)
        layout = [None, r_rand, r_single, r_zero, None, r_rand2] + [None] * 10
        draise = {id(r): DevArray(r) for r in (r0, r_rand, r_rand2, r_single, r_zero)}
        for kk in (2, 5, 16):
            rz = [None, r_single] if kk == 2 else layout[:kk]
            want = {}
            for mode in ("plain", "raised", "raised0"):                # no raises / operands 1.. raised / operand 0 as well
                acc = [1] * N
                for j in range(kk):
                    r = None if mode == "plain" else (r0 if j == 0 and mode == "raised0" else rz[j])
                    col = ops[j][off:off + N]
                    if r is not None:
                        col = [pow(x, 1 << int(s), M) for x, s in zip(col, r)]
                    acc = [a * x % M for a, x in zip(acc, col)]
                want[mode] = live(acc)
            ptr_r = {"plain": None}
            for mode, first in (("raised", None), ("raised0", r0)):
                ptr_r[mode] = (C.c_void_p * kk)(*[None if r is None else draise[id(r)].ptr.value for r in [first] + rz[1:]])
            for tag0, tag in ((0, 0), (1, 1), (0, 1), (-2, 3)):
                ptrs = (C.c_void_p * kk)(*([at(d0[tag0], off, k).value] + [at(dj[tag][j], off, k).value for j in range(1, kk)]))
                for dom in sorted({0, 1, tag0 + (kk - 1) * (tag - 1)}):
                    assert abs(dom) <= RPOW_SPAN
                    f = rpow(k, dom)
                    for mode in ("plain", "raised0" if tag0 == tag else "raised"):
                        _native.check(nk.lib.pai_ct_addn(nk.pk, ptrs, ptr_r[mode], kk, tag0, tag, dom, N, out.ptr, None))
                        path = ran(k, "addn")
                        assert limbs_to_ints(out.get()) == [w * f % M for w in want[mode]], (k.ident, off, kk, tag0, tag, dom, mode, path)
                        assert path == ["k_addn:"], (k.ident, path)


# ---- pai_ct_add_plain, pai_ct_add_aligned_dom -------------------------------------------------------------------------------------
def test_add_plain_and_add_aligned_dom(ak, monkeypatch):
    """pai_ct_add_plain: ct (1 + m n) with m in the plain() corners, on lane groups and on the latency geometry; pai_ct_add_aligned_dom
    at dom in {0, 1} with delta in -3 .. 8: a b^(2^delta) or a^(2^-delta) b, at the operands' tag."""
    k, nk = ak, ak.nk
    M, n, N, W = k.key.nsq, k.key.n, k.N, k.nk.cw
    a = ciphertexts(k, k.T, 51)
    bad, _ = split(k, a)
    b = unit_rows(k, 52, 23)
    m = plain(k, k.T, 53)
    assert m[:3] == [0, 1, n - 1]
    dm, da = DevArray(ints_to_limbs(m, nk.nw)), dev(k, a)
    out = DevArray(shape=(N, W))
    want = [x * (1 + y * n) % M for x, y in zip(a, m)]
    for lat in ("0", "4096"):
        monkeypatch.setenv("PAI_LAT_ADD_MAX", lat)
        for off in k.offs:
            _native.check(nk.lib.pai_ct_add_plain(nk.pk, at(da, off, k), C.c_void_p(dm.ptr.value + 4 * nk.nw * off), N, out.ptr, None))
            path = ran(k, f"add_plain(lat_add_max={lat})")
            assert limbs_to_ints(out.get()) == live(want[off:off + N]), (k.ident, lat, off, path)
            assert path == ["k_encrypt(add_plain):"], (k.ident, path)
    monkeypatch.delenv("PAI_LAT_ADD_MAX")
    rng = np.random.default_rng(k.b + 1)
    delta = rng.integers(-3, 9, k.T).astype(np.int32)
    for off in k.offs:
        delta[off:off + 6] = [0, 1, -3, 8, -1, 7]
    for i in bad:
        delta[i] = abs(int(delta[i]))                                  # a multiple of n is not squared (its square is 0)
    assert delta.min() == -3 and delta.max() == 8
    dd = DevArray(delta)
    want = [x * pow(y, 1 << int(d), M) % M if d > 0 else pow(x, 1 << int(-d), M) * y % M for x, y, d in zip(a, b, delta)]
    for dom in (0, 1):
        entry = dev(k, [rpow(k, 2 - dom)])
        ta, tb = dev(k, tagged(k, a, dom)), dev(k, tagged(k, b, dom))
        f = rpow(k, dom)
        for off in k.offs:
            _native.check(nk.lib.pai_ct_add_aligned_dom(nk.pk, at(ta, off, k), at(tb, off, k), 0, C.c_void_p(dd.ptr.value + 4 * off), N,
                                                        out.ptr, entry.ptr, None))
            path = ran(k, "add_aligned_dom")
            assert limbs_to_ints(out.get()) == [w * f % M for w in live(want[off:off + N])], (k.ident, dom, off, path)
            assert path == ["k_add_aligned:lane_group"], (k.ident, path)


# ---- pai_ct_segment_prod ----------------------------------------------------------------------------------------------------------
def seg_plan(k, pool, seed):
    """(rows, shift, offsets) of k.N chains with lengths 50, 17, 3, 2, 1, 0 in turn: a gather with repeats over the units of the
    pool (every unit at least once), shifts in 0..3, and every row that is no unit as the last member of a chain of its own — the 0
    alone in a chain of one, n behind 49 members."""
    rng = np.random.default_rng(seed)
    bad, _ = split(k, pool)
    good = [i for i in range(len(pool)) if i not in bad]
    lens = [(50, 17, 3, 2, 1, 0)[s % 6] for s in range(k.N)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    members = int(offsets[-1])
    rows = np.array([good[int(j)] for j in rng.integers(0, len(good), members)], dtype=np.uint32)
    rows[::2] = [good[(j // 2) % len(good)] for j in range(0, members, 2)]
    hosts = ([4] + [s for s in range(k.N) if lens[s] >= 1 and s != 4])[:len(bad)]
    for s, i in zip(hosts, bad):                                       # the row 0 alone in a chain of one, n behind 49 members
        rows[offsets[s + 1] - 1] = i
    assert {1, 50} <= {lens[s] for s in hosts} and set(rows.tolist()) == set(range(len(pool)))
    shift = rng.integers(0, 4, members).astype(np.int32)
    return rows, shift, offsets


def want_segprod(cts, rows, shift, offsets, M):
    out = []
    for s in range(len(offsets) - 1):
        acc = None
        for j in range(int(offsets[s]), int(offsets[s + 1])):
            v = cts[int(rows[j])]
            acc = v if acc is None else pow(acc, 1 << int(shift[j]), M) * v % M
        out.append(1 if acc is None else acc)
    return out


def test_segment_prod(ak, monkeypatch):
    """Chains of 0, 1, 2, 3, 17 and 50 members over a gather with repeats, shifts in 0..3, rows at tags 0, 1, -2 and 3: the default
    chunking, a forced chunk of 3 (more levels) and a forced chunk of 64 — one chain per segment, where 50 members at tag -2 move
    the accumulator's power of R by -3 each and cross RPOW_SPAN three times, and at tag 3 (+2 each) twice: both directions of the
    re-centring.  (The default chunk of 4 never leaves the table: only the forced long chains reach that branch.)"""
    k, nk = ak, ak.nk
    M, S, W = k.key.nsq, k.N, k.nk.cw
    pool = ciphertexts(k, k.T, 61)
    rows, shift, offsets = seg_plan(k, pool, k.b + 2)
    want = live(want_segprod(pool, rows, shift, offsets, M))
    assert want[5] == 1 and want.count(0) >= 1                         # an empty chain; the chain that ends in the row 0
    drows, dshift, doff = DevArray(rows), DevArray(shift), DevArray(offsets)
    out = DevArray(shape=(S, W))
    for tag in (0, 1, -2, 3):
        assert abs(tag + 49 * (tag - 1)) > RPOW_SPAN or tag in (0, 1)
        dct = dev(k, tagged(k, pool, tag))
        for chunk in (None, 3, 64):
            tune(monkeypatch, "segprod_chunk", chunk)
            _native.check(nk.lib.pai_ct_segment_prod(nk.pk, dct.ptr, len(pool), tag, drows.ptr, dshift.ptr, doff.ptr, S, out.ptr, None))
            path = ran(k, "segment_prod")
            assert limbs_to_ints(out.get()) == want, (k.ident, tag, chunk, path)
            assert set(path) == {"k_segprod:"} and (len(path) == 1) == (chunk == 64), (k.ident, chunk, path)
    tune(monkeypatch, "segprod_chunk", None)
    st = C.c_int(-1)
    _native.check(nk.lib.pai_pubkey_status(nk.pk, C.byref(st), 0, None))
    assert st.value == 0


# ---- pai_ct_scan ------------------------------------------------------------------------------------------------------------------
def test_scan(ak, monkeypatch):
    """seg_len in {1, 7, N}, both directions, the default chunking and scan_chunk = 3, tag in {0, 1, -2}, dom_out in {0, 1}, raise
    and step in 0..3 -> tests/test_gpu_cumsum.want_chain.  seg_len 1 scans the corner set itself (every row its own chain);
    the runs of 7 and of N are units with one row that is no unit as the last member in scan order (a different one per run,
    batch and direction).  The batches of 37 take their runs of 7 from 42 rows."""
    k, nk = ak, ak.nk
    M, N, T, W = k.key.nsq, k.N, k.T, k.nk.cw
    pool = ciphertexts(k, T, 71)
    bad, _ = split(k, pool)
    units = unit_rows(k, 72)
    cases = [(1, N, off) for off in k.offs] + [(N, N, off) for off in k.offs]
    cases += [(7, 70, 0)] if N == 70 else [(7, 42, 0), (7, 42, T - 42)]
    rng = np.random.default_rng(k.b + 3)
    for L, cnt, off in cases:
        out = DevArray(shape=(cnt, W))
        for reverse in (0, 1):
            raise_, step = rng.integers(0, 4, cnt).astype(np.int32), rng.integers(0, 4, cnt).astype(np.int32)
            if L == 1:
                arr = pool[off:off + cnt]
                for i in bad:
                    if off <= i < off + cnt:
                        raise_[i - off] = 0
            else:
                arr = units[off:off + cnt]
                runs = cnt // L
                pick = [bad[(1 + (off > 0) + 2 * reverse) % 4]] if runs == 1 else bad
                for r, i in zip(range(runs), pick):
                    pos = r * L + (0 if reverse else L - 1)
                    arr[pos], raise_[pos] = pool[i], 0
            want = live(want_chain(arr, raise_, step, L, reverse, M))
            draise, dstep = DevArray(raise_), DevArray(step)
            for tag in (0, 1, -2):
                dct = dev(k, tagged(k, arr, tag))
                for dom in (0, 1):
                    exp = [w * rpow(k, dom) % M for w in want]
                    for chunk in (None, 3):
                        tune(monkeypatch, "scan_chunk", chunk)
                        _native.check(nk.lib.pai_ct_scan(nk.pk, dct.ptr, cnt, tag, dom, L, reverse, draise.ptr, dstep.ptr, out.ptr, None))
                        path = ran(k, "scan")
                        assert limbs_to_ints(out.get()) == exp, (k.ident, L, cnt, off, reverse, tag, dom, chunk, path)
                        assert set(path) == {"k_segscan:"} and (len(path) > 1) == (L > 4 or (L > 3 and chunk == 3)), (k.ident, L, chunk, path)
    tune(monkeypatch, "scan_chunk", None)
    st = C.c_int(-1)
    _native.check(nk.lib.pai_pubkey_status(nk.pk, C.byref(st), 0, None))
    assert st.value == 0


# ---- pai_ct_sparse_multiexp -------------------------------------------------------------------------------------------------------
def test_sparse_multiexp(ak, monkeypatch):
    """12 bases (the six corner units 1, 2, n - 1, n + 1, M - 1, M - 2 and six grid cells) with their CPython inverses, about 160
    terms in k.N segments of 0..9 terms, 53-bit exponents with 0, 1, 2^52 and 2^53 - 1, mixed signs and the unsigned form, the
    default window and mexp_wbits = 2, the default lanes (a chunk per term: the combine levels) and mexp_lanes = 50 (chunks of
    several terms that cut the long segments).  Keys the digit engine serves run again on a handle created with
    PAI_DISABLE=padic, so both k_smexp forms see them."""
    k = ak
    M, S, W = k.key.nsq, k.N, k.nk.cw
    u = unit_rows(k, 81)
    assert u[:6] == [1, 2, k.key.n - 1, k.key.n + 1, M - 1, M - 2]
    base = u[:6] + u[6:60:9]
    inv = [pow(x, -1, M) for x in base]
    assert len(base) == 12
    rng = random.Random(k.b + 4)
    cyc = (0, 1, 2, 3, 9, 5, 1, 0, 2, 0) if S == 70 else (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
    lens = [cyc[s % 10] for s in range(S)]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(offsets[-1])
    assert 140 <= T <= 180
    bidx = [(5 * t + t // 12) % 12 for t in range(T)]
    e = [rng.getrandbits(53) for _ in range(T)]
    e[3], e[4], e[5], e[6] = 0, 1, 1 << 52, (1 << 53) - 1
    e[T - 1] = (1 << 53) - 1
    sign = [(t * 7 // 3) % 2 for t in range(T)]
    assert 0 < sum(sign) < T
    pw = {True: pow_many([inv[b] if s else base[b] for b, s in zip(bidx, sign)], e, M), False: pow_many([base[b] for b in bidx], e, M)}
    want = {}
    for signed in (True, False):
        want[signed] = []
        for s in range(S):
            acc = 1
            for t in range(int(offsets[s]), int(offsets[s + 1])):
                acc = acc * pw[signed][t] % M
            want[signed].append(acc)
        live(want[signed])
    dbase, dinv = dev(k, base), dev(k, inv)
    didx, de = DevArray(np.array(bidx, dtype=np.int32)), DevArray(ints_to_limbs(e, 2))
    dsign, doff = DevArray(np.array(sign, dtype=np.uint8)), DevArray(offsets)
    out = DevArray(shape=(S, W))
    handles = [("default", k.nk)]
    if k.digit:
        knob_disable(monkeypatch, "padic")
        handles.append(("PAI_DISABLE=padic", NativeKey(k.key)))
        knob_disable(monkeypatch, "padic", False)
    else:
        HANDDOWN.add((k.ident, "sparse_multiexp", "lane groups only: the digit engine does not serve n"))
    for label, nk in handles:
        for signed, wbits, lanes in ((True, None, None), (True, 2, 50), (False, None, 50), (False, 2, None)):
            tune(monkeypatch, "mexp_wbits", wbits)
            tune(monkeypatch, "mexp_lanes", lanes)
            _native.check(nk.lib.pai_ct_sparse_multiexp(nk.pk, dbase.ptr, dinv.ptr if signed else None, 12, didx.ptr, de.ptr, 2, 53,
                                                        dsign.ptr if signed else None, T, doff.ptr, S, out.ptr, None))
            path = ran(k, f"sparse_multiexp({'digit pairs' if k.digit and label == 'default' else 'lane groups'})")
            assert limbs_to_ints(out.get()) == want[signed], (k.ident, label, signed, wbits, lanes, path)
            assert path[:2] == ["k_mexp_table:", "k_smexp:"] and set(path[2:]) == {"k_segprod:"}, (k.ident, path)
        st = C.c_int(-1)
        _native.check(nk.lib.pai_pubkey_status(nk.pk, C.byref(st), 0, None))
        assert st.value == 0


# ---- pai_ct_pack, pai_ct_pack_step ------------------------------------------------------------------------------------------------
def pack_edges(nk):
    cnt = C.c_int(0)
    buf = (C.c_size_t * 8)()
    _native.check(nk.lib.pai_path_edges(nk.pk, 4, buf, 8, C.byref(cnt)))
    return [int(buf[i]) for i in range(min(cnt.value, 8))]


def test_pack_and_pack_step(ak, monkeypatch):
    """pai_ct_pack with 64-bit slots, the largest slot count the key allows capped at 8, and pai_ct_pack_step with 4 rows at steps of
    128 bits: k.N chains, the last one ragged, at tag 0 on both sides of the hand-over (the edge moved onto the batch with
    pack_padic_min and read back through pai_path_edges, as tests/test_gpu_packed.py does) and at tag 1 -> want_packed /
    want_stepped.  A chain joins its rows from the last to the first, so the rows that are no units are row 0 of the first chains."""
    k, nk = ak, ak.nk
    M, G, W = k.key.nsq, k.N, k.nk.cw
    nb = k.key.n.bit_length()
    pool = ciphertexts(k, k.T, 91)
    bad, units = split(k, pool)
    units += unit_rows(k, 92)
    for name, step, count in (("pack", 64, min(8, (nb - 2) // 64)), ("pack_step", 128, 4)):
        assert count * step <= nb - 2 and count >= 4
        rows_n = (G - 1) * count + count - 2                           # a ragged last chain
        arr = [units[(i + 3 * (i // len(units))) % len(units)] for i in range(rows_n)]
        for g, i in enumerate(bad):
            arr[g * count] = pool[i]
        want = live(want_packed(arr, step, count, M) if name == "pack" else want_stepped(arr, step, count, M))
        assert len(want) == G
        out = DevArray(shape=(G, W))
        for tag, min_rows in ((0, G + 1), (0, G), (1, G)):
            tune(monkeypatch, "pack_padic_min", min_rows)
            edge = pack_edges(nk)
            assert edge == [min_rows - 1] and (G <= edge[0]) == (min_rows == G + 1)      # G = E below the hand-over, G = E + 1 above
            dct = dev(k, tagged(k, arr, tag))
            if name == "pack":
                _native.check(nk.lib.pai_ct_pack(nk.pk, dct.ptr, rows_n, tag, step, count, out.ptr, None))
            else:
                _native.check(nk.lib.pai_ct_pack_step(nk.pk, dct.ptr, rows_n, tag, step, count, out.ptr, None))
            path = ran(k, name)
            assert limbs_to_ints(out.get()) == want, (k.ident, name, tag, min_rows, path)
            if min_rows == G and tag == 0 and k.digit:
                assert path == ["k_mexp_table:", "k_ct_pack_padic:"], (k.ident, name, path)
            else:
                assert set(path) == {"k_segprod:"}, (k.ident, name, tag, min_rows, path)
                if min_rows == G:
                    HANDDOWN.add((k.ident, name, "k_segprod above the hand-over: " + ("tagged rows" if tag else "the digit engine does not serve n")))
    tune(monkeypatch, "pack_padic_min", None)


# ---- what the structured keys already get, on the limit keys ---------------------------------------------------------------------
@limit_only
def test_limit_ct_add_family(ak, monkeypatch):
    """tests/test_gpu_extreme_keys.py::test_ct_add_family on the limit keys: pai_ct_add (no limit key has the context of the
    most-significant-limb-first product: asserted), the Montgomery products on lane groups and on the latency geometry — where
    the latency limit keys have R/M just above 4 —, pai_ct_mont_mul, pai_ct_add_aligned and pai_ct_pow2."""
    monkeypatch.setattr(xkeys, "SEEN", XSEEN)
    xkeys.test_ct_add_family(ak, monkeypatch)
    assert XSEEN[("msb_context", ak.b)] >= {f"{ak.family}=False"}, "a limit key with the msb-first context: not the documented hand-down"
    HANDDOWN.add((ak.ident, "ct_add", "k_modmul: no most-significant-limb-first context"))
    for (op, b), names in XSEEN.items():
        if b == ak.b and op != "msb_context":
            COV.setdefault((op, ak.NL), set()).update(names)


@limit_only
def test_limit_invert_prod_multiexp(ak, monkeypatch):
    """tests/test_gpu_extreme_keys.py::test_invert_prod_multiexp on the limit keys: the single-product trees of pai_ct_invert and
    pai_ct_prod, and pai_ct_multiexp."""
    monkeypatch.setattr(xkeys, "SEEN", XSEEN)
    xkeys.test_invert_prod_multiexp(ak)


@limit_only
def test_limit_fallback_engines(ak, monkeypatch):
    """tests/test_gpu_extreme_keys.py::test_fallback_engines on the limit keys: DJN encryption, ct * pt and decryption on the
    lane-group kernels."""
    monkeypatch.setattr(xkeys, "SEEN", XSEEN)
    xkeys.test_fallback_engines(ak, monkeypatch)
    for (op, b), names in XSEEN.items():
        if b == ak.b and op != "msb_context":
            COV.setdefault((op, ak.NL), set()).update(names)


def test_chain_kernels_ran_at_every_limit():
    """What ran, per operation and lane-group geometry (printed: the record of the coverage), the hand-downs, and k_addn, k_segprod
    and k_segscan on every lane-group geometry at a limit key of that geometry and on every latency limit key.  Holds when the whole
    file ran; a selection of keys only prints."""
    for (op, nl), names in sorted(COV.items()):
        print(f"COVERAGE {op} NL={nl}: {' '.join(sorted(names))}")
    for (kern, engine, nl), host in sorted(LIMIT_RAN.items()):
        print(f"COVERAGE limit {engine} NL={nl}: {kern} on {host} limbs")
    for item in sorted(HANDDOWN):
        print("HANDDOWN " + " | ".join(item))
    if VISITED != set(IDS):
        print(f"COVERAGE not asserted: {len(VISITED)} of {len(IDS)} keys ran")
        return
    for kern in ("k_addn", "k_segprod", "k_segscan"):
        for nl in LANE_GROUP_NL:
            assert LIMIT_RAN.get((kern, "lane_group", nl)) == nl, (kern, nl)
        for nl in LATENCY_NL:
            assert LIMIT_RAN.get((kern, "latency", nl), 0) > nl, (kern, nl)
