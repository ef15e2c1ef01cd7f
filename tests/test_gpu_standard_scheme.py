"""GPU: the standard scheme (enable_DJN=False, obfuscator r^n mod n^2) on the 27 structured keys of tests/golden/extreme_keys.json
and the 15 limit keys of tests/golden/limit_keys.json, both power routes of csrc/dispatch_encrypt.hpp: encrypt_common, bit-exact
against CPython integers (bulk powers through tests/_util.pow_many, the C oracle spot-checked against CPython's pow at every call).

  * k_pow_padic runs a host-compiled sliding-window schedule of n on the base-n digit engine, for the keys that engine accepts
    (n of 700 .. 1024 and 1400 .. 2068 bits).  Its "no multiplication" entries are runs of more than 255 squarings: they occur for
    the `ones`, `zeros`, `ones_zeros` and `half` keys at 512- and 1024-bit primes, whose n has a zero run of 330 to 1012 bits
    (tests/test_codec_keys_cpu.py holds that property of the fixture).
  * lane-group modexp_fixed serves every other key — rows n_words wide going in, ct_words wide coming out, an exponent of bits(n)
    bits — and, on a handle created with PAI_DISABLE=padic, the digit-served keys as well.
k_encrypt mode 3 (pai_encrypt) or mode 4 (pai_obfuscate) multiplies the power in.  Which power kernel ran is read back
(pai_profile_last / pai_profile_last_path); the last test requires k_pow(r^n):padic at a 1024-bit and a 2048-bit n and
k_pow(r^n):lane_group on every key.

r holds 1, 2, n - 1, n - 2, p, q, n - p, 2^(bits(n) - 1), 2^(bits(n) - 1) - 1 and a pattern tail.  p, q and n - p are deliberate: the
call is arithmetic, and r^n of a non-unit is defined; only decryption leaves those rows out."""
import math

import numpy as np
import pytest
import torch

from oracle import paillier_oracle as orc
from pailliercryptolib_python_amd import _native
from tests import test_gpu_extreme_keys as xkeys
from tests._util import DevArray, ints_to_limbs, limbs_to_ints, pow_many
from tests._util import disable as knob_disable
from tests.test_extreme_keys_cpu import load_extreme_keys
from tests.test_gpu_extreme_keys import Key, ciphertexts, pattern, plain, ran
from tests.test_gpu_paillier_abi import NativeKey, _last_kernels, bench_key
from tests.test_limit_keys_cpu import load_limit_keys

pytestmark = pytest.mark.gpu

ALL_KEYS = [(e[0], e[1], e[4], e[5], e[6]) for e in load_limit_keys()] + list(load_extreme_keys())
IDS = [e[0] for e in ALL_KEYS]
SEEN = {}                            # ("r^n", prime bits) -> {"kernel:path"}
ROUTES = {}                          # key id -> {"padic", "lane_group"}
VISITED = set()


def digit_served(n_bits):
    """csrc/padic_enc_kernels.hip: padic_enc_nl_for_n_bits"""
    return 700 <= n_bits <= 1024 or 1400 <= n_bits <= 2068


def longest_zero_run(n):
    return max(len(run) for run in bin(n)[2:].split("1"))


def standard_inputs(key, N, seed):
    """(m, r): the plaintext corners of test_gpu_extreme_keys.plain and the obfuscator bases of the module docstring"""
    n, nb = key.n, key.n.bit_length()
    r = [1, 2, n - 1, n - 2, key.p, key.q, n - key.p, 1 << (nb - 1), (1 << (nb - 1)) - 1] + pattern(n, N, seed)
    return [x or 1 for x in r[:N]]


class StdKey(Key):
    """test_gpu_extreme_keys.Key with the standard-scheme key of the same primes (no hs)"""

    def __init__(self, ident, family, b, p, q):
        self.ident, self.family, self.b = ident, family, b
        self.key = orc.make_key(p, q, djn_x=None, bits=2 * b)
        self.nk = NativeKey(self.key)
        self.N = 70 if 2 * b < 4000 else 37
        self.consts = orc.crt_constants(self.key)


@pytest.fixture(scope="module", params=ALL_KEYS, ids=IDS)
def sk(request):
    _native.check(_native.load().pai_profile_enable(1))
    k = StdKey(*request.param)
    VISITED.add(k.ident)
    yield k
    _native.check(k.nk.lib.pai_profile_enable(0))


def test_standard_scheme_both_routes(sk, monkeypatch):
    """pai_encrypt -> (1 + m n) r^n, pai_obfuscate -> ct r^n, pai_decrypt of the encryptions -> m (rows whose r is a unit), on the
    handle as created and, where the digit engine serves the key, on a handle created with PAI_DISABLE=padic."""
    monkeypatch.setattr(xkeys, "SEEN", SEEN)
    k, key, N = sk, sk.key, sk.N
    n, M = key.n, key.nsq
    m, r = plain(k, N, 41), standard_inputs(key, N, 42)
    assert r[:9] == [1, 2, n - 1, n - 2, key.p, key.q, n - key.p, 1 << (n.bit_length() - 1), (1 << (n.bit_length() - 1)) - 1]
    cts = ciphertexts(k, N, 43)
    obf = pow_many(r, n, M)
    want = [(1 + x * n) % M * o % M for x, o in zip(m, obf)]
    assert want[1] == orc.encrypt(key, m[1], r[1])
    want_obf = [c * o % M for c, o in zip(cts, obf)]
    assert want_obf[12] == orc.apply_obfuscator(key, cts[12], r[12])
    units = [i for i in range(N) if math.gcd(r[i], n) == 1]
    assert len(units) == N - 3
    digit = digit_served(n.bit_length())
    handles = [("default", k.nk, "padic" if digit else "lane_group")]
    if digit:
        knob_disable(monkeypatch, "padic")
        handles.append(("PAI_DISABLE=padic", NativeKey(key), "lane_group"))
        knob_disable(monkeypatch, "padic", False)
    for label, nk, route in handles:
        dm, dr = DevArray(ints_to_limbs(m, nk.nw)), DevArray(ints_to_limbs(r, nk.nw))
        ct = DevArray(shape=(N, nk.cw))
        _native.check(nk.lib.pai_encrypt(nk.pk, dm.ptr, dr.ptr, N, ct.ptr, None))
        path = ran(k, "r^n")
        got = limbs_to_ints(ct.get())
        assert got == want, (k.ident, label, path, [i for i in range(N) if got[i] != want[i]])
        assert path == [f"k_pow(r^n):{route}"], (k.ident, label, path)
        dc = DevArray(ints_to_limbs(cts, nk.cw))
        _native.check(nk.lib.pai_obfuscate(nk.pk, dc.ptr, dr.ptr, N, None))
        path = ran(k, "r^n")
        got = limbs_to_ints(dc.get())
        assert got == want_obf, (k.ident, label, path, [i for i in range(N) if got[i] != want_obf[i]])
        assert path == [f"k_pow(r^n):{route}"], (k.ident, label, path)
        ROUTES.setdefault(k.ident, set()).add(route)
    du = DevArray(ints_to_limbs([want[i] for i in units], k.nk.cw))
    out = DevArray(shape=(len(units), k.nk.nw))
    _native.check(k.nk.lib.pai_decrypt(k.nk.sk, du.ptr, len(units), out.ptr, None))
    assert limbs_to_ints(out.get()) == [m[i] for i in units], k.ident


def test_pow_padic_more_tiles_than_workgroups(monkeypatch):
    """k_pow_padic launches at most one workgroup per CU over 256-element tiles: 256 CU + 77 elements make every workgroup's tile
    loop run again (workgroup 0 twice more) and end ragged.  The whole batch equals the lane-group route's; the oracle holds rows
    0-63 (the corner bases and plaintexts), 255, 256, 256 CU - 1, 256 CU, N - 2 and N - 1."""
    monkeypatch.setattr(xkeys, "SEEN", SEEN)
    key = bench_key(djn=False)
    nk = NativeKey(key)
    knob_disable(monkeypatch, "padic")
    nk_lg = NativeKey(key)
    knob_disable(monkeypatch, "padic", False)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    N = 256 * cu + 77
    n, M, nw = key.n, key.nsq, nk.nw
    rng = np.random.default_rng(cu)
    m_l, r_l = (rng.integers(0, 1 << 32, (N, nw), dtype=np.uint32) for _ in range(2))
    m_l[:, -1] = 0                                       # below 2^(32 (nw - 1)) < n
    r_l[:, -1] = 0
    r_l[:, 0] |= 1                                       # never 0
    sample = list(range(64)) + [255, 256, 256 * cu - 1, 256 * cu, N - 2, N - 1]
    head = ints_to_limbs(standard_inputs(key, 64, 52), nw)
    r_l[:64] = head
    r_l[N - 2:] = head[2:4]                               # n - 1, n - 2 in the ragged tile
    m_l[:64] = ints_to_limbs(([0, 1, n - 1, key.p, key.q, n - key.p, n - key.q] + pattern(n, 64, 51))[:64], nw)
    m, r = limbs_to_ints(m_l[sample]), limbs_to_ints(r_l[sample])
    want = [(1 + x * n) % M * o % M for x, o in zip(m, pow_many(r, n, M))]
    dm, dr = DevArray(m_l), DevArray(r_l)
    got = {}
    lib = nk.lib
    _native.check(lib.pai_profile_enable(1))
    try:
        for h, route in ((nk, "padic"), (nk_lg, "lane_group")):
            ct = DevArray(shape=(N, h.cw))
            _native.check(h.lib.pai_encrypt(h.pk, dm.ptr, dr.ptr, N, ct.ptr, None))
            names = _last_kernels(lib)
            assert names == ["k_pow(r^n)"], names
            got[route] = ct.get()
            ct.free()
    finally:
        _native.check(lib.pai_profile_enable(0))
    diff = np.nonzero((got["padic"] != got["lane_group"]).any(axis=1))[0]
    assert diff.size == 0, (N, diff[:10].tolist())
    assert limbs_to_ints(got["padic"][sample]) == want


def test_both_power_routes_ran():
    """What ran per prime width (printed), k_pow(r^n):padic at a 1024-bit and a 2048-bit n and k_pow(r^n):lane_group on every key.
    Holds when the whole file ran; a selection of keys only prints."""
    for (op, b), names in sorted(SEEN.items()):
        print(f"COVERAGE {op} prime_bits={b}: {' '.join(sorted(names))}")
    if VISITED != set(IDS):
        print(f"COVERAGE not asserted: {len(VISITED)} of {len(IDS)} keys ran")
        return
    assert len(VISITED) == 42
    n_bits = {e[0]: (e[3] * e[4]).bit_length() for e in ALL_KEYS}
    for want_bits in (1024, 2048):
        assert any("padic" in ROUTES[i] for i in IDS if n_bits[i] == want_bits), want_bits
    assert all("lane_group" in ROUTES[i] for i in IDS), [i for i in IDS if "lane_group" not in ROUTES.get(i, ())]
