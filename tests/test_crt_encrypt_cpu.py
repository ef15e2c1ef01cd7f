"""CPU: the Python-int model of the owner-side CRT encryption (tools/crt_encrypt_model.py: hs mod s^2, the two half
exponentiations, the Garner lift with p^-2 mod q^2, the message factor) against the oracle's public encryption, over every
fixture key and every extreme-structure key.  Pins the formulas and constants the kernels of csrc/dispatch_encrypt_crt.hpp use."""
import json
import random
import sys
from pathlib import Path

import pytest

from oracle import paillier_oracle as orc

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import crt_encrypt_model as model  # noqa: E402

DJN_X = 0xABCDEF1234567


def _keys():
    fx = json.loads((ROOT / "tests" / "golden" / "fixture_keys.json").read_text())
    out = [(f"fixture-{b}", int(v["p"], 16), int(v["q"], 16)) for b, v in sorted(fx.items(), key=lambda kv: int(kv[0]))]
    ex = json.loads((ROOT / "tests" / "golden" / "extreme_keys.json").read_text())
    out += [(f"{e['family']}-{e['prime_bits']}", int(e["p"], 16), int(e["q"], 16)) for e in ex]
    return out


KEYS = _keys()


@pytest.mark.parametrize("ident,p,q", KEYS, ids=[k[0] for k in KEYS])
def test_model_matches_oracle(ident, p, q):
    key = orc.make_key(p, q, djn_x=DJN_X, bits=(p * q).bit_length())
    rng = random.Random(ident)
    n, nsq = key.n, key.nsq
    c = model.constants(p, q, key.hs)
    assert c["p"] < c["q"] and c["pinv2"] == pow(c["p2"], -1, c["q2"])
    assert c["hs_p"] == key.hs % c["p2"] and c["hs_q"] == key.hs % c["q2"]
    ms = [0, 1, n - 1, c["p"], c["q"], 2 * c["p"], rng.randrange(n)]
    rs = [0, 1, (1 << key.randbits) - 1, rng.getrandbits(key.randbits)]
    # the obfuscators once per r (the half exponentiations dominate), then every m
    for r in rs:
        o = model.obfuscator(c, r)
        assert o == orc.obfuscator_djn(key.hs, r, nsq)
        for m in ms:
            want = orc.encrypt(key, m, r)
            assert (1 + m * n) % nsq * o % nsq == want
            fp, fq = model.fold(c, m, n)
            assert 0 <= fp < c["p"] and 0 <= fq < c["q"]
    assert model.encrypt(p, q, key.hs, ms[-1], rs[1]) == orc.encrypt(key, ms[-1], rs[1])
    assert model.apply_obfuscator(p, q, key.hs, 12345, rs[1]) == orc.apply_obfuscator(key, 12345, rs[1])
    assert model.lift(c, 1, 1) == 1                              # m = 0, r = 0: c_q - c_p = 0


def test_served_key_sizes():
    # both primes on one instantiation of the encryption digit engine (36 / 72 limbs), q^2 on a lane-group geometry with a lift kernel
    assert [model.enc_nl(b) for b in (256, 699, 700, 768, 1024, 1025, 1399, 1400, 1536, 2048, 2064, 2068, 2069)] == \
        [0, 0, 36, 36, 36, 0, 0, 72, 72, 72, 72, 72, 0]
    assert [model.lift_nl(2 * b) for b in (700, 768, 1024, 1400, 1536, 1604, 2048, 2064, 2068)] == [72, 72, 72, 112, 112, 112, 144, 144, 144]
