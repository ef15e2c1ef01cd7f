"""CPU: the generators and models of the differential fuzz for the extension entry points (tests/_fuzz_ext.py), without a device.

  * determinism: case() is a function of its arguments;
  * models: every family's expectation against an independent restatement of the header's definition — plain loops with pow,
    closed forms where the model is a recurrence — on a toy key of 96 bits, rounds 0 .. 11 (clean and dirty);
  * coverage: the schedule of tests/test_gpu_fuzz_ext.py (SEED, ROUNDS, the real keys of every class) contains every shape class
    and knob value, each asserted by name.  Shapes do not depend on the powers, so the schedule is generated with the bulk powers
    stubbed out (the generator draws the same numbers); the real keys are needed because units are chosen by gcd with n;
  * not vacuous: conditions on the expected outputs alone, on the toy key and on the 1024-bit fixture key."""
import math

import numpy as np
import pytest

from oracle import paillier_oracle as orc
from tests import _fuzz_ext as fz
from tests._fuzz_ext_run import oracle_key

TOY_ROUNDS = range(12)


def toy_key():
    p, q = 0, 0
    c = (1 << 47) + 3
    found = []
    while len(found) < 2:
        if c % 4 == 3 and orc.is_probable_prime(c):
            found.append(c)
            c += 1 << 20
        c += 2
    p, q = found
    key = orc.make_key(p, q, djn_x=12345, bits=96)
    assert key.n.bit_length() in (95, 96) and math.gcd(key.n, (p - 1) * (q - 1)) == 1
    return key


TOY = toy_key()


def plain(v):
    if isinstance(v, np.ndarray):
        return ("ndarray", str(v.dtype), v.tolist())
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, set):
        return sorted(v)
    return v


@pytest.mark.parametrize("family", fz.FAMILIES)
def test_case_is_a_function_of_its_arguments(family):
    for rnd in (0, 1, 3):
        a, b = fz.case(family, TOY, 7, rnd), fz.case(family, TOY, 7, rnd)
        assert plain(a) == plain(b)
        assert plain(a) != plain(fz.case(family, TOY, 8, rnd))
        assert plain(a) != plain(fz.case(family, TOY, 7, rnd + 4))
        assert a["family"] == family and a["bits"] == TOY.bits and a["round"] == rnd and a["runs"]


# ---- the models against restatements -----------------------------------------------------------------------------------------------
def test_model_segprod():
    M = TOY.nsq
    for rnd in TOY_ROUNDS:
        c = fz.case("segprod", TOY, 3, rnd)
        off = c["offsets"]
        for s in range(c["S"]):
            mem = []
            for j in range(int(off[s]), int(off[s + 1])):                      # the members that count, with their shifts
                r = j if c["rows"] is None else int(c["rows"][j])
                if r < c["N"]:
                    mem.append((r, 0 if c["shift"] is None else max(0, int(c["shift"][j]))))
            want = 1
            for a, (r, _) in enumerate(mem):                                   # closed form: every later shift squares member a
                want = want * pow(c["cts"][r], 1 << sum(sh for _, sh in mem[a + 1:]), M) % M
            assert c["want"][s] == want, (rnd, s)
        assert c["dirty"] == (rnd % 8 == 1) and [r["tune"]["segprod_chunk"] for r in c["runs"]] == list(fz.SEGPROD_CHUNKS)
        if c["dirty"]:
            assert (c["rows"] >= c["N"]).any() and (c["shift"] < 0).any() and c["status_bit"] == 4
        firsts = [int(off[s]) for s in range(c["S"]) if off[s + 1] > off[s]]
        if c["shift"] is not None:                                             # negative values: only where the case says so
            inner = np.delete(c["shift"], firsts)
            assert (c["shift"][firsts] < 0).any() == c["first_negative"] and (inner < 0).any() == c["dirty"]
            assert (np.abs(c["shift"][firsts]) >= 7).all()                     # garbage on every first shift
        assert c["status_bit"] == (4 if c["first_negative"] else 0) and c["first_negative"] == (c["dirty"] or rnd % 4 == 2)


def test_model_scan():
    M = TOY.nsq
    for rnd in TOY_ROUNDS:
        c = fz.case("scan", TOY, 3, rnd)
        L, N = c["seg_len"], c["N"]
        rz = [0] * N if c["raise"] is None else [max(0, int(v)) for v in c["raise"]]
        st = [0] * N if c["step"] is None else [max(0, int(v)) for v in c["step"]]
        for base in range(0, N, L):
            order = [base + (L - 1 - p if c["reverse"] else p) for p in range(L)]
            for a, i in enumerate(order):
                want = 1
                for b in range(a + 1):                                          # closed form over the prefix in scan order
                    j = order[b]
                    want = want * pow(c["cts"][j], 1 << (rz[j] + sum(st[order[k]] for k in range(b + 1, a + 1))), M) % M
                assert c["want"][i] == want, (rnd, i)
        if c["dirty"]:
            assert (c["raise"] < 0).any() and c["status_bit"] == 16
        if c["first_negative"]:
            assert c["step"][L - 1 if c["reverse"] else 0] < 0                 # the first step of the first run
        elif c["step"] is not None:
            assert (c["step"] >= 0).all() and (c["raise"] is None or (c["raise"] >= 0).all())
        assert c["status_bit"] == (16 if c["first_negative"] else 0) and c["first_negative"] == (c["dirty"] or rnd % 4 == 2)


def test_model_smexp():
    M = TOY.nsq
    for rnd in TOY_ROUNDS:
        c = fz.case("smexp", TOY, 3, rnd)
        T, off = c["T"], [int(v) for v in c["offsets"]]
        clean = [max(min(max(v, 0), T) for v in off[:s + 1]) for s in range(len(off))]
        for s in range(c["S"]):
            want = 1
            for t in range(clean[s], clean[s + 1]):
                b = int(c["bidx"][t])
                if 0 <= b < c["N"]:
                    x = c["inv"][b] if c["sign"] is not None and c["sign"][t] else c["base"][b]
                    want = want * pow(x, c["e"][t], M) % M
            assert c["want"][s] == want, (rnd, s)
        if c["inv"] is not None:
            assert all(x * y % M == 1 for x, y in zip(c["base"], c["inv"]))
        assert all(e < 1 << c["ebits"] for e in c["e"]) and (1 << c["ebits"]) - 1 in c["e"]
        if c["dirty"]:
            assert clean != off and ((c["bidx"] < 0) | (c["bidx"] >= c["N"])).any() and c["status_bit"] == 8
        else:
            assert clean == off


def test_model_pack():
    M, nb = TOY.nsq, TOY.n.bit_length()
    for rnd in TOY_ROUNDS:
        c = fz.case("pack", TOY, 3, rnd)
        for rows, step, count, want in ((c["cts"][:c["N"]], c["slot_bits"], c["slots"], c["want"]),
                                        (c["cts"][:c["N_step"]], c["step_bits"], c["count"], c["want_step"])):
            assert 8 <= step <= 128 and count >= 1 and count * step <= nb - 2
            assert len(want) == -(-len(rows) // count)
            for g in range(len(want)):
                acc = 1
                for j, v in enumerate(rows[g * count:(g + 1) * count]):
                    acc = acc * pow(v, 1 << (step * j), M) % M
                assert want[g] == acc, (rnd, g)


def test_model_open():
    n, M, p, q = TOY.n, TOY.nsq, TOY.p, TOY.q
    for rnd in TOY_ROUNDS:
        c = fz.case("open", TOY, 3, rnd)
        for i, (ct, r) in enumerate(zip(c["cts"], c["want_r"])):
            if i == c["bad_row"]:
                assert ct % p == 0 and r % p == 0 and pow(r, n, q) == ct % q and 0 <= r < n     # r_p = 0, the q side opens
            else:
                assert math.gcd(r, n) == 1 and ct == (1 + orc.decrypt_crt(TOY, ct) * n) * pow(r, n, M) % M
        L, unit = c["seg_len"], True
        for s, s0 in enumerate(range(0, c["N"], L)):
            A, B, Ms = 1, 1, 0
            for i in range(s0, min(s0 + L, c["N"])):
                A = A * pow(c["fold_ct"][i], c["e"][i], M) % M
                B = B * pow(c["fold_r"][i], c["e"][i], n) % n
                Ms = (Ms + c["e"][i] * c["fold_m"][i]) % n
            assert c["want_lhs"][s] == A and c["want_rhs"][s] == (1 + n * Ms) * pow(B, n, M) % M, (rnd, s)
            unit = unit and math.gcd(B, n) == 1
            hit = c["falsified"] is not None and s0 <= c["falsified"] < s0 + L
            bad = s0 <= c["bad_row"] < s0 + L and "bad_row_kept" in c["shape"]
            if unit and not bad:
                assert (A != c["want_rhs"][s]) == hit, (rnd, s)                # a falsified opening, and only that, breaks its segment
        assert c["want_flag"] == int(not unit)
        assert 1 <= c["e_words"] <= 8 and 0 < c["ebits"] <= 32 * c["e_words"]


def test_model_crtenc():
    for rnd in TOY_ROUNDS:
        c = fz.case("crtenc", TOY, 3, rnd)
        assert c["want_enc"] == [orc.encrypt(TOY, m, r) for m, r in zip(c["m"], c["r"])]
        assert c["want_obf"] == [orc.apply_obfuscator(TOY, x, r) for x, r in zip(c["cts"], c["r"])]
        assert all(r < 1 << TOY.randbits for r in c["r"]) and all(m < TOY.n for m in c["m"]) and not c["served"]


def test_model_tpart():
    for rnd in TOY_ROUNDS:
        c = fz.case("tpart", TOY, 3, rnd)
        for E, want in zip(c["E"], c["want"]):
            assert E > 0 and want == [pow(x, E, TOY.nsq) for x in c["cts"]]


def test_model_tcomb():
    """the (1 + alpha n) identity of the generator against the direct definition: x = prod parts^(+-mu) mod n^2,
    m = ((x - 1) // n) theta mod n, on every row"""
    for rnd in range(16):
        c = fz.case("tcomb", TOY, 3, rnd)
        direct = fz.model_tcomb_direct(TOY, c["parts"], c["mu"], c["neg"], c["theta"], range(c["N"]))
        for i in range(c["N"]):
            x = 1
            for j in range(c["t"]):
                b = pow(c["parts"][j][i], -1, TOY.nsq) if c["neg"][j] else c["parts"][j][i]
                x = x * pow(b, c["mu"][j], TOY.nsq) % TOY.nsq
            assert direct[i] == (x % TOY.n != 1, (x - 1) // TOY.n * c["theta"] % TOY.n)
            assert c["want_rowflag"][i] == int(direct[i][0]), (rnd, i)
            if not direct[i][0]:
                assert c["want"][i] == direct[i][1], (rnd, i)
            if i not in c["corrupt"]:
                assert not direct[i][0]
        assert all(0 < v < 1 << 128 for v in c["mu"]) and 1 <= c["mu_words"] <= 4 and max(c["mu"]) < 1 << (32 * c["mu_words"])
        assert 4 * sum(c["want_rowflag"]) <= max(c["N"], 4) and c["N"] >= 4 and len(c["corrupt"]) >= 1
        if c["poison"] is not None:
            j, i, v = c["poison"]
            assert c["neg"][j] and math.gcd(v, TOY.n) != 1


# ---- not vacuous ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", (TOY, None), ids=("toy", "fixture-1024"))
def test_expectations_are_not_vacuous(key):
    key = key or oracle_key(1024)
    for rnd in range(16 if key is TOY else 6):
        for family in ("segprod", "smexp"):
            c = fz.case(family, key, fz.SEED, rnd)
            want = c["want"]
            if not c["dirty"]:
                lens = np.diff(c["offsets"])
                assert 8 * int((lens == 0).sum()) <= max(len(lens), 8), (family, rnd)
                assert all(want[s] == 1 for s in np.flatnonzero(lens == 0))
            assert 0 not in want, (family, rnd)
            if family == "segprod" and c["planted_non_unit"] is not None:
                assert c["S"] >= 16 and math.gcd(want[c["planted_non_unit"]], key.n) != 1
                assert sum(1 for w in want if math.gcd(w, key.n) != 1) == 1
            else:
                assert all(math.gcd(w, key.n) == 1 for w in want), (family, rnd)
        for family, names in (("scan", ("want",)), ("pack", ("want", "want_step")), ("crtenc", ("want_enc", "want_obf"))):
            c = fz.case(family, key, fz.SEED, rnd)
            for name in names:
                assert all(math.gcd(w, key.n) == 1 for w in c[name]), (family, rnd)
        c = fz.case("tpart", key, fz.SEED, rnd)
        assert all(math.gcd(w, key.n) == 1 for want in c["want"] for w in want)
        c = fz.case("open", key, fz.SEED, rnd)
        assert 0 not in c["want_lhs"] and 0 not in c["want_rhs"] and 0 not in c["want_r"]
        c = fz.case("tcomb", key, fz.SEED, rnd)
        assert 4 * sum(c["want_rowflag"]) <= max(c["N"], 4)


# ---- the schedule of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def schedule():
    """{(family, class): [cases]} for the seed and the round counts of tests/test_gpu_fuzz_ext.py, the bulk powers stubbed out"""
    mp = pytest.MonkeyPatch()
    mp.setattr(fz, "pow_many", lambda bases, exps, M, check=3: [1] * len(bases))
    mp.setattr(fz, "djn_encrypt_many", lambda key, ms, rs: [1] * len(ms))
    mp.setattr(fz, "djn_obfuscate_many", lambda key, cts, rs: [1] * len(cts))
    mp.setattr(fz, "model_tcomb_direct", lambda key, parts, mu, negs, theta, rows: {i: (True, 0) for i in rows})
    mp.setattr(fz, "model_recover", lambda key, c: 0)
    mp.setattr(fz, "model_segprod", lambda *a: [])
    mp.setattr(fz, "model_scan", lambda *a: [])
    try:
        keys = {bits: oracle_key(bits) for sizes in fz.KEY_CLASSES.values() for bits in sizes}
        yield {(family, cls): [fz.case(family, keys[fz.key_bits_for(cls, rnd)], fz.SEED, rnd) for rnd in range(fz.rounds_for(family, cls))]
               for family in fz.FAMILIES for cls in fz.KEY_CLASSES}
    finally:
        mp.undo()


def shapes(cases):
    out = set()
    for c in cases:
        out |= c["shape"]
    return out


def knob_values(cases, name):
    return {run["tune"].get(name) for c in cases for run in c["runs"]}


CLASSES = list(fz.KEY_CLASSES)


def test_schedule_is_round_counted(schedule):
    assert len(schedule) == 32
    for (family, cls), cases in schedule.items():
        assert 2 <= len(cases) == fz.rounds_for(family, cls) <= max(fz.ROUNDS[cls], 7 if family == "scan" else 4 if family == "tcomb" else 0)
        assert {c["bits"] for c in cases} <= set(fz.KEY_CLASSES[cls])
    for cls in ("digit72", "lanes"):
        assert {c["bits"] for c in schedule[("segprod", cls)]} == set(fz.KEY_CLASSES[cls])           # every size of the class
    assert {c["bits"] for c in schedule[("segprod", "wide")]} == {3328, 3584}                        # two rounds: 4096 in the long runs


@pytest.mark.parametrize("cls", CLASSES)
def test_schedule_segment_structure(schedule, cls):
    for family in ("segprod", "smexp"):
        got = shapes(schedule[(family, cls)])
        for name in ("empty_front", "empty_middle", "empty_end", "single_member", "majority"):
            assert name in got, (family, cls, name)
        straddle = {"len64", "len65", "len256", "len257"} if family == "segprod" or cls != "wide" else set()   # (60 terms at most on wide keys)
        assert straddle <= got, (family, cls, straddle - got)
        assert any(c["dirty"] for c in schedule[(family, cls)]) and any(not c["dirty"] for c in schedule[(family, cls)])
    sp = schedule[("segprod", cls)]
    assert knob_values(sp, "segprod_chunk") == set(fz.SEGPROD_CHUNKS) == {None, 1, 2, 3, 7}
    assert knob_values(schedule[("smexp", cls)], "smexp_chunk") == set(fz.SMEXP_CHUNKS) == {None, 1, 2, 3}
    assert all(c["N"] <= (80 if cls == "wide" else 600) and -2 <= c["tag"] <= 2 for c in sp)
    assert all(c["N"] <= 40 and c["T"] <= (60 if cls == "wide" else 300) for c in schedule[("smexp", cls)])
    assert "gather" in shapes(sp) and "shift" in shapes(sp) and "first_negative" in shapes(sp)
    assert any(c["status_bit"] == 0 for c in sp)                               # and a clean round, whose status must read 0


@pytest.mark.parametrize("cls", CLASSES)
def test_schedule_scan_pack_open_crtenc_per_class(schedule, cls):
    sc = schedule[("scan", cls)]
    assert {f"seg_len_{v}" for v in fz.SCAN_SEG} | {"reverse_0", "reverse_1", "first_negative", "step", "raise"} <= shapes(sc)
    assert knob_values(sc, "scan_chunk") == {None, 1, 2, 3, 5}
    assert any(c["dirty"] for c in sc) and any(c["status_bit"] == 0 for c in sc)
    pk = schedule[("pack", cls)]
    assert {8, 128} <= {c["slot_bits"] for c in pk} and {"slots_1", "slots_max"} <= shapes(pk)
    assert 0 in {c["tag"] for c in pk} and {c["tag"] for c in pk} - {0}
    op = schedule[("open", cls)]
    assert 8 in {c["e_words"] for c in op} and any(c["e_words"] == (c["ebits"] + 31) // 32 for c in op)
    assert {"bad_row_kept", "bad_row_excluded", "falsified"} <= shapes(op)
    ce = shapes(schedule[("crtenc", cls)])
    assert {"r_zero", "r_one", "r_all_ones", "r_one_window", "m_zero", "m_n_minus_1", "m_max_int"} <= ce, (cls, ce)


def test_schedule_over_all_classes(schedule):
    """what two rounds cannot hold is asserted over the four tests of a family"""
    def family(name):
        return [c for cls in CLASSES for c in schedule[(name, cls)]]

    sp = shapes(family("segprod"))
    assert {"gather", "rows_null", "shift", "shift_null"} <= sp
    assert {c["tag"] for c in family("segprod")} == {-2, -1, 0, 1, 2}
    assert any(c["planted_non_unit"] is not None for c in family("segprod"))
    sc = family("scan")
    assert {f"seg_len_{v}" for v in fz.SCAN_SEG} <= shapes(sc) and {"reverse_0", "reverse_1", "raise", "raise_null", "step", "step_null"} <= shapes(sc)
    assert knob_values(sc, "scan_chunk") == {None, 1, 2, 3, 5}
    assert {c["tag"] for c in sc} == {-2, -1, 0, 1, 2} == {c["dom_out"] for c in sc}
    assert any(c["dirty"] for c in sc)
    sm = shapes(family("smexp"))
    assert {f"ebits_{v}" for v in fz.SMEXP_EBITS} <= sm and {"signed", "unsigned", "e_zero", "e_ones"} <= sm
    pk = family("pack")
    assert {"slots_1", "slots_max", "slots_mid", "ragged"} <= shapes(pk) and {c["tag"] for c in pk} == {-2, -1, 0, 1, 2}
    assert {c["slot_bits"] for c in pk} | {c["step_bits"] for c in pk} <= set(range(8, 129))
    assert {tuple(r["disable"]) for c in pk for r in c["runs"]} == {(), ("pack_padic",)} and knob_values(pk, "pack_padic_min") == {0, None}
    op = shapes(family("open"))
    assert {f"ebits_{v}" for v in fz.OPEN_EBITS} <= op and {f"seg_len_{v}" for v in fz.OPEN_SEG} <= op
    assert {f"chunk_{v}" for v in fz.OPEN_CHUNKS} <= op and {f"wbits_{v}" for v in fz.OPEN_WBITS} <= op
    assert {"falsified", "honest", "bad_row_kept", "bad_row_excluded"} <= op
    assert {c["e_words"] for c in family("open")} >= {1, 8}
    ce = family("crtenc")
    assert {f"N_{v}" for v in fz.CRT_N} | {"N_random"} <= shapes(ce)
    assert {c["served"] for c in ce} == {True, False}
    tp = shapes(family("tpart"))
    assert {f"E_{v}" for v in fz.TPART_SMALL} | {"E_pow2", "E_pow2_minus_1", "E_zero_run", "E_random"} <= tp
    assert {f"N_{v}" for v in fz.TPART_N} | {"tpart_min_0", "tpart_min_unset", "tpart_grid_1"} <= tp
    tc = shapes(family("tcomb"))
    assert {"all_positive", "all_negative", "mixed_signs", "bit127", "mu_one", "mu_two64", "mu_bit127", "mu_same_top", "mu_random", "t_1", "t_16",
            "mu_words_4", "mu_words_fit", "theta_1", "theta_n_minus_1", "theta_random", "grid_1", "grid_unset"} <= tc
    assert any(6 <= c["t"] <= 15 for c in family("tcomb"))


@pytest.mark.parametrize("cls", CLASSES)
def test_schedule_threshold_families(schedule, cls):
    tp, tc = schedule[("tpart", cls)], schedule[("tcomb", cls)]
    got = shapes(tp)
    assert "E_1" in got and "E_pow2" in got and "E_pow2_minus_1" in got and "E_zero_run" in got and "E_random" in got
    for c in tp:
        bits = c["bits"]
        for E in c["E"]:
            assert 0 < E < 1 << (2 * bits + 65) and (E.bit_length() + 31) // 32 <= 1024
            s = bin(E)[2:]
            if E > 1 << 64 and "0" * 300 in s.strip("0"):
                got.add("inner zero run >= 300")
        assert c["N"] <= (513 if cls.startswith("digit") else 40)
    assert "inner zero run >= 300" in got
    if cls.startswith("digit"):
        assert {"tpart_min_0", "tpart_min_unset", "tpart_grid_1"} <= got and any(c["digit_route"] for c in tp)
    got = shapes(tc)
    assert {"all_positive", "all_negative", "mixed_signs", "bit127", "mu_same_top", "mu_one", "mu_two64", "mu_words_4", "mu_words_fit"} <= got, (cls, got)
    assert any(c["t"] >= 2 and 0 < sum(c["neg"]) < c["t"] for c in tc)         # both sides in one call
    assert all(c["N"] >= 4 and len(c["corrupt"]) >= 1 for c in tc)             # every case has falsified rows
    assert any(6 <= c["t"] <= 15 for c in tc) and {1, 16} <= {c["t"] for c in tc}
    assert any(c["poison"] is not None for c in tc)
    assert all(1 <= c["t"] <= 16 and len(c["parts"]) == c["t"] for c in tc)
    assert all([r["disable"] for r in c["runs"]] == [[], ["tcombine"]] and all(r["tune"]["tcomb_min"] == 0 for r in c["runs"]) for c in tc)
