"""CPU: the case table of the stream-contract tests (tests/_stream_cases.py) against include/paillier_hip.h, by name: every
prototype with a `void* stream` parameter has a row or a written reason to have none, no row names a function the header does not
have, and a row's `syncs` flag says what the header's own comment says about the call."""
import re
from pathlib import Path

from tests import _stream_cases as sc

HEADER = (Path(__file__).resolve().parents[1] / "include" / "paillier_hip.h").read_text()
# the header's wordings for "this call synchronises its stream"
SYNC_WORDS = re.compile(r"Synchronous;|ynchronises `stream`|ynchronisation of `stream`")


def prototypes():
    """[(name, parameter text, the comment block in front of it — shared by prototypes that follow one another without a comment)]"""
    out, comment = [], ""
    body = HEADER[HEADER.index('extern "C" {'):]
    for m in re.finditer(r"/\*(.*?)\*/|\b(?:int|void|const char\*)\s+(pai_\w+)\s*\(([^;{]*)\)\s*;", body, re.S):
        if m.group(1) is not None:
            comment = m.group(1)
        else:
            out.append((m.group(2), " ".join(m.group(3).split()), comment))
    return out


def stream_takers():
    return [(name, comment) for name, params, comment in prototypes() if re.search(r"\bvoid\s*\*\s*stream\b", params)]


def test_the_parser_sees_the_whole_header():
    from pailliercryptolib_python_amd import _native

    names = {name for name, _, _ in prototypes()}
    assert names == set(_native.PROTOTYPES), sorted(names ^ set(_native.PROTOTYPES))
    assert len(stream_takers()) >= 45


def test_every_stream_taking_entry_point_has_a_row_or_a_reason():
    takers = [name for name, _ in stream_takers()]
    assert len(takers) == len(set(takers))
    rows = [r.name for r in sc.TABLE]
    assert len(rows) == len(set(rows)), "a row twice"
    missing = [n for n in takers if n not in sc.BY_NAME and n not in sc.EXCLUDED]
    assert not missing, f"entry points with a stream argument and neither a row nor a reason: {missing}"
    assert not [n for n in rows if n not in takers], "rows for functions that take no stream"
    assert not [n for n in sc.EXCLUDED if n not in takers or n in sc.BY_NAME], "stale exclusions"
    assert set(sc.EXCLUDED) == {"pai_memcpy_h2d", "pai_memcpy_d2h", "pai_stream_sync"}       # the harness itself, nothing else
    assert all(len(reason) > 20 for reason in sc.EXCLUDED.values())


def test_syncs_flags_say_what_the_header_says():
    said = {name for name, comment in stream_takers() if SYNC_WORDS.search(comment)}
    flagged = {r.name for r in sc.TABLE if r.syncs}
    assert {"pai_ct_invert", "pai_pubkey_status", "pai_ct_pow2", "pai_ct_segment_prod", "pai_ct_sparse_multiexp", "pai_opening_fold",
            "pai_ct_pack"} <= flagged
    assert flagged == said - set(sc.EXCLUDED), (sorted(flagged - said), sorted(said - flagged))


def test_rows_are_well_formed():
    for r in sc.TABLE:
        assert r.build is not None or (r.family is not None and not r.chained), r.name      # every chained row can be called alone (test B)
        assert set(r.variants) <= set(sc.VARIANTS) and r.variants, r.name
        assert 2048 in r.bits and set(r.bits) <= set(sc.ALL_BITS), r.name
        assert isinstance(r.chained, (bool, set)), r.name
        if isinstance(r.chained, set):
            assert r.chained <= set(r.variants), r.name
        assert r.N in (sc.N_TILE, sc.N_LANES)
    # the rows whose dispatcher takes a different route per key class run on one key of every class
    for name in ("pai_ct_mul", "pai_decrypt", "pai_encrypt", "pai_partial_decrypt", "pai_threshold_combine", "pai_ct_segment_prod",
                 "pai_ct_scan", "pai_ct_sparse_multiexp", "pai_opening_fold", "pai_encrypt_crt"):
        assert sc.BY_NAME[name].bits == sc.ALL_BITS, name
    from tests import _fuzz_ext as fz

    assert {r.family for r in sc.TABLE if r.family} <= set(fz.FAMILIES)
    for cls, sizes in fz.KEY_CLASSES.items():
        assert any(b in sizes for b in sc.ALL_BITS), cls


def test_fillers_are_rotations_and_sentinels_are_not_values():
    import numpy as np

    from tests import _streams

    s = _streams.sentinel((3, 4))
    assert s.dtype == np.uint32 and (s == 0xA5A5A5A5).all()
    assert np.isfinite(_streams.sentinel((2,), np.float64)).all()
    assert _streams.MAX_STREAMS == 3 and _streams.BLOCKER_BITS == 4096
