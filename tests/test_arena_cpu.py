"""CPU: the layout and check code of tests/_arena.py over a numpy buffer standing in for the device — the harness of
tests/test_gpu_memory_contract.py has to see what it is for before a kernel is held to it."""
import numpy as np
import pytest

from tests._util import chacha_block
from tests._arena import ALIGNED, ALIGNS, FILLERS, GOLDEN, GUARD_MIN, NATURAL, Arena, HostBackend, filler_words

W = 34                                   # a row that is no multiple of 16 bytes (n of 521 bits: rows of 34 words)
DTYPES = (np.uint32, np.int32, np.float64, np.int64, np.uint64, np.uint8)


def build(filler, align):
    """an input, an output and a one-word flag, as a call of the library has them; the "kernel" writes through the backend's buffer"""
    be = HostBackend()
    ar = Arena(filler, backend=be)
    a = ar.place("a", np.arange(5 * W, dtype=np.uint32).reshape(5, W) + 7, align=align)
    out = ar.place("out", shape=(5, W), dtype=np.uint32, align=align)
    flag = ar.place("flag", shape=(1,), dtype=np.int32, align=align)
    ar.commit()
    return be, ar, a, out, flag


def words(be, region):
    """the region's words as a writable view of the stand-in device buffer"""
    return be.buf[region.offset:region.offset + region.nbytes].view(np.uint32)


def good_write(be, out, flag, want):
    words(be, out)[:] = want.reshape(-1)
    words(be, flag)[:] = 0


def test_filler_patterns():
    p = filler_words("pattern", 5)
    assert [int(x) for x in p] == [GOLDEN * (i + 1) % 2**32 for i in range(5)]
    assert len(set(int(x) for x in filler_words("pattern", 1 << 16))) == 1 << 16          # position-dependent: no word repeats
    assert (filler_words("ones", 9) == 0xFFFFFFFF).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_alignment_classes_land_on_their_residues(dtype):
    item = np.dtype(dtype).itemsize
    be = HostBackend()
    ar = Arena("pattern", backend=be)
    regs = [ar.place(f"r{i}{al}", shape=(3, 17), dtype=dtype, align=al) for i in range(3) for al in ALIGNS]
    ar.commit()
    assert ar.base % 256 == 0
    for r in regs:
        addr = r.address
        if r.name.endswith(ALIGNED):
            assert addr % 256 == 0
        else:
            assert addr % 16 == {4: 4, 8: 8, 1: 1}[item]
            assert addr % item == 0
            if item == 1:
                assert addr % 2 == 1
        assert r.at(2).value == addr + 2 * 17 * item


def test_guards_surround_every_region():
    be = HostBackend()
    ar = Arena("pattern", backend=be)
    small = ar.place("small", shape=(2, 4), dtype=np.uint32, align=NATURAL)
    wide = ar.place("wide", shape=(2, 2048), dtype=np.uint32, align=NATURAL)          # 4 rows = 32 KiB: more than the 4096-byte floor
    byte = ar.place("byte", shape=(5,), dtype=np.uint8, align=NATURAL)
    ar.commit()
    assert small.guard == GUARD_MIN and wide.guard == 4 * 2048 * 4 and byte.guard == GUARD_MIN
    regs = sorted(ar.regions, key=lambda r: r.offset)
    assert regs[0].offset >= regs[0].guard
    for lo, hi in zip(regs, regs[1:]):
        assert hi.offset - (lo.offset + lo.nbytes) >= lo.guard + hi.guard               # guards are not shared
    assert len(be.buf) - (regs[-1].offset + regs[-1].nbytes) >= regs[-1].guard
    # the shadow outside the regions is the filler, inside an unwritten region too
    assert (ar.shadow.view(np.uint32) == filler_words("pattern", len(be.buf) // 4)).all()


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filler", FILLERS)
def test_a_correct_call_passes(filler, align):
    be, ar, a, out, flag = build(filler, align)
    want = a.host * 3
    good_write(be, out, flag, want)
    ar.check({"out": want, "flag": np.zeros(1, np.int32)})


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filler", FILLERS)
def test_stray_word_before_a_region(filler, align):
    be, ar, a, out, flag = build(filler, align)
    want = a.host * 3
    good_write(be, out, flag, want)
    be.buf[out.offset - 4:out.offset].view(np.uint32)[0] = 0x12345678
    with pytest.raises(AssertionError, match=r"0x12345678.*in guard before 'out'") as e:
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})
    assert f"byte offset {out.offset - 4} " in str(e.value)


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filler", FILLERS)
def test_stray_word_after_a_region(filler, align):
    be, ar, a, out, flag = build(filler, align)
    want = a.host * 3
    good_write(be, out, flag, want)
    end = out.offset + out.nbytes
    be.buf[end:end + 4].view(np.uint32)[0] = 0x0BADF00D              # the word a store of W32 + 1 words per row leaves behind the last row
    with pytest.raises(AssertionError, match=r"0x0badf00d.*in guard after 'out'") as e:
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})
    assert f"byte offset {end} " in str(e.value)
    # a whole stray row at the far end of the guard is still the guard of `out`
    be.buf[end:end + 4] = ar.shadow[end:end + 4]
    far = end + out.guard - 4
    be.buf[far:far + 4].view(np.uint32)[0] = 1
    with pytest.raises(AssertionError, match=r"in guard after 'out'"):
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filler", FILLERS)
def test_stray_word_inside_an_input(filler, align):
    be, ar, a, out, flag = build(filler, align)
    want = a.host * 3
    good_write(be, out, flag, want)
    words(be, a)[2 * W + 5] ^= 1                                      # a kernel that stores its result into `a` as well
    with pytest.raises(AssertionError, match=r"in region 'a' \(row 2, byte 20 of the row\)"):
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("filler", FILLERS)
def test_missing_output_write(filler, align):
    """under the all-ones filler too: an unwritten row is no reduced residue"""
    be, ar, a, out, flag = build(filler, align)
    want = a.host * 3
    good_write(be, out, flag, want)
    words(be, out)[4 * W:] = ar.shadow[out.offset + 4 * W * 4:out.offset + out.nbytes].view(np.uint32)     # the last row never written
    with pytest.raises(AssertionError, match=r"in region 'out' \(row 4, byte 0 of the row\)"):
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})
    good_write(be, out, flag, want)
    words(be, flag)[:] = ar.shadow[flag.offset:flag.offset + 4].view(np.uint32)                            # the flag word never written
    with pytest.raises(AssertionError, match=r"in region 'flag'"):
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})


def test_aliased_output_replaces_the_input_in_the_shadow():
    be, ar, a, out, flag = build("pattern", NATURAL)
    want = a.host + 1
    words(be, a)[:] = want.reshape(-1)                                # in place: d_out == d_a
    ar.check({"a": want})
    with pytest.raises(AssertionError, match=r"in region 'a'"):
        ar.check({})                                                  # declared as an input, it must not change


def test_wrong_value_reports_first_differing_word():
    be, ar, a, out, flag = build("ones", ALIGNED)
    want = a.host * 3
    good_write(be, out, flag, want)
    words(be, out)[W + 1] += 1
    words(be, out)[3 * W] += 1
    with pytest.raises(AssertionError, match=r"in region 'out' \(row 1, byte 4 of the row\); 2 bytes differ"):
        ar.check({"out": want, "flag": np.zeros(1, np.int32)})


def test_chacha_model_is_rfc8439():
    """the block function of tests/_util.chacha_block, the model behind tests/test_gpu_memory_contract.py::test_draw_r_and_buffers, on the test vector of RFC 8439 section 2.3.2"""
    key8 = [int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8)]
    out = chacha_block(key8, 1, [0x09000000, 0x4A000000, 0])
    assert out[:4] == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3] and out[15] == 0x4E3C50A2
