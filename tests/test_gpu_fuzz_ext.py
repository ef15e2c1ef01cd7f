"""GPU: a round-counted, seeded differential fuzz of the extension entry points of the C ABI — the half tools/fuzz_gpu.py
(tests/test_gpu_fuzz.py) does not reach:

    pai_ct_segment_prod, pai_ct_scan, pai_ct_sparse_multiexp, pai_ct_pack, pai_ct_pack_step, pai_recover_r, pai_opening_fold,
    pai_encrypt_crt, pai_obfuscate_crt, pai_keyshare_create / pai_partial_decrypt, pai_threshold_combine.

One test per family and key class: a CONSTANT number of rounds (tests/_fuzz_ext.py: ROUNDS, ROUNDS_FOR, SEED), never a time
budget, so a seed covers the same cases on every machine.  Cases and expectations come from tests/_fuzz_ext.py (CPython integers; bulk powers
through tests/_util.pow_many), the calls from tests/_fuzz_ext_run.py; tests/test_fuzz_ext_cpu.py holds the models to plain
restatements and asserts, by name, that this schedule contains every shape class and knob value.  Knobs are set through
monkeypatch per run and restored; the profile is on; every test prints one COVERAGE line and asserts the kernels its family
exists to reach.  A mismatch fails with the reproducer line of tools/fuzz_ext_gpu.py.

Key classes: digit36 (1024 bits), digit72 (1408, 1536, 2048), lanes (2304, 2560, 3072), wide (3328, 3584, 4096); round r of a
test takes the r-th size of its class in turn.  Handles are created once per module and released at its end.

Measured on one MI355X, seconds per test (expectations on the host included; profiles/r22/fuzz_ext_times.json):
    segprod  digit36 0.51  digit72 0.54  lanes 1.32  wide 1.63
    scan     digit36 0.22  digit72 0.17  lanes 0.39  wide 1.24
    smexp    digit36 0.20  digit72 0.52  lanes 0.13  wide 0.10
    pack     digit36 0.43  digit72 0.93  lanes 1.70  wide 0.43
    open     digit36 0.46  digit72 0.93  lanes 2.54  wide 3.51
    crtenc   digit36 0.27  digit72 0.96  lanes 1.21  wide 2.58
    tpart    digit36 1.50  digit72 3.28  lanes 4.16  wide 6.90
    tcomb    digit36 1.13  digit72 1.20  lanes 0.74  wide 1.23
(sum 43.1 s; the longest, tpart-wide, is two rounds of two full-length exponents on 3328- and 3584-bit keys, most of it
CPython's side of the comparison.  With two rounds a wide test sees 3328 and 3584 bits; 4096 bits, the committed fixture
primes, run in scan-wide and tcomb-wide, which have more rounds, and in the long runs.)"""
import contextlib

import pytest

from pailliercryptolib_python_amd import _native
from tests import _fuzz_ext as fz
from tests import _fuzz_ext_run as fr
from tests._util import disable, tune

pytestmark = pytest.mark.gpu

DIGIT = ("digit36", "digit72")


@pytest.fixture(scope="module", autouse=True)
def handles_released():
    """later files find the device as this one found it: no key handle of this module, hence no table, stays"""
    yield
    fr.release_handles()


@pytest.fixture(autouse=True)
def profiled():
    lib = _native.load()
    _native.check(lib.pai_profile_enable(1))
    yield
    _native.check(lib.pai_profile_enable(0))


def required(family, cls, cov):
    """the kernels (as the profile names them) a test must have reached"""
    names = {c.split(":")[0].split("(")[0] for c in cov}
    digit = cls in DIGIT
    if family == "segprod":
        return "k_segprod:levels>=2" in cov
    if family == "scan":
        return "k_segscan:carry" in cov
    if family == "smexp":
        lanes = any(c.startswith("k_smexp:") and c.endswith("[lane groups]") for c in cov)
        pairs = any(c.startswith("k_smexp:") and c.endswith("[digit pairs]") for c in cov)
        return lanes and pairs == digit
    if family == "pack":
        return "k_segprod" in names and ("k_ct_pack_padic" in names) == digit
    if family == "open":
        return {"k_rrec_a", "k_rrec_b"} <= names and ("k_open_fold" in names) == digit
    if family == "crtenc":
        return "k_encrypt" in names and ("k_crt_lift" in names) == (cls != "digit36")     # 512-bit primes: below the digit engine
    if family == "tpart":
        return "k_ctmul" in names and ("k_pow_padic" in names) == digit
    if family == "tcomb":
        return "k_tfinish" in names and ("k_tcomb_padic" in names) == digit
    raise KeyError(family)


@pytest.mark.parametrize("cls", list(fz.KEY_CLASSES))
@pytest.mark.parametrize("family", fz.FAMILIES)
def test_fuzz_ext(family, cls, monkeypatch):
    @contextlib.contextmanager
    def with_knobs(run):
        with monkeypatch.context() as mp:
            for name, value in run["tune"].items():
                tune(mp, name, value)
            for name in run["disable"]:
                disable(mp, name)
            yield

    cov, checks = set(), 0
    for rnd in range(fz.rounds_for(family, cls)):
        checks += fr.run_round(family, cls, fz.SEED, rnd, with_knobs, cov)
    print(f"COVERAGE fuzz-ext {family} {cls}: {fz.rounds_for(family, cls)} rounds, {checks} comparisons: {' '.join(sorted(cov))}"
          + (" (engine labels inferred from the handle)" if family == "smexp" else ""))
    assert required(family, cls, cov), sorted(cov)
