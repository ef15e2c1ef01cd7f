"""Round-counted differential run of the extension entry points of the C ABI against CPython integers, for long runs by hand
(the committed, short schedule: tests/test_gpu_fuzz_ext.py; the other half of the ABI: tools/fuzz_gpu.py).
    python tools/fuzz_ext_gpu.py ROUNDS [SEED] [FAMILY] [CLASS]
Round r runs every family (or FAMILY) once, on key class (r + r // 8) % 4 of digit36, digit72, lanes, wide — the generators key
their round kinds on r modulo 2, 4 and 8, and the r // 8 term lets every class meet every kind — or on CLASS in every round, as the
tests do, and that class's (r % sizes)-th key size, with the case tests/_fuzz_ext.case(family, key, SEED, r) — the cases depend on
the arguments only, never on the clock.  Prints one JSON line; before it, for every mismatch (the run stops after five), the one-line reproducer — family, key
bits, seed, round, knobs, first differing row — and then exits 1."""
import contextlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pailliercryptolib_python_amd import _native
from tests import _fuzz_ext as fz
from tests import _fuzz_ext_run as fr

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
SEED = int(sys.argv[2]) if len(sys.argv) > 2 else fz.SEED
FAMILIES = (sys.argv[3],) if len(sys.argv) > 3 else fz.FAMILIES
CLASS = sys.argv[4] if len(sys.argv) > 4 else None
assert all(f in fz.FAMILIES for f in FAMILIES), f"families: {fz.FAMILIES}"
assert CLASS is None or CLASS in fz.KEY_CLASSES, f"classes: {list(fz.KEY_CLASSES)}"


@contextlib.contextmanager
def with_knobs(run):
    saved = {k: os.environ.get(k) for k in ("PAI_TUNE", "PAI_DISABLE")}
    tune = [f"{k}={v}" for k, v in run["tune"].items() if v is not None]
    os.environ["PAI_TUNE"] = ",".join(tune)
    os.environ["PAI_DISABLE"] = ",".join(run["disable"])
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


for k in ("PAI_TUNE", "PAI_DISABLE", "PAI_LATENCY_MAX", "PAI_LAT_ADD_MAX", "PAI_POW2_DIGIT_MIN"):
    os.environ.pop(k, None)
_native.check(_native.load().pai_profile_enable(1))
classes = list(fz.KEY_CLASSES)
t0 = time.time()
cov, checks, cases, failures = set(), 0, 0, 0
per_family = {f: 0.0 for f in FAMILIES}
for r in range(ROUNDS):
    cls = CLASS or classes[(r + r // 8) % 4]                   # (r // 8: no class is tied to a residue of r modulo 2, 4 or 8)
    for family in FAMILIES:
        t1 = time.time()
        try:
            checks += fr.run_round(family, cls, SEED, r, with_knobs, cov)
        except AssertionError as e:                            # a wrong result: the reproducer, and on with the next case (five at most)
            failures += 1
            print(str(e), flush=True)
        cases += 1
        per_family[family] += time.time() - t1
    if failures >= 5:
        break
    if r % 10 == 9:
        print(f"[fuzz-ext] {r + 1} of {ROUNDS} rounds, {checks} comparisons, {failures} failures, {time.time() - t0:.0f} s", file=sys.stderr, flush=True)
fr.release_handles()
print(json.dumps({"rounds": ROUNDS, "cases": cases, "checks": checks, "seconds": round(time.time() - t0, 1), "failures": failures, "seed": SEED, "class": CLASS,
                  "families": list(FAMILIES), "seconds_per_family": {f: round(v, 1) for f, v in per_family.items()}, "kernels": sorted(cov)}))
sys.exit(1 if failures else 0)
