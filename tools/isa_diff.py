#!/usr/bin/env python3
"""Which device functions differ between two builds: diffs two directories of assembly listings per symbol.

usage: isa_diff.py DIR_A DIR_B
The listings are what `hipcc --offload-device-only -S` writes with the flags of build.py, one NAME.s per translation unit
in each directory.  A symbol's text is everything from its `.type SYM,@function` to its `.size SYM`, plus its
`.amdhsa_kernel SYM` descriptor (registers, LDS, scratch).  Local labels carry the ordinal of the function inside its
file (.LBB12_3, .Lfunc_end12); the ordinal and the compiler's `;` comments (which repeat it) are dropped, so a function
that only moved inside the file compares equal.
Prints the symbols that are missing on one side or whose text differs; exit status 1 if there are any."""
import re
import sys
from pathlib import Path

ORDINAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|LCPI|Ltmp)\d+")


def symbols(path):
    out, cur, name = {}, None, None
    for ln in path.read_text().split("\n"):
        m = re.match(r"\s*\.type\s+(\S+),@function", ln) or re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m and cur is None:
            name, cur = m.group(1), out.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(ORDINAL.sub(r".\1", ln.split(";")[0].rstrip()))
            if re.match(r"\s*\.size\s+%s," % re.escape(name), ln) or ln.strip() == ".end_amdhsa_kernel":
                cur = None
    return out


def main():
    a, b = Path(sys.argv[1]), Path(sys.argv[2])
    names = sorted({p.name for p in a.glob("*.s")} | {p.name for p in b.glob("*.s")})
    total = same = 0
    for n in names:
        sa = symbols(a / n) if (a / n).exists() else {}
        sb = symbols(b / n) if (b / n).exists() else {}
        for sym in sorted(set(sa) | set(sb)):
            total += 1
            if sym not in sa or sym not in sb:
                print(f"{n}: {sym}: only in {a if sym in sa else b}")
            elif sa[sym] != sb[sym]:
                print(f"{n}: {sym}: differs ({len(sa[sym])} / {len(sb[sym])} lines)")
            else:
                same += 1
    print(f"{total} symbols in {len(names)} listings, {same} identical")
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
