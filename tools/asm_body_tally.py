"""Instruction tally of the large straight-line bodies of a gfx950 assembly listing (hipcc --cuda-device-only -S with the
flags of build.py): for every basic block of at least MIN instructions, the instruction count and the counts of the
multiply-adds and of the carry-stream instructions around them.  The squaring and the product of the register-resident
digit-pair decrypt kernels (csrc/mont_padic.hpp: sqr_kara_reg*, mul_kara_reg*) are the two largest blocks.

    python tools/asm_body_tally.py listing.s [MIN]
"""
import collections
import re
import sys

WATCH = ("v_mad_u64_u32", "v_mad_i64_i32", "v_lshl_add_u64", "v_lshrrev_b64", "v_ashrrev_i64", "v_and_b32", "v_bfe_i32",
         "v_addc_co_u32", "v_add_co_u32", "v_subb_co_u32", "v_sub_co_u32", "v_ashrrev_i32", "v_mov_b32",
         "v_accvgpr_write_b32", "v_accvgpr_read_b32")


def blocks(path):
    name, ops = None, collections.Counter()
    for line in open(path):
        s = line.strip()
        if re.match(r"^[A-Za-z_.$][\w.$]*:", s):
            if name is not None:
                yield name, ops
            name, ops = s.split(":")[0], collections.Counter()
            continue
        if not s or s.startswith((";", ".", "//")):
            continue
        ops[s.split()[0]] += 1
    if name is not None:
        yield name, ops


def main():
    path = sys.argv[1]
    least = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    for name, ops in blocks(path):
        total = sum(ops.values())
        if total >= least:
            print({"block": name, "instructions": total, **{w: ops[w] for w in WATCH if ops[w]}})
    for line in open(path):
        if re.search(r"\.(vgpr_count|agpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):", line):
            print(line.strip())


if __name__ == "__main__":
    main()
