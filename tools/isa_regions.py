#!/usr/bin/env python3
"""Instruction mix of ONE kernel of a hipcc -S listing, split at its phase stamps:

    tools/isa_regions.py file.s name-filter [name-filter ...] [--blocks]

(`make -C parallel-gps_amd/csrc res_asm` emits the listing of the resident unit; the default instantiation of config c2 is
`k_pkfs_resident IdLi2ELi16ELb0ELb1ELb0E`.)

A stamp is the `global_store_dwordx2` of the cycle counter behind PGPS_RSTAMP / PGPS_RSTAMP_WAVE (pgps_resident.hip.h): the
first such store after an `s_memtime`.  PGPS_RSTAMP(k) stores at `offset:8k` of the workgroup's row, so the slot is read
off the store (14 = the diagnostic stamp in front of the suffix scan); the per-wave stamps go to a table of their own and
print as `wave`.  Regions are in LAYOUT order, which is the program's order for the straight-line phases of the kernel; a
region that holds branches is the sum of all its sides.
Per region: fp64 arithmetic (of which: with a literal-zero operand -- a sum started at zero or a product with a compile-time
identity), AGPR moves, DPP, LDS, global memory, branches, other VALU, scalar, waits.  `head` is the part of the region in front of its first
DPP instruction (for the region behind stamp 5: whatever stands between the Kalman pass and the suffix scan's first level).
--blocks adds one line per basic block."""
import collections
import re
import sys

COLS = ("fp64", "fp64_zero", "agpr", "dpp", "lds", "global", "branch", "valu", "salu", "wait")


def classify(op, rest):
    dpp = "_dpp" in op or re.search(r"\b(row_|wave_|quad_perm|row_bcast|row_mirror|row_half_mirror)", rest) is not None
    if dpp:
        return ["dpp"]
    if op.startswith("v_accvgpr"):
        return ["agpr"]
    if re.match(r"v_\w+_f64", op):
        ops = [o.strip() for o in rest.split(",")]
        return ["fp64", "fp64_zero"] if any(o in ("0", "-0", "0.0") for o in ops[1:]) else ["fp64"]
    if op.startswith("v_"):
        return ["valu"]
    if op.startswith("ds_"):
        return ["lds"]
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return ["global"]
    if op.startswith(("s_cbranch", "s_branch")):
        return ["branch"]
    if op.startswith(("s_waitcnt", "s_nop")):
        return ["wait"]
    return ["salu"]


def fmt(name, c, n):
    return f"{name:34s} {n:6d}  " + " ".join(f"{c[k]:>9d}" for k in COLS)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    blocks = "--blocks" in sys.argv
    if len(args) < 2:
        sys.exit(__doc__)
    lines = open(args[0]).read().split("\n")
    flt = args[1:]
    start = None
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m and all(f in m.group(1) for f in flt):
            if start is not None:
                sys.exit(f"the filter matches more than one kernel: {name} and {m.group(1)}")
            start, name = i, m.group(1)
    if start is None:
        sys.exit("no kernel matches")
    regions = []            # (label, first line, Counter, n, head Counter or None, head n, blocks)
    cur = dict(label="start", line=start + 1, c=collections.Counter(), n=0, head=None, headn=0, blocks=[])
    blk = dict(label="(entry)", c=collections.Counter(), n=0)
    armed, last = False, -1
    for i in range(start + 1, len(lines)):
        s = lines[i].split(";")[0].strip()
        if not s or s[0] in "./":
            if s.startswith(".LBB") and s.endswith(":"):
                cur["blocks"].append(blk)
                blk = dict(label=s[:-1], c=collections.Counter(), n=0)
            continue
        if s.endswith(":"):
            continue
        op, _, rest = s.partition(" ")
        op, rest = op.strip(), rest.strip()
        kinds = classify(op, rest)
        if "dpp" in kinds and cur["head"] is None:
            cur["head"], cur["headn"] = collections.Counter(cur["c"]), cur["n"]
        for k in kinds:
            cur["c"][k] += 1
            blk["c"][k] += 1
        cur["n"] += 1
        blk["n"] += 1
        if op.startswith("s_memtime"):
            armed = True
        elif armed and op.startswith("global_store_dwordx2"):
            armed = False
            m = re.search(r"offset:(\d+)", rest)
            off = int(m.group(1)) if m else 0
            # a per-wave stamp K follows workgroup stamp 1 / 4 at offset 32 K of its own table: never a slot not yet passed
            if off % 8 == 0 and off < 128 and (off // 8 > last or off // 8 == 14):
                slot = f"stamp {off // 8}"
                last = max(last, off // 8) if off // 8 != 14 else last
            else:
                slot = "stamp (wave)"
            cur["blocks"].append(blk)
            blk = dict(label="(behind the stamp)", c=collections.Counter(), n=0)
            regions.append(cur)
            cur = dict(label=slot, line=i + 1, c=collections.Counter(), n=0, head=None, headn=0, blocks=[])
        if op.startswith("s_endpgm"):
            break
    cur["blocks"].append(blk)
    regions.append(cur)
    print(name)
    print(f"{'region (from .. to the next stamp)':34s} {'instr':>6s}  " + " ".join(f"{k:>9s}" for k in COLS))
    for r in regions:
        print(fmt(f"{r['label']} @ line {r['line']}", r["c"], r["n"]))
        if r["head"] is not None and r["headn"] != r["n"]:
            print(fmt("    head (before its first DPP)", r["head"], r["headn"]))
        if blocks:
            for b in r["blocks"]:
                if b["n"]:
                    print(fmt(f"      {b['label']}", b["c"], b["n"]))
    tot = collections.Counter()
    for r in regions:
        tot.update(r["c"])
    print(fmt("whole kernel", tot, sum(r["n"] for r in regions)))


if __name__ == "__main__":
    main()
