#!/usr/bin/env python3
"""Two builds of the kernels side by side, kernel by kernel: registers, scratch, spills and static
instruction counts from the compiler's gfx950 assembly (tools/isa_stats.py reads one file).

    python tools/isa_compare.py before.s after.s [--kernel SUBSTRING]

Prints every kernel whose figures differ, with REGS+ / SCRATCH+ behind those that gained vector
registers (VGPR + AGPR) or scratch, and exits 1 if any did.  This is how the exclusion list of
hx_open_retry_k (hx_dev_solver.h) is derived, and how to re-derive it after a change of compiler:
  1. take every `return false` line but the first out of hx_open_retry_k;
  2. compile hx_kernels.hip twice with the product flags and -save-temps=obj, once with
     -DHX_NO_OPENING_RETRY (before.s) and once without (after.s);
  3. run this tool: every run kernel it marks goes (back) into the list; rebuild and run it again
     to see that nothing is marked (profiles/opening_retry_ab.md section 2)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_stats  # noqa: E402

KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "sgpr_spill_count",
        "vgpr_spill_count"]


def main():
    argv = sys.argv[1:]
    sub = None
    if "--kernel" in argv:
        i = argv.index("--kernel")
        sub = argv[i + 1]
        del argv[i:i + 2]
    a, ma = isa_stats.parse(argv[0])
    b, mb = isa_stats.parse(argv[1])
    n = changed = gained = 0
    print("kernel  [vgpr, agpr, sgpr, scratch B, spilled sgpr, spilled vgpr]  static instructions")
    for k in ma:
        if sub and sub not in k:
            continue
        if k not in mb:
            print("only in %s: %s" % (argv[0], k))
            continue
        n += 1
        da = [int(ma[k].get(x, 0) or 0) for x in KEYS]
        db = [int(mb[k].get(x, 0) or 0) for x in KEYS]
        ia, ib = sum(isa_stats.hist(a[k]).values()), sum(isa_stats.hist(b[k]).values())
        if da == db and ia == ib:
            continue
        changed += 1
        flag = (" SCRATCH+" if db[3] > da[3] else "") + (" REGS+" if db[0] + db[1] > da[0] + da[1] else "")
        gained += bool(flag)
        print("%-62s %s -> %s  %d -> %d%s" % (k[:62], da, db, ia, ib, flag))
    for k in mb:
        if k not in ma and not (sub and sub not in k):
            print("only in %s: %s" % (argv[1], k))
    print("%d kernels compared, %d differ, %d gained registers or scratch" % (n, changed, gained))
    return 1 if gained else 0


if __name__ == "__main__":
    sys.exit(main())
