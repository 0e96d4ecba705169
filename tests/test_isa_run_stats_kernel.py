"""Static figures of hx_run_kernel_stats -- the plain one-biome kernel with the statistics epilogue,
what the headline configuration launches -- held against the plain kernel's of the same build
(tests/test_isa_lint.py holds those): same registers, same LDS, no scratch, the spilled scalars
within the plain kernel's bound, and every loop of the plain kernel present with its instruction
count -- the loops that enclose a whole year within 8 instructions (the epilogue's presence costs
the register allocator one more scalar reload there; measured: +1 and 0).  No GPU needed: the
compiler's assembly in hector_amd/build."""
import glob
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

PLAIN = "_Z13hx_run_kernelILi1ELb0ELb0ELi0EEvPK6HxArgsii"
STATS = "_Z19hx_run_kernel_statsILi1ELb1EEvPK6HxArgsii"


def _loops(isa_stats, ins):
    """Instruction counts of a kernel's loops (backward branches), in program order of their ends --
    what `tools/isa_stats.py --loops` prints."""
    labels = {s: i for i, (op, s) in enumerate(ins) if op == "label"}
    out, seen = [], set()
    for i, (op, s) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = s.split()[-1]
            if tgt in labels and labels[tgt] < i and (labels[tgt], i) not in seen:
                seen.add((labels[tgt], i))
                n = sum(isa_stats.hist(ins[labels[tgt]:i + 1]).values())
                if n >= 40:
                    out.append(n)
    return out


def test_stats_kernel_keeps_the_plain_kernels_figures():
    files = glob.glob(os.path.join(ROOT, "hector_amd", "build", "hx_kernels-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not files:
        pytest.skip("no assembly in hector_amd/build (the library was not built in this tree)")
    import isa_stats
    kernels, meta = isa_stats.parse(files[0])
    assert PLAIN in meta and STATS in meta
    p, s = meta[PLAIN], meta[STATS]
    assert int(s["private_segment_fixed_size"]) == 0
    assert int(s["vgpr_count"]) == int(p["vgpr_count"])
    assert int(s["group_segment_fixed_size"]) == int(p["group_segment_fixed_size"])
    assert int(s["sgpr_spill_count"]) <= 30                      # the plain kernel's bound
    n_p = sum(isa_stats.hist(kernels[PLAIN]).values())
    n_s = sum(isa_stats.hist(kernels[STATS]).values())
    assert n_p < n_s <= n_p + 900                                 # the epilogue: ~870 instructions, once a launch
    lp, ls = _loops(isa_stats, kernels[PLAIN]), _loops(isa_stats, kernels[STATS])
    assert len(ls) > len(lp)                                      # (the epilogue has loops of its own, behind)
    for a, b in zip(lp, ls):
        if a < 3000:        # loops inside a year: instruction for instruction
            assert a == b, (lp, ls)
        else:               # the year loop and the block loop around it
            assert a <= b <= a + 8, (lp, ls)
