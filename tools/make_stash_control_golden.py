#!/usr/bin/env python3
"""Record tests/golden/stash_control_parent.npz on the GPU:

    python tools/make_stash_control_golden.py [--lib PATH/libhector_amd.so]
        [--only gpu|emul] [--merge OTHER.npz] [--out FILE.npz]

The cases of tests/stash_control_cases.py -- 96 members S x Q10, SSP2-4.5 and SSP5-8.5, plain run
kernel, two-wave flavour, four biomes -- as computed by the build of the commit BEFORE a change to
the control of the stash and of the segment loop, so that the tests can demand the same bits of the
build after it.  Per case ("gpu/<scenario>/<kernel>/"): CO2, tas, sst, land_tas of eight years as
float64, every year's stash count, the status words, and a SHA-256 of each output's whole series.
The same for that commit's host emulation ("emul/..."), whose arithmetic is the host compiler's and
not the GPU's bit for bit, and for the flag cases (HX_ERR_NEGPOOL, HX_ERR_MASS) on both.
--only records one of the two halves (the emulation needs no GPU; it is always the tests' own
tests/emul/libhector_amd_emul.so), --merge adds the entries of a file recorded that way."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stash_control_cases as sc  # noqa: E402


def flag_entries(r, prefix):
    d = {prefix + "status": r["status"].astype(np.int64)}
    for v in sc.FLAG_OUTS:
        d[prefix + v + "_sha256"] = np.array(sc.digest(r[v]))
    return d


def record(lib, tag, only_extra=False, **kw):
    data = {}
    for scen, kernel in sc.CASES:
        if only_extra and kernel not in sc.EXTRA:
            continue
        r = sc.run_case(lib, scen, kernel, **kw)
        data.update(sc.golden_entries(r, "%s/%s/%s/" % (tag, scen, kernel)))
        print("%s %s %s: status clean %s, stashes %d" % (tag, scen, kernel, (r["status"] == 0).all(),
                                                        int(r["timesteps"][1:].sum())), flush=True)
    for which in sc.FLAG_CASES:
        r = sc.run_flag_case(lib, which, **kw)
        data.update(flag_entries(r, "%s/flag_%s/" % (tag, which)))
        print("%s flag case %s: status %s" % (tag, which, r["status"].tolist()), flush=True)
    return data


def main():
    lib = os.path.join(ROOT, "hector_amd", "lib", "libhector_amd.so")
    emul = os.path.join(ROOT, "tests", "emul", "libhector_amd_emul.so")
    out = sc.GOLDEN
    only, merge = None, None
    argv = sys.argv[1:]
    while argv:
        a = argv.pop(0)
        if a == "--lib":
            lib = os.path.abspath(argv.pop(0))
        elif a == "--only":
            only = argv.pop(0)
        elif a == "--merge":
            merge = os.path.abspath(argv.pop(0))
        elif a == "--out":
            out = os.path.abspath(argv.pop(0))
        else:
            sys.exit(__doc__)
    S, q10 = sc.ensemble96()
    data = {"S": S, "q10": q10, "years": np.array(sc.GOLDEN_YEARS)}
    if merge:
        with np.load(merge) as g:
            data.update({k: g[k] for k in g.files})
    if only in (None, "gpu"):
        data.update(record(lib, "gpu", device=0))
    if only in (None, "emul"):
        data.update(record(emul, "emul", allow_emulation=True))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **data)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
