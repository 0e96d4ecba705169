#!/usr/bin/env python3
"""The device-math probe's figures on the GPU and on the host build, side by side.

    make -C tests/devmath && python tools/devmath_report.py [out.json]   ->  profiles/devmath_report.json

Run by hand on a machine with the GPU, never by a test.  Per operation (tests/devmath/devmath_checks.py:
every form and output position over the inputs of tests/golden/devmath_reference.npz): the worst error
on the device with the input that gives it, the worst error of the host emulation, the number of
outputs whose bits differ between the two, and the bound the tests hold both to.  Then the outputs of
the exp / log forms whose bits differ from hx_exp_batch<1> / hx_log on the device (expected: none)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "devmath"))
import bench  # noqa: E402
import devmath_checks as dm  # noqa: E402


def main(path=os.path.join(ROOT, "profiles", "devmath_report.json")):
    G = dm.golden()
    dev, emu = dm.Probe(dm.HIP_PROBE), dm.Probe(dm.EMUL_PROBE)
    assert dev.backend == "hip" and emu.backend == "host-emulation"
    rep = {"compiler": bench.compiler_id(), "kernel_source_hash": bench.kernel_source_hash(),
           "fixture": "tests/golden/devmath_reference.npz", "operations": {}}
    for op in dm.OPERATIONS:
        md, me = dm.measure(dev, G, op), dm.measure(emu, G, op)
        wd, xd, _ = dm.worst(md)
        we, _, _ = dm.worst(me)
        bound = md["bound"]
        entry = {"unit": md["unit"], "outputs": int(md["err"].size),
                 "bound": float(bound) if not np.ndim(bound) else "8 * 2^-53 * sum|terms| + 2^-52 (per output)",
                 "worst_device": wd, "worst_device_input": xd, "worst_emulation": we,
                 "outputs_differing_device_vs_emulation": int((dm.bits(md["got"]) != dm.bits(me["got"])).sum())}
        if np.ndim(bound):
            entry["worst_device_share_of_bound"] = float((md["err"] / bound).max())
            entry["worst_emulation_share_of_bound"] = float((me["err"] / bound).max())
        rep["operations"][op] = entry
    rep["device_exp_forms_differing_from_hx_exp_batch_1"] = dm.exp_mismatches(dev, G)
    rep["device_log_forms_differing_from_hx_log"] = dm.log_mismatches(dev, G)
    assert dev.failed is None and emu.failed is None
    with open(path, "w") as fo:
        json.dump(rep, fo, indent=1)
        fo.write("\n")
    print(json.dumps(rep, indent=1))


if __name__ == "__main__":
    main(*sys.argv[1:2])
