#!/usr/bin/env python3
"""Record tests/golden/step_control_parent.npz on the GPU:

    python tools/make_step_control_golden.py [--lib PATH/libhector_amd.so] [--out FILE.npz]

The 96-member S x Q10 ensemble of tests/test_gpu_step_control.py (SSP2-4.5, run kernel and its
two-wave flavour) as computed by the library given with --lib: the build of the commit BEFORE a
change to the step loop's control, so that the test can demand the same bits of the build after
it.  Holds CO2 and Tgav of eight years and each member's 555-year sums of solver_steps and
timesteps, for the plain run kernel (`co2`, `tgav`, `solver_steps`, `timesteps`) and the two-wave
flavour (`*_run2`)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hector_amd  # noqa: E402

YEARS = (1850, 1950, 2000, 2050, 2100, 2150, 2200, 2300)


def ensemble96():
    """S on a grid of 12 values from 1.5 to 6.0, Q10 on 8 from 1.2 to 4.0: member i = (i // 8, i % 8)."""
    S = np.repeat(np.linspace(1.5, 6.0, 12), 8)
    q10 = np.tile(np.linspace(1.2, 4.0, 8), 12)
    return S, q10


def record(lib, two_wave):
    S, q10 = ensemble96()
    c = hector_amd.Core(hector_amd.DEFAULT_SCENARIO, S.size, device=0, lib_path=lib)
    assert c.backend == "hip"
    c.set_pair_kernel_limit(0)
    c.set_two_wave_from(1 if two_wave else 0)
    c.setvar("S", S, "degC").setvar("q10_rh", q10, "(unitless)")
    c.set_outputs(["CO2_concentration", "global_tas", "timesteps", "solver_steps"])
    c.run(2300)
    assert c.last_run_kernel() == ("run2" if two_wave else "run")
    assert (c.status() == 0).all()
    rows = [y - 1745 for y in YEARS]
    out = {"co2": c.fetchvars("CO2_concentration", (1745, 2300))[rows].copy(),
           "tgav": c.fetchvars("global_tas", (1745, 2300))[rows].copy(),
           "solver_steps": c.fetchvars("solver_steps", (1746, 2300)).sum(0).astype(np.int64),
           "timesteps": c.fetchvars("timesteps", (1746, 2300)).sum(0).astype(np.int64)}
    c.shutdown()
    return out


def main():
    lib = None
    out = os.path.join(ROOT, "tests", "golden", "step_control_parent.npz")
    argv = sys.argv[1:]
    while argv:
        a = argv.pop(0)
        if a == "--lib":
            lib = os.path.abspath(argv.pop(0))
        elif a == "--out":
            out = os.path.abspath(argv.pop(0))
        else:
            sys.exit(__doc__)
    S, q10 = ensemble96()
    data = {"S": S, "q10": q10, "years": np.array(YEARS)}
    data.update(record(lib, False))
    data.update({k + "_run2": v for k, v in record(lib, True).items()})
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez(out, **data)
    print("wrote %s (%d bytes): solver_steps %d, timesteps %d in all" % (
        out, os.path.getsize(out), data["solver_steps"].sum(), data["timesteps"].sum()))


if __name__ == "__main__":
    main()
