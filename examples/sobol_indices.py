#!/usr/bin/env python3
"""Variance-based (Sobol) sensitivity indices of a perturbed-parameter ensemble, without a trajectory
leaving the GPU (Core.sobol, Core.metric_sobol): which of the climate sensitivity `S`, the respiration
sensitivity `q10_rh`, the CO2 fertilisation `beta` and the ocean heat diffusivity `diff` drives the
spread of the 2100 warming and of the year the warming crosses 2 K -- alone (first-order index) and
with its interactions (total index), from a Saltelli (A, B, AB_i) design.  Beside them the squared
standardised regression coefficients of Core.moments on the same members: what a linear analysis
attributes to each parameter.  Where the model is additive in a parameter the three agree; where the
total index exceeds the first-order one the parameter acts through interactions a regression misses.
Needs an MI355X:  python examples/sobol_indices.py [n_base]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric, ensemble              # noqa: E402

FACTORS = (("S", 1.5, 6.0, "degC"), ("q10_rh", 1.0, 3.0, "(unitless)"), ("beta", 0.2, 0.8, "(unitless)"),
           ("diff", 1.0, 4.0, "cm2/s"))


def main(n_base=4096, **core_kwargs):
    names = [f[0] for f in FACTORS]
    k = len(names)
    u = ensemble.saltelli(n_base, k)                  # [(k + 2) n_base, k]: groups of A_j, B_j, AB_0j .. AB_3j
    core = hector_amd.Core(n_members=u.shape[0], **core_kwargs)   # packaged SSP2-4.5
    for i, (name, lo, hi, units) in enumerate(FACTORS):
        core.setvar(name, lo + (hi - lo) * u[:, i], units)
    core.run(2100)

    specs = [Metric("mean", (2100, 2100), baseline=(1850, 1900)),
             Metric("first_ge", (1850, 2100), baseline=(1850, 1900), threshold=2.0)]
    so = core.metric_sobol("global_tas", specs, names)
    lin = core.metric_moments("global_tas", specs, against=names)
    src2 = lin.src() ** 2
    for row, title in enumerate(("warming in 2100 relative to 1850-1900 (K)", "year the warming crosses 2 K")):
        print("%s: mean %.2f, sd %.2f over %d of %d groups" %
              (title, so.mean[row], np.sqrt(so.var[row]), so.n_part[row], n_base))
        print("  factor     first-order        total              SRC^2")
        for i, name in enumerate(names):
            print("  %-8s %7.4f +- %.4f  %7.4f +- %.4f  %9.4f" %
                  (name, so.first[row, i], so.first_se[row, i], so.total[row, i], so.total_se[row, i], src2[row, i]))
        print("  sum      %7.4f            %7.4f            %9.4f" %
              (so.first[row].sum(), so.total[row].sum(), np.nansum(src2[row])))
    # the same indices year by year: when does the carbon cycle start to matter?
    years = np.arange(2000, 2101, 25)
    ts = core.sobol("global_tas", names, (2000, 2100))
    print("total index of global_tas by year:  " + "  ".join("%8s" % n for n in names))
    for y in years:
        print("  %d                              " % y + "  ".join("%8.4f" % t for t in ts.total[y - 2000]))
    core.shutdown()
    return so, lin


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
