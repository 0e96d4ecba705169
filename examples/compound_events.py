#!/usr/bin/env python3
"""Questions that take a whole expression of a member's outputs, asked on the GPU (Core.derive_expr:
one launch, every operand row read once, nothing copied to the host), for a perturbed-parameter
ensemble of SSP2-4.5:

- a compound event.  P(warming >= 2 K AND surface-ocean pH < a threshold) per year: the indicator
  `(dT >= 2.0) & (pH < 8.0)` is a series of 0 / 1, and Core.probabilities of it against the edge 0.5
  is the share of the members in the event.  It is not the product of its margins, which the
  example prints beside it: both follow the same carbon-cycle parameters.
- degree-years of overshoot above 1.5 K: `maximum(dT - 1.5, 0)`, then derive("cumsum") adds it up
  year by year; Core.quantiles gives its band.
- the 2100 warming per kelvin of the member's own equilibrium sensitivity S (a parameter as an
  operand: expr.param), which says how much of the spread S alone explains.

Needs an MI355X:  python examples/compound_events.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import ensemble, expr                # noqa: E402

PARAMS = (("S", 1.5, 6.0, "degC"), ("q10_rh", 1.0, 3.0, "(unitless)"), ("beta", 0.2, 0.8, "(unitless)"),
          ("diff", 1.0, 4.0, "cm2/s"))


def main(n=20000, ph_threshold=8.0, **core_kwargs):
    idx = np.arange(n, dtype=np.uint64)
    core = hector_amd.Core(n_members=n, **core_kwargs)   # packaged SSP2-4.5
    for i, (name, lo, hi, units) in enumerate(PARAMS):
        core.setvar(name, lo + (hi - lo) * ensemble.uniform01(idx, i), units)
    core.set_outputs(["global_tas", "pH"])
    core.run(2100)
    win = (2000, 2100)
    core.derive("dT", "anomaly", "global_tas", years=(1850, 1900))   # warming relative to 1850-1900

    # --- the compound event and its margins, one launch each ---------------------------------------
    core.derive_expr("both", "(dT >= 2.0) & (pH < thr)", {"thr": ph_threshold})
    core.derive_expr("warm", "dT >= 2.0")
    core.derive_expr("acid", "pH < thr", {"thr": ph_threshold})
    p = {k: core.probabilities(k, [0.5], win)[:, 1] for k in ("both", "warm", "acid")}
    print("year   P(dT >= 2 K)   P(pH < %.2f)   P(both)   product of the margins" % ph_threshold)
    for y in range(2020, 2101, 10):
        r = y - win[0]
        print("%d   %11.3f   %12.3f   %7.3f   %7.3f" % (y, p["warm"][r], p["acid"][r], p["both"][r],
                                                        p["warm"][r] * p["acid"][r]))

    # --- degree-years of overshoot above 1.5 K -------------------------------------------------------
    core.derive_expr("over", "maximum(dT - 1.5, 0)")
    core.derive("degyears", "cumsum", "over", years=core.strtdate)
    band = core.quantiles("degyears", (0.05, 0.5, 0.95), win)
    print("degree-years above 1.5 K (5 %, median, 95 %):")
    for y in (2040, 2060, 2080, 2100):
        print("  %d   %7.1f  %7.1f  %7.1f K yr" % ((y,) + tuple(band[y - win[0]])))

    # --- the 2100 warming per kelvin of the member's S ---------------------------------------------------
    core.derive_expr("per_S", "dT / S", {"S": expr.param("S")})
    q = core.quantiles("per_S", (0.05, 0.5, 0.95), (2100, 2100))[0]
    qt = core.quantiles("dT", (0.05, 0.5, 0.95), (2100, 2100))[0]
    print("2100 warming            %.2f  %.2f  %.2f K          (95 %% / 5 %%: %.2f)" % (tuple(qt) + (qt[2] / qt[0],)))
    print("2100 warming per K of S %.3f %.3f %.3f K/K        (95 %% / 5 %%: %.2f)" % (tuple(q) + (q[2] / q[0],)))
    core.shutdown()
    return p, band, q


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
