#!/usr/bin/env python3
"""Several scenarios in ONE ensemble, summarised per scenario from ONE call each (the groups= keyword
of Core.quantiles / probabilities / moments): four post-2030 emission variants -- the fossil-fuel and
industrial emissions of SSP2-4.5 times 0.25, 0.5, 1 and 1.5 from 2031 on, as mixes
(Core.setvar_dated_mix) -- each run with the SAME sample of the climate sensitivity `S`, the respiration
sensitivity `q10_rh` and the CO2 fertilisation `beta`; the member's label is its scenario.

Printed: the 2100 warming band and P(< 1.5 K), P(1.5-2 K), P(>= 2 K) per scenario; how much of the
variance of global_tas is BETWEEN the scenarios in 2030, 2050 and 2100 and how much within them (the
Hawkins-Sutton partition: scenario against parameter uncertainty); and, with the members labelled by
the decile of `S` instead, the correlation ratio eta^2 of the 2100 warming -- the given-data estimate
of the first-order sensitivity to `S` -- beside the squared standardised regression coefficient of
Core.moments.
Needs an MI355X:  python examples/scenario_groups.py [members_per_scenario]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric                        # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, GLOBAL_TAS, FFI_EMISSIONS  # noqa: E402

FACTORS = (0.25, 0.5, 1.0, 1.5)
YEARS = np.arange(2031, 2101)
WARMING = [Metric("mean", (2100, 2100), baseline=(1850, 1900))]


def main(n_per=8192, **core_kwargs):
    G = len(FACTORS)
    n = G * n_per
    rng = np.random.default_rng(1)
    S, q10, beta = rng.uniform(1.5, 6.0, n_per), rng.uniform(1.0, 3.0, n_per), rng.uniform(0.1, 0.9, n_per)
    core = hector_amd.Core(n_members=n, **core_kwargs)          # packaged SSP2-4.5
    core.setvar(ECS(), np.tile(S, G), "degC").setvar(Q10_RH(), np.tile(q10, G), "(unitless)")
    core.setvar(BETA(), np.tile(beta, G), "(unitless)")
    scenario = np.repeat(np.arange(G), n_per).astype(np.int32)  # the label: which variant the member runs
    ffi = core.fetchvars(FFI_EMISSIONS(), (int(YEARS[0]), int(YEARS[-1])))[:, 0].copy()
    core.setvar_dated_mix(FFI_EMISSIONS(), YEARS, ffi, np.asarray(FACTORS)[scenario], "Pg C/yr")
    core.run(2100)

    band = core.metric_quantiles(GLOBAL_TAS(), WARMING, (0.05, 0.5, 0.95), groups=scenario)       # [G, 1, 3]
    cls = core.metric_probabilities(GLOBAL_TAS(), WARMING, [1.5, 2.0], groups=scenario)           # [G, 1, 3]
    print("%d members: %d scenarios x %d parameter sets; warming in 2100 relative to 1850-1900" % (n, G, n_per))
    print("  emissions x   median (5-95 %)        P(< 1.5 K)  P(1.5-2 K)  P(>= 2 K)")
    for g, f in enumerate(FACTORS):
        print("  %-12.2f  %.2f (%.2f-%.2f) K     %9.3f  %10.3f  %9.3f"
              % ((f, band[g, 0, 1], band[g, 0, 0], band[g, 0, 2]) + tuple(cls[g, 0])))

    gm = core.moments(GLOBAL_TAS(), (2030, 2100), groups=scenario)
    print("variance of global_tas: share between the scenarios (the rest is parameter spread within them)")
    for y in (2030, 2050, 2100):
        print("  %d  sd %.3f K   between %5.1f %%" % (y, np.sqrt(gm.pooled_var[y - 2030]), 100 * gm.eta2[y - 2030]))

    Sm = core.getvar(ECS())
    decile = np.searchsorted(np.quantile(Sm, np.arange(1, 10) / 10.0), Sm, side="right").astype(np.int32)
    by_s = core.metric_moments(GLOBAL_TAS(), WARMING, groups=(decile, 10))
    lin = core.metric_moments(GLOBAL_TAS(), WARMING, against=[ECS(), Q10_RH(), BETA()])
    print("first-order sensitivity of the 2100 warming to S: eta^2 by decile of S %.3f, SRC^2 %.3f"
          % (by_s.eta2[0], lin.src()[0, 0] ** 2))
    core.shutdown()
    return band, cls, gm, by_s


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
