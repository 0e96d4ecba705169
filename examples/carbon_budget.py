#!/usr/bin/env python3
"""The carbon-budget questions of a perturbed-parameter ensemble, each of which relates TWO series of
the same member (Core.pair_metrics and its ensemble-wide siblings): every member's TCRE -- the slope of
its warming on the cumulative CO2 emissions --, the CO2 concentration and the cumulative emissions in
the year its 1850-1900 anomaly first reaches 1.5 K and 2 K (the remaining-budget question), and their
prior and score-weighted bands and class probabilities.  No trajectory leaves the GPU: one number per
member comes back from pair_metrics, a handful per question from the ensemble-wide verbs.  The
"observations" are pseudo-observations: one held-out member plus seeded noise.
Needs an MI355X:  python examples/carbon_budget.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import PairMetric                    # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, CONCENTRATIONS_CO2, GLOBAL_TAS  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
SIGMA_CO2, SIGMA_TAS = 2.0, 0.12          # ppmv, K: the noise of the pseudo-observations
BASE = (1850, 1900)
LEVELS = (1.5, 2.0)                       # K above 1850-1900


def main(n=20000, truth=0, **core_kwargs):
    rng = np.random.default_rng(1)
    core = hector_amd.newcore(None, n_members=n, **core_kwargs)   # packaged SSP2-4.5
    hector_amd.setvar(core, None, ECS(), rng.uniform(1.5, 6.0, n), "degC")
    hector_amd.setvar(core, None, Q10_RH(), rng.uniform(1.0, 3.0, n), "(unitless)")
    hector_amd.setvar(core, None, BETA(), rng.uniform(0.1, 0.9, n), "(unitless)")
    hector_amd.run(core, 2100)

    # the likelihood weights of examples/constrained_projection.py: CO2 and the warming 1850-2014
    years = np.arange(1850, 2015)
    co2 = core.fetchvars(CONCENTRATIONS_CO2(), (1850, 2014))[:, truth]
    tas = core.fetchvars(GLOBAL_TAS(), (1850, 2014))[:, truth]
    obs_co2 = co2 + rng.normal(0.0, SIGMA_CO2, years.size)
    obs_tas = tas - tas[:51].mean() + rng.normal(0.0, SIGMA_TAS, years.size)
    chi2 = core.score(CONCENTRATIONS_CO2(), years, obs_co2, sigma=SIGMA_CO2)
    chi2 += core.score(GLOBAL_TAS(), years, obs_tas, sigma=SIGMA_TAS, baseline=BASE)
    ok = core.status() == 0
    ok[truth] = False                                  # held out
    weights = np.where(ok, np.exp(-0.5 * (chi2 - chi2[ok].min())), 0.0)

    # cumulative CO2 emissions since 1850, Pg C: a scenario input, the same for every member -- the
    # vector operand of the pair verbs
    span = np.arange(1850, 2101)
    emitted = core.fetchvars("ffi_emissions", (1850, 2100))[:, 0] + core.fetchvars("luc_emissions", (1850, 2100))[:, 0]
    cumulative = (span, np.cumsum(emitted))

    # TCRE: each member's regression of its warming (all forcings, as the scenario has them) on the
    # cumulative emissions while they grow
    window = (1850, int(span[np.argmax(cumulative[1])]))
    tcre_spec = [PairMetric("slope", window, baseline=BASE), PairMetric("r2", window, baseline=BASE)]
    tcre, r2 = core.pair_metrics(GLOBAL_TAS(), cumulative, tcre_spec)
    tcre *= 1000.0                                     # K per 1000 Pg C
    print("TCRE of the first members: %s K / 1000 Pg C (r2 %s)"
          % (" ".join("%.2f" % v for v in tcre[:5]), " ".join("%.3f" % v for v in r2[:5])))
    bands = {}
    for name, wts in (("prior", None), ("constrained", weights)):
        q = core.pair_metric_quantiles(GLOBAL_TAS(), cumulative, tcre_spec[:1], PROBS, weights=wts)[0] * 1000.0
        p = core.pair_metric_probabilities(GLOBAL_TAS(), cumulative, tcre_spec[:1], (2.0e-3, 3.0e-3, 4.0e-3), weights=wts)[0]
        bands[name] = q
        print("%-12s TCRE %.2f (%.2f-%.2f) K / 1000 Pg C   P(< 2) %.3f  P(2-3) %.3f  P(3-4) %.3f  P(>= 4) %.3f"
              % ((name, q[1], q[0], q[2]) + tuple(p)))

    # the CO2 concentration in the year the 1850-1900 anomaly first reaches 1.5 K and 2 K ...
    cross = [PairMetric("at_first_ge", (1850, 2100), baseline_b=BASE, threshold=level) for level in LEVELS]
    crossing = core.pair_metrics(CONCENTRATIONS_CO2(), GLOBAL_TAS(), cross)
    # ... and the emissions until then -- the budget: the cumulative vector as a per-member series
    core.derive("cumulative_emissions", "mul", GLOBAL_TAS(), 0.0)
    core.derive("cumulative_emissions", "add", "cumulative_emissions", cumulative[1], first_year=1850)
    for name, wts in (("prior", None), ("constrained", weights)):
        conc, n_conc = core.pair_metric_quantiles(CONCENTRATIONS_CO2(), GLOBAL_TAS(), cross, PROBS, weights=wts, counts=True)
        budget = core.pair_metric_quantiles("cumulative_emissions", GLOBAL_TAS(), cross, PROBS, weights=wts)
        reach = core.pair_metric_probabilities(CONCENTRATIONS_CO2(), GLOBAL_TAS(), cross, (450.0, 500.0), weights=wts)
        for k, level in enumerate(LEVELS):
            print("%-12s %.1f K reached by %d members at %.0f (%.0f-%.0f) ppmv CO2, after %.0f (%.0f-%.0f) Pg C;"
                  "  P(< 450 ppmv) %.3f  P(450-500) %.3f  P(>= 500) %.3f"
                  % ((name, level, n_conc[k], conc[k][1], conc[k][0], conc[k][2], budget[k][1], budget[k][0],
                      budget[k][2]) + tuple(reach[k])))
    # which parameter decides the concentration at 1.5 K, before and after the constraint
    drivers = [ECS(), Q10_RH(), BETA()]
    for name, wts in (("prior", None), ("constrained", weights)):
        mom = core.pair_metric_moments(CONCENTRATIONS_CO2(), GLOBAL_TAS(), cross[:1], weights=wts, against=drivers)
        print("%-12s CO2 at 1.5 K: %.1f +- %.1f ppmv   correlation with %s"
              % (name, mom.mean[0], mom.sd[0], "  ".join("%s %+.3f" % (p, r) for p, r in zip(drivers, mom.corr[0]))))
    hector_amd.shutdown(core)
    return tcre, crossing, bands


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
