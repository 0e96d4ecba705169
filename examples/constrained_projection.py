#!/usr/bin/env python3
"""A constrained projection: run a perturbed-parameter ensemble, score every member against an
observed record, weight the members by their likelihood and report the weighted median and 5-95 %
band -- without a trajectory leaving the GPU (Core.score, Core.quantiles) -- and then what a user
reports: the constrained 2081-2100 warming relative to 1850-1900, the distribution of the
peak-warming year and the probability of the warming classes in 2100 (Core.metric_quantiles,
Core.metric_probabilities), a constrained sea-level band, the crossing year of a 20-year mean and
an emissions what-if on held series (Core.hold, Core.derive), and which parameter drives the 2100
warming before and after the constraint (Core.moments).  The "observations" here are pseudo-observations: one held-out member
plus seeded noise.
Needs an MI355X:  python examples/constrained_projection.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric                        # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, CONCENTRATIONS_CO2, GLOBAL_TAS  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
SIGMA_CO2, SIGMA_TAS = 2.0, 0.12          # ppmv, K: the noise of the pseudo-observations


def main(n=20000, truth=0, **core_kwargs):
    rng = np.random.default_rng(1)
    core = hector_amd.newcore(None, n_members=n, **core_kwargs)   # packaged SSP2-4.5
    hector_amd.setvar(core, None, ECS(), rng.uniform(1.5, 6.0, n), "degC")
    hector_amd.setvar(core, None, Q10_RH(), rng.uniform(1.0, 3.0, n), "(unitless)")
    hector_amd.setvar(core, None, BETA(), rng.uniform(0.1, 0.9, n), "(unitless)")
    hector_amd.run(core, 2100)

    # pseudo-observations: the held-out member's record 1850-2014 plus noise; its temperature as
    # an anomaly relative to 1850-1900, the way observed records come
    years = np.arange(1850, 2015)
    co2 = core.fetchvars(CONCENTRATIONS_CO2(), (1850, 2014))[:, truth]
    tas = core.fetchvars(GLOBAL_TAS(), (1850, 2014))[:, truth]
    obs_co2 = co2 + rng.normal(0.0, SIGMA_CO2, years.size)
    obs_tas = tas - tas[:51].mean() + rng.normal(0.0, SIGMA_TAS, years.size)

    # chi-square of every member, on the device; n_members doubles come back per call
    chi2 = core.score(CONCENTRATIONS_CO2(), years, obs_co2, sigma=SIGMA_CO2)
    chi2 += core.score(GLOBAL_TAS(), years, obs_tas, sigma=SIGMA_TAS, baseline=(1850, 1900))
    ok = core.status() == 0
    ok[truth] = False                                  # held out
    weights = np.where(ok, np.exp(-0.5 * (chi2 - chi2[ok].min())), 0.0)
    n_eff = weights.sum() ** 2 / (weights ** 2).sum()

    for var, unit in ((GLOBAL_TAS(), "K"), (CONCENTRATIONS_CO2(), "ppmv")):
        prior = core.quantiles(var, PROBS, (2100, 2100))[0]
        post = core.quantiles(var, PROBS, (2100, 2100), weights=weights)[0]
        actual = core.fetchvars(var, (2100, 2100))[0, truth]
        print("%-18s 2100  prior %.2f (%.2f-%.2f) %s   constrained %.2f (%.2f-%.2f) %s   held-out member %.2f"
              % (var, prior[1], prior[0], prior[2], unit, post[1], post[0], post[2], unit, actual))
    print("%d members, %d with a model error, effective sample size %.1f, %.1f ms on the GPU"
          % (n, int((core.status() != 0).sum()), n_eff, core.last_run_ms()))
    band = core.quantiles(GLOBAL_TAS(), PROBS, (1850, 2100), weights=weights)   # [251, 3]: the plot

    # a number per member, reduced on the device; only the weighted summaries come back
    base = (1850, 1900)
    specs = [Metric("mean", (2081, 2100), baseline=base), Metric("year_of_max", (1850, 2100), baseline=base)]
    for name, wts in (("prior", None), ("constrained", weights)):
        warm, peak = core.metric_quantiles(GLOBAL_TAS(), specs, PROBS, weights=wts)
        print("%-12s 2081-2100 warming rel. 1850-1900: %.2f (%.2f-%.2f) K   peak-warming year: %d (%d-%d)"
              % (name, warm[1], warm[0], warm[2], peak[1], peak[0], peak[2]))
    classes = core.metric_probabilities(GLOBAL_TAS(), [Metric("mean", 2100, baseline=base)], (1.5, 2.0, 3.0),
                                        weights=weights)[0]
    print("constrained 2100 warming: P(< 1.5 K) %.3f  P(1.5-2 K) %.3f  P(2-3 K) %.3f  P(>= 3 K) %.3f" % tuple(classes))

    # which parameter drives the spread of the 2100 warming, before and after the constraint: the
    # weighted moments and cross moments with the parameters, reduced on the device
    core.derive("warming", "anomaly", GLOBAL_TAS(), years=base)
    drivers = [ECS(), Q10_RH(), BETA()]
    for name, wts in (("prior", None), ("constrained", weights)):
        mom = core.moments("warming", (2100, 2100), weights=wts, against=drivers)
        q = core.quantiles("warming", PROBS, (2100, 2100), weights=wts)[0]
        print("%-12s 2100 warming %.2f +- %.2f K (median %.2f, 5-95 %% %.2f-%.2f)"
              % (name, mom.mean[0], mom.sd[0], q[1], q[0], q[2]))
        print("%-12s   correlation with %s" % ("", "  ".join("%s %+.3f" % (p, r) for p, r in zip(drivers, mom.corr[0]))))
        print("%-12s   SRC              %s" % ("", "  ".join("%s %+.3f" % (p, r) for p, r in zip(drivers, mom.src()[0]))))

    # a diagnostic the core derives on the device takes the same verbs: the constrained sea-level band
    slr = core.quantiles("slr", PROBS, (2100, 2100), weights=weights)[0]
    print("constrained 2100 sea-level rise: %.3f (%.3f-%.3f) m" % (slr[1], slr[0], slr[2]))
    # the year a centred 20-year mean of the warming crosses 1.5 K: two series, composed by name
    core.derive("warming20", "runmean", "warming", width=20, align="centred")
    cross, = core.metric_quantiles("warming20", [Metric("first_ge", (1900, 2090), threshold=1.5)], PROBS,
                                   weights=weights)
    print("constrained crossing year of 1.5 K (20-year mean): %.0f (%.0f-%.0f)" % (cross[1], cross[0], cross[2]))

    # an emissions what-if: hold this run's warming, cut the fossil emissions from 2030 on, run again
    # and summarise the per-member avoided warming -- both trajectories stay on the device
    core.hold("reference_tas", GLOBAL_TAS())
    cut = np.arange(2030, 2101)
    core.setvar_dated("ffi_emissions", cut, np.full(cut.size, 2.0), "Pg C/yr")
    hector_amd.reset(core)
    hector_amd.run(core, 2100)
    core.derive("avoided", "sub", "reference_tas", GLOBAL_TAS())
    avoided = core.quantiles("avoided", PROBS, (2100, 2100), weights=weights)[0]
    classes = core.probabilities("avoided", (0.5, 1.0), (2100, 2100), weights=weights)[0]
    print("constrained avoided warming in 2100: %.2f (%.2f-%.2f) K   P(< 0.5 K) %.3f  P(0.5-1 K) %.3f  P(>= 1 K) %.3f"
          % (avoided[1], avoided[0], avoided[2], classes[0], classes[1], classes[2]))
    hector_amd.shutdown(core)
    return band, weights


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
