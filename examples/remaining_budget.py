#!/usr/bin/env python3
"""The remaining carbon budget of every member of a perturbed-parameter ensemble, by bisection on
its own emissions: from 2031 on each member's fossil-fuel and industrial emissions are the
scenario's (SSP2-4.5) times a factor of its own, and the factor is bisected, 20 iterations, until
that member's 2081-2100 warming relative to 1850-1900 is 1.5 K.  The member's budget is what it
then emits from 2031 to 2100.

Every member has its own emission series, yet nothing of n_members x n_years ever exists on the
host: the series is a MIX (Core.setvar_dated_mix) of one shared year-vector, the scenario's
emissions, with one coefficient per member, the factor.  Only that coefficient vector changes
between the iterations -- n_members doubles of upload and one kernel that rewrites the 70 covered
rows of the device table; the warming comes back as one number per member (Core.metrics), and with
the state history on the re-run starts in 2030.
Needs an MI355X:  python examples/remaining_budget.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric                        # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, GLOBAL_TAS, FFI_EMISSIONS  # noqa: E402

TARGET = 1.5                                # K, 2081-2100 above 1850-1900
YEARS = np.arange(2031, 2101)
WARMING = [Metric("mean", (2081, 2100), baseline=(1850, 1900))]
F_MAX = 4.0                                 # the bracket of the factor: 0 .. F_MAX
ITERATIONS = 20
PGC_TO_GTCO2 = 44.0095 / 12.0107


def main(n=10000, **core_kwargs):
    rng = np.random.default_rng(1)
    core = hector_amd.newcore(None, n_members=n, **core_kwargs)   # packaged SSP2-4.5
    hector_amd.setvar(core, None, ECS(), rng.uniform(1.5, 6.0, n), "degC")
    hector_amd.setvar(core, None, Q10_RH(), rng.uniform(1.0, 3.0, n), "(unitless)")
    hector_amd.setvar(core, None, BETA(), rng.uniform(0.1, 0.9, n), "(unitless)")
    core.enable_history(True)               # the re-runs go back to 2030, not to 1745
    scenario = core.fetchvars(FFI_EMISSIONS(), (int(YEARS[0]), int(YEARS[-1])))[:, 0].copy()
    total = float(scenario.sum())           # Pg C, 2031-2100, at factor 1

    def warming(factor):
        core.setvar_dated_mix(FFI_EMISSIONS(), YEARS, scenario, factor, "Pg C/yr")
        core.run(2100)
        return core.metrics(GLOBAL_TAS(), WARMING)[0]

    lo, hi = np.zeros(n), np.full(n, F_MAX)
    w_lo, w_hi = warming(lo), warming(hi)   # the ends of the bracket
    ok = core.status() == 0
    gone = ok & (w_lo >= TARGET)            # above 1.5 K even without any further emissions
    never = ok & (w_hi < TARGET)            # below it even at F_MAX times the scenario
    solve = ok & ~gone & ~never
    for it in range(ITERATIONS):
        mid = 0.5 * (lo + hi)
        above = warming(mid) >= TARGET
        hi = np.where(above, mid, hi)
        lo = np.where(above, lo, mid)
    factor = 0.5 * (lo + hi)
    w = warming(factor)
    budget = factor * total                 # Pg C from 2031 on
    print("%d members; SSP2-4.5 emits %.0f Pg C of fossil carbon 2031-2100" % (n, total))
    print("%d members are above %.1f K without any further emissions, %d stay below it at %.0f times the "
          "scenario, %d ended with an error flag" % (gone.sum(), TARGET, never.sum(), F_MAX, (~ok).sum()))
    # (the model's response has small jumps -- a member's warming can move by 0.01 K between two
    #  neighbouring factors --, so a few members end beside the target, not on it)
    miss = np.abs(w[solve] - TARGET)
    print("the %d others: factor bracketed to %.0e after %d bisections; |warming - %.1f K| median %.1e K, "
          "above 1e-4 K for %d members (largest %.1e K); run %.2f ms"
          % (solve.sum(), F_MAX / 2.0**ITERATIONS, ITERATIONS, TARGET, np.median(miss), (miss > 1e-4).sum(),
             miss.max(), core.last_run_ms()))
    q = np.quantile(np.where(gone, 0.0, budget)[solve | gone], (0.05, 0.5, 0.95))
    print("remaining budget from 2031 for %.1f K in 2081-2100: %.0f (%.0f-%.0f) Pg C = %.0f (%.0f-%.0f) Gt CO2"
          % ((TARGET, q[1], q[0], q[2]) + tuple(PGC_TO_GTCO2 * v for v in (q[1], q[0], q[2]))))
    hector_amd.shutdown(core)
    return factor, budget, (gone, never, solve)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10000)
