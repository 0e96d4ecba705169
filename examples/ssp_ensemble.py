#!/usr/bin/env python3
"""The shipped SSPs as members of ONE core: a scenario x parameter ensemble in one launch, summarised
per scenario by the grouped verbs.  Core.enable_slcf_mixes() lets the mix verb take the aerosol and
ozone / OH precursor emissions, which is what the SSPs differ in besides the always-mixable inputs;
Core.setvar_scenarios(paths, labels) then turns every differing series of SSP1-2.6, SSP2-4.5,
SSP5-8.5 and SSP1-1.9 into one mix with one-hot coefficients, so that a member's inputs are its
scenario's own bits.  Every scenario runs with the SAME sample of the climate sensitivity `S`, the
aerosol forcing scale `aero_scalar`, the respiration sensitivity `q10_rh` and the CO2 fertilisation
`beta`; the member's label is its scenario.

Printed: the 2100 warming band per scenario, the 2100 aerosol and ozone state per scenario, and how
much of the variance of global_tas is BETWEEN the scenarios (eta^2) in 2030, 2050 and 2100.
Needs an MI355X:  python examples/ssp_ensemble.py [members_per_scenario]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric                        # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, AERO_SCALE, GLOBAL_TAS  # noqa: E402

SCENARIOS = ("ssp126", "ssp245", "ssp585", "ssp119")
WARMING = [Metric("mean", (2100, 2100), baseline=(1850, 1900))]


def main(n_per=8192, **core_kwargs):
    G = len(SCENARIOS)
    n = G * n_per
    rng = np.random.default_rng(1)
    S, alpha = rng.uniform(1.5, 6.0, n_per), rng.uniform(0.5, 1.5, n_per)
    q10, beta = rng.uniform(1.0, 3.0, n_per), rng.uniform(0.1, 0.9, n_per)
    data = os.path.dirname(hector_amd.DEFAULT_SCENARIO)
    core = hector_amd.Core(os.path.join(data, "ssp245.hxs"), n, **core_kwargs)
    core.setvar(ECS(), np.tile(S, G), "degC").setvar(AERO_SCALE(), np.tile(alpha, G), "(unitless)")
    core.setvar(Q10_RH(), np.tile(q10, G), "(unitless)").setvar(BETA(), np.tile(beta, G), "(unitless)")
    scenario = np.repeat(np.arange(G), n_per).astype(np.int32)   # the label: which SSP the member runs
    core.set_outputs(["CO2_concentration", "global_tas", "RF_tot", "O3_concentration"])
    core.enable_slcf_mixes()
    nseries = core.setvar_scenarios([os.path.join(data, s + ".hxs") for s in SCENARIOS], scenario)
    core.run(2100)
    assert (core.status() == 0).all()

    band = core.metric_quantiles(GLOBAL_TAS(), WARMING, (0.05, 0.5, 0.95), groups=scenario)   # [G, 1, 3]
    aci = core.fetchvars("RF_aci", (2100, 2100))[0]
    o3 = core.fetchvars("O3_concentration", (2100, 2100))[0]
    print("%d members: %d shipped SSPs x %d parameter sets in one core (%d series mixed, kernel %s/%d, %.2f ms)"
          % (n, G, n_per, nseries, core.last_run_kernel(), core.last_run_variant(), core.last_run_ms()))
    print("  scenario   warming 2100, median (5-95 %)   RF_aci 2100, median   O3 2100, median")
    for g, s in enumerate(SCENARIOS):
        print("  %-9s  %.2f (%.2f-%.2f) K              %8.3f W/m2        %6.2f DU"
              % (s, band[g, 0, 1], band[g, 0, 0], band[g, 0, 2], np.median(aci[scenario == g]),
                 np.median(o3[scenario == g])))
    gm = core.moments(GLOBAL_TAS(), (2030, 2100), groups=scenario)
    print("variance of global_tas: share between the scenarios (eta^2; the rest is parameter spread within them)")
    for y in (2030, 2050, 2100):
        print("  %d  sd %.3f K   between %5.1f %%" % (y, np.sqrt(gm.pooled_var[y - 2030]), 100 * gm.eta2[y - 2030]))
    core.shutdown()
    return band, gm


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
