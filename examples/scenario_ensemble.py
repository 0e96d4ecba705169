#!/usr/bin/env python3
"""All eight shipped SSPs x one parameter draw in ONE core (Core.setvar_scenarios), summarised per
scenario through groups=.

What a member can hold of "its" scenario today is every MIXABLE input: the carbon-cycle and CH4
emissions, N2O_emissions, RF_albedo and the halocarbons' emissions.  The aerosol emissions and the
ozone / OH precursors cannot be mixed yet, so the shipped packs are refused against each other (the
message is printed first) and every member keeps SSP2-4.5's aerosols and precursors: the scenarios
run here are the shipped ones reduced to their mixable series, written next to each other in a
temporary folder.

Printed: the 2100 warming band per scenario; the share of the variance of global_tas that lies
BETWEEN the scenarios in 2050 and 2100 -- once with every mixable input per scenario, once with only
the five carbon-cycle / CH4 names (what the mix verb took before N2O, albedo and the halocarbons):
the difference is the error that closing those inputs removes.
Needs an MI355X:  python examples/scenario_ensemble.py [members_per_scenario]"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric                        # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, GLOBAL_TAS  # noqa: E402

SSPS = ("ssp119", "ssp126", "ssp245", "ssp370", "ssp434", "ssp460", "ssp534-over", "ssp585")
OLD = ("ffi_emissions", "daccs_uptake", "luc_emissions", "luc_uptake", "CH4_emissions")
WARMING = [Metric("mean", (2100, 2100), baseline=(1850, 1900))]


def reduced(path, base, donor, take):
    """`base` with the series named in `take` from `donor` (its own text lines: its own bits)."""
    theirs = {}
    with open(donor) as f:
        for line in f:
            p = line.split(None, 3)
            if len(p) > 3 and p[0] == "series" and p[2] in take:
                theirs[(p[1], p[2])] = line
    with open(base) as f, open(path, "w") as g:
        for line in f:
            p = line.split(None, 3)
            g.write(theirs.get((p[1], p[2]), line) if len(p) > 3 and p[0] == "series" else line)
    return path


def ensemble(paths, n_per, rng, **core_kwargs):
    G = len(paths)
    S, q10, beta = rng.uniform(1.5, 6.0, n_per), rng.uniform(1.0, 3.0, n_per), rng.uniform(0.1, 0.9, n_per)
    core = hector_amd.Core(n_members=G * n_per, **core_kwargs)   # packaged SSP2-4.5
    core.setvar(ECS(), np.tile(S, G), "degC").setvar(Q10_RH(), np.tile(q10, G), "(unitless)")
    core.setvar(BETA(), np.tile(beta, G), "(unitless)")
    scenario = np.repeat(np.arange(G), n_per).astype(np.int32)
    nseries = core.setvar_scenarios(paths, scenario)
    core.run(2100)
    band = core.metric_quantiles(GLOBAL_TAS(), WARMING, (0.05, 0.5, 0.95), groups=scenario)
    gm = core.moments(GLOBAL_TAS(), (2050, 2100), groups=scenario)
    core.shutdown()
    return nseries, band, gm


def main(n_per=4096, **core_kwargs):
    data = os.path.dirname(hector_amd.DEFAULT_SCENARIO)
    base = os.path.join(data, "ssp245.hxs")
    shipped = [os.path.join(data, s + ".hxs") for s in SSPS]
    probe = hector_amd.Core(n_members=len(SSPS), **core_kwargs)
    mixable = probe.mix_capabilities()
    try:
        probe.setvar_scenarios(shipped, np.arange(len(SSPS)))
    except hector_amd.HectorAmdError as e:
        print("the shipped packs as they are:", str(e)[:400])
    probe.shutdown()
    out = {}
    with tempfile.TemporaryDirectory(prefix="scenario_ensemble_") as tmp:
        for what, take in (("all mixable inputs", mixable), ("the five carbon-cycle / CH4 names only", OLD)):
            paths = [reduced(os.path.join(tmp, "%s_%d.hxs" % (s, len(take))), base, p, set(take))
                     for s, p in zip(SSPS, shipped)]
            out[what] = ensemble(paths, n_per, np.random.default_rng(1), **core_kwargs)
    for what, (nseries, band, gm) in out.items():
        print("%s: %d series mixed, %d scenarios x %d parameter sets; warming in 2100 relative to 1850-1900"
              % (what, nseries, len(SSPS), n_per))
        for g, s in enumerate(SSPS):
            print("  %-12s  %.2f (%.2f-%.2f) K" % (s, band[g, 0, 1], band[g, 0, 0], band[g, 0, 2]))
        for y in (2050, 2100):
            print("  %d  sd of global_tas %.3f K   between the scenarios %5.1f %%"
                  % (y, np.sqrt(gm.pooled_var[y - 2050]), 100 * gm.eta2[y - 2050]))
    return out


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
