#!/usr/bin/env python3
"""What whole scenarios as members cost on one MI355X (Core.setvar_scenarios, hx_gas_mix_kernel).
65 536 members, S / q10_rh perturbed, a core on ssp245 run 1745-2300; the scenarios are the shipped
ssp126 / ssp245 / ssp585 / ssp119 reduced to their mixable series (tests/test_member_gas_mix.py does
the same), one label per member.

    python tools/prof/gas_mix_times.py [--members 65536] [--steps 12]

Three cores live in ONE process and take turns, step by step (reset + run + sync each), after two
untimed steps each:
  (a) the five carbon-cycle / CH4 names mixed alone (what every earlier commit can do)
  (b) the full setvar_scenarios: those five, N2O_emissions, RF_albedo and the halocarbons
  (d) a CO2-constrained core without any mix (the extended kernel flavour)
last_run_ms of every step is printed, then mean (min .. max).  (c): the wall time of
setvar_scenarios + reset + run + sync minus that run's last_run_ms -- everything but the run kernel:
recipe upload, the gas pre-pass, the five tables -- for new coefficients on an existing set of mixes,
and for the first call after clear_mix of every name."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
OLD = ["ffi_emissions", "daccs_uptake", "luc_emissions", "luc_uptake", "CH4_emissions"]
SCENARIOS = ["ssp126", "ssp245", "ssp585", "ssp119"]


def series_lines(path):
    out = {}
    with open(path) as f:
        for line in f:
            p = line.split(None, 3)
            if len(p) > 3 and p[0] == "series":
                out[(p[1], p[2])] = line
    return out


def reduced(path, base, donor, take):
    theirs = {k: v for k, v in series_lines(donor).items() if k[1] in take}
    with open(base) as f, open(path, "w") as g:
        for line in f:
            p = line.split(None, 3)
            if len(p) > 3 and p[0] == "series" and (p[1], p[2]) in theirs:
                line = theirs[(p[1], p[2])]
            g.write(line)
    return path


def stat(v):
    return "%.3f (%.3f .. %.3f)" % (np.mean(v), np.min(v), np.max(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=12)
    a = ap.parse_args()
    import hector_amd
    from hector_amd import ensemble
    n = a.members
    data = os.path.dirname(hector_amd.DEFAULT_SCENARIO)
    base = os.path.join(data, "ssp245.hxs")
    tmp = tempfile.mkdtemp(prefix="gas_mix_times_")
    S, q10 = ensemble.ecs_q10(n)
    labels = np.arange(n) % len(SCENARIOS)

    def core():
        c = hector_amd.Core(base, n, device=0)
        c.setvar("S", S, "degC").setvar("q10_rh", q10)
        return c

    ca, cb, cd = core(), core(), core()
    full = cb.mix_capabilities()
    old_paths = [reduced(os.path.join(tmp, s + "_old.hxs"), base, os.path.join(data, s + ".hxs"), OLD) for s in SCENARIOS]
    all_paths = [reduced(os.path.join(tmp, s + "_all.hxs"), base, os.path.join(data, s + ".hxs"), full) for s in SCENARIOS]
    na, nb = ca.setvar_scenarios(old_paths, labels), cb.setvar_scenarios(all_paths, labels)
    y = np.arange(1850, 2015)
    probe = hector_amd.Core(base, 64, device=0)
    probe.run(2015)
    cd.setvar_dated("CO2_constrain", y, 1.05 * probe.fetchvars("CO2_concentration", (1850, 2014))[:, 0], "ppmv CO2")
    probe.shutdown()
    arms = {"a": ca, "b": cb, "d": cd}
    ms = {k: [] for k in arms}
    for step in range(a.steps + 2):
        for k, c in arms.items():
            c.reset(c.strtdate)
            c.run(2300)
            c.sync()
            if step >= 2:
                ms[k].append(c.last_run_ms())
    print("%d members, 1745-2300, %d steps per arm, arms alternating in one process; last_run_ms" % (n, a.steps))
    what = {"a": "(a) the five old names mixed (%d series)" % na, "b": "(b) setvar_scenarios, four scenarios (%d series)" % nb,
            "d": "(d) CO2-constrained, no mix"}
    for k, c in arms.items():
        print("| %s | %s/%d | %s | %s |" % (what[k], c.last_run_kernel(), c.last_run_variant(), stat(ms[k]),
                                            " ".join("%.3f" % x for x in ms[k])))
    rng = np.random.default_rng(3)
    new, first = [], []
    for step in range(a.steps):
        w = (labels[None, :] == np.arange(len(SCENARIOS))[:, None]) * rng.uniform(0.9, 1.1, (len(SCENARIOS), n))
        t0 = time.perf_counter()
        cb.setvar_scenarios(all_paths, w)
        cb.reset(cb.strtdate); cb.run(2300); cb.sync()
        new.append(1e3 * (time.perf_counter() - t0) - cb.last_run_ms())
    for step in range(max(3, a.steps // 4)):
        for name in full:
            cb.clear_mix(name)
        cb.run(2300); cb.sync()
        t0 = time.perf_counter()
        cb.setvar_scenarios(all_paths, labels)
        cb.reset(cb.strtdate); cb.run(2300); cb.sync()
        first.append(1e3 * (time.perf_counter() - t0) - cb.last_run_ms())
    print("| (c) new coefficients: setvar_scenarios + reset + run + sync, minus the run kernel | %s | %s |"
          % (stat(new), " ".join("%.1f" % x for x in new)))
    print("| (c) the first call after clear_mix of every name, likewise | %s | %s |"
          % (stat(first), " ".join("%.1f" % x for x in first)))
    for c in arms.values():
        assert (c.status() == 0).all()
        c.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
