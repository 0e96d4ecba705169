#!/usr/bin/env python3
"""What the shipped SSPs as members of one core cost on one MI355X (Core.enable_slcf_mixes,
Core.setvar_scenarios, hx_slcf_mix_kernel).  65 536 members, S / q10_rh perturbed, a core on ssp245 run
1745-2300, one label per member; the scenarios are ssp126 / ssp245 / ssp585 / ssp119 as shipped.

    python tools/prof/slcf_mix_times.py [--members 65536] [--steps 12]

Cores in ONE process take turns, step by step (reset + run + sync each), after two untimed steps each:
  (a) the five carbon-cycle / CH4 names mixed alone: tools/prof/gas_mix_times.py's arm (a), the
      extended kernel with only the mixes every earlier commit has -- the figure to hold against the
      parent commit's, measured by that tool on the parent's tree in the same session
  (b) the four shipped SSPs through setvar_scenarios with the switch on: every differing series,
      the seven aerosol / precursor names among them (7 more rows for the year loop to read)
  (e) four cores of members / 4 each, one per scenario on its own shipped pack, no mix: what (b)
      replaces; the SUM of their last_run_ms per step
last_run_ms of every step is printed, then mean (min .. max).  (c): new coefficients on (b)'s mixes --
the wall time of setvar_scenarios + reset + run + sync minus that run's last_run_ms, and of it the
pre-pass (hx_slcf_mix_kernel with its synchronise) and prepare()'s whole "gas kernel / member series"
stage, read from the library's HECTOR_AMD_TIMING lines."""
import argparse
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gas_mix_times import OLD, SCENARIOS, reduced, stat  # noqa: E402


class Stderr:
    """The process's stderr into a file while the block runs (the library's timing lines)."""

    def __enter__(self):
        self.f = tempfile.TemporaryFile(mode="w+")
        sys.stderr.flush()
        self.keep = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.keep, 2)
        os.close(self.keep)
        self.f.seek(0)
        self.text = self.f.read()
        self.f.close()

    def laps(self, what):
        return [float(x) for x in re.findall(r"\[hector_amd timing\] %s\s+([0-9.]+) ms" % re.escape(what), self.text)]


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
    shipped = [os.path.join(data, s + ".hxs") for s in SCENARIOS]
    tmp = tempfile.mkdtemp(prefix="slcf_mix_times_")
    S, q10 = ensemble.ecs_q10(n)
    labels = np.arange(n) % len(SCENARIOS)

    def core(path, members, who=slice(None)):
        c = hector_amd.Core(path, members, device=0)
        c.setvar("S", S[who], "degC").setvar("q10_rh", q10[who])
        return c

    ca, cb = core(base, n), core(base, n)
    old_paths = [reduced(os.path.join(tmp, s + "_old.hxs"), base, p, OLD) for s, p in zip(SCENARIOS, shipped)]
    na = ca.setvar_scenarios(old_paths, labels)
    nb = cb.enable_slcf_mixes().setvar_scenarios(shipped, labels)
    ce = [core(p, n // len(SCENARIOS), labels == g) for g, p in enumerate(shipped)]
    ms = {"a": [], "b": [], "e": []}

    def step(c):
        c.reset(c.strtdate)
        c.run(2300)
        c.sync()
        return c.last_run_ms()

    for i in range(a.steps + 2):
        t = {"a": step(ca), "b": step(cb), "e": sum(step(c) for c in ce)}
        if i >= 2:
            for k in ms:
                ms[k].append(t[k])
    print("%d members, 1745-2300, %d steps per arm, arms alternating in one process; last_run_ms" % (n, a.steps))
    rows = (("a", "(a) the five old names mixed (%d series)" % na, ca),
            ("b", "(b) setvar_scenarios, the four shipped SSPs (%d series)" % nb, cb),
            ("e", "(e) four cores of %d members, one per SSP, no mix: the sum" % (n // len(SCENARIOS)), ce[0]))
    for k, what, c in rows:
        print("| %s | %s/%d | %s | %s |" % (what, c.last_run_kernel(), c.last_run_variant(), stat(ms[k]),
                                            " ".join("%.3f" % x for x in ms[k])))
    rng = np.random.default_rng(3)
    rest, pre, stage = [], [], []
    os.environ["HECTOR_AMD_TIMING"] = "1"
    for i in range(a.steps):
        w = (labels[None, :] == np.arange(len(SCENARIOS))[:, None]) * rng.uniform(0.9, 1.1, (len(SCENARIOS), n))
        with Stderr() as err:
            t0 = time.perf_counter()
            cb.setvar_scenarios(shipped, w)
            cb.reset(cb.strtdate); cb.run(2300); cb.sync()
            rest.append(1e3 * (time.perf_counter() - t0) - cb.last_run_ms())
        pre.append(sum(err.laps("slcf mix kernel + sync")))
        stage.append(sum(err.laps("gas kernel / member series")))
    del os.environ["HECTOR_AMD_TIMING"]
    print("| (c) new coefficients: setvar_scenarios + reset + run + sync, minus the run kernel | %s | %s |"
          % (stat(rest), " ".join("%.1f" % x for x in rest)))
    print("| ... of it hx_slcf_mix_kernel with its synchronise | %s | %s |" % (stat(pre), " ".join("%.2f" % x for x in pre)))
    print("| ... of it prepare()'s stage 'gas kernel / member series' (both pre-passes, uploads, five tables) | %s | %s |"
          % (stat(stage), " ".join("%.1f" % x for x in stage)))
    for c in [ca, cb] + ce:
        assert (c.status() == 0).all()
        c.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
