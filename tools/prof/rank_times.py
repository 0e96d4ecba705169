#!/usr/bin/env python3
"""Wall times of Core.rank_series, Core.crps and Core.spearman against Core.quantiles of the same rows
and the host route they replace, by the protocol of profiles/post_summaries.md: a warm core, two
untimed calls, then --calls timed calls (at least 10) of every device arm, interleaved round by round
in ONE process on the same core; median (min .. max) in ms, time.perf_counter around the Python call,
every result in host memory or the call synchronised.  ssp245 to 2100, S, q10_rh, beta and diff
varied, 65 536 members, global_tas over 1850-2100, the CRPS over the 165 years 1850-2014.

    python tools/prof/rank_times.py [--members 65536] [--calls 10] [--host-calls 3] [--json out.json]
    rocprofv3 --kernel-trace --stats -- python tools/prof/rank_times.py --trace-only

The host arms (fetchvars, then hector_amd.ensemble.midpit / .crps in numpy) take seconds a call: they
are timed on their own, --host-calls times after one untimed call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import hector_amd                                   # noqa: E402
from hector_amd import Metric, ensemble             # noqa: E402
from post_times import fetch_into, timed            # noqa: E402

PARAMS = ["S", "q10_rh", "beta", "diff"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--trace-only", action="store_true",
                    help="10 calls of the device arms and nothing else (for a kernel trace)")
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be at least 10")
    n = a.members
    i = np.arange(n, dtype=np.uint64)
    core = hector_amd.Core(n_members=n, device=0)
    core.setvar("S", 1.5 + 4.5 * ensemble.uniform01(i, 0), "degC")
    core.setvar("q10_rh", 1.0 + 2.0 * ensemble.uniform01(i, 1))
    core.setvar("beta", 0.2 + 0.6 * ensemble.uniform01(i, 2))
    core.setvar("diff", 0.8 + 2.4 * ensemble.uniform01(i, 3), "cm2/s")
    core.run(2100)
    print("## %d members (%s kernel, run %.1f ms)" % (n, core.last_run_kernel(), core.last_run_ms()), flush=True)
    win = (1850, 2100)
    years = np.arange(1850, 2015)
    obs = 0.1 + 0.007 * (years - 1850) + 0.1 * np.sin(years * 0.7)      # a stand-in record
    chi2 = core.score("global_tas", years, obs, sigma=np.full(years.size, 0.15), baseline=(1850, 1900))
    w = np.exp(-0.5 * (chi2 - np.nanmin(chi2)))
    w[~np.isfinite(w)] = 0.0
    one = [Metric("mean", (2081, 2100), baseline=(1850, 1900))]
    probs = (0.05, 0.25, 0.5, 0.75, 0.95)
    arms = {
        "Core.rank_series(global_tas, 1850-2100)": lambda: core.rank_series("r", "global_tas", win),
        "Core.rank_series, score weights": lambda: core.rank_series("r", "global_tas", win, weights=w),
        "Core.crps(global_tas, 165 years)": lambda: core.crps("global_tas", years, obs, return_pit=True),
        "Core.crps, score weights": lambda: core.crps("global_tas", years, obs, weights=w, return_pit=True),
        "Core.spearman(global_tas, 4 parameters, 1850-2100)": lambda: core.spearman("global_tas", PARAMS, win),
        "Core.moments(global_tas, 4 parameters, 1850-2100) (Pearson)":
            lambda: core.moments("global_tas", win, against=PARAMS),
        "Core.metric_ranks(global_tas, 1 specification)": lambda: core.metric_ranks("global_tas", one),
        "Core.quantiles(global_tas, 5 probabilities, 1850-2100)": lambda: core.quantiles("global_tas", probs, win),
    }
    if a.trace_only:
        for _ in range(10):
            for fn in arms.values():
                fn()
        core.shutdown()
        return
    buf = np.empty((win[1] - win[0] + 1, n))
    # the two routes answer the same question
    x = fetch_into(core, "global_tas", buf, win)
    core.rank_series("r", "global_tas", win, weights=w)
    assert np.array_equal(core.fetchvars("r", (2100, 2100))[0], ensemble.midpit(x[-1], w), equal_nan=True)
    dev = core.crps("global_tas", years[-3:], obs[-3:], weights=w)
    ref = ensemble.crps(x[162:165], obs[-3:], w)
    print("CRPS 2012-2014: device %s numpy %s" % (dev, ref))
    assert np.allclose(dev, ref, rtol=1e-11, atol=0)
    rho, pear = core.spearman("global_tas", PARAMS, (2100, 2100))[0], core.moments(
        "global_tas", (2100, 2100), against=PARAMS).corr[0]
    print("2100: Spearman %s\n      Pearson  %s" % (np.round(rho, 4), np.round(pear, 4)))
    res = timed(arms, a.calls)
    host = {
        "host: the fetchvars alone (1850-2100)": lambda: fetch_into(core, "global_tas", buf, win),
        "host: fetchvars + ensemble.midpit (1850-2100)": lambda: ensemble.midpit(fetch_into(core, "global_tas", buf, win)),
        "host: fetchvars + ensemble.crps (165 years)":
            lambda: ensemble.crps(fetch_into(core, "global_tas", buf[:165], (1850, 2014)), obs),
    }
    for k, fn in host.items():
        fn()
        t = []
        for _ in range(max(a.host_calls, 1)):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        res[k] = (float(np.median(t)), float(min(t)), float(max(t)))
    for key, (med, lo, hi) in res.items():
        print("| %s | %.3f (%.3f .. %.3f) |" % (key, med, lo, hi), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    core.shutdown()


if __name__ == "__main__":
    main()
