#!/usr/bin/env python3
"""Wall times of Core.sobol against the host route it replaces, by the protocol of
profiles/post_summaries.md: a warm core, two untimed calls, then --calls timed calls (at least 10) of
every arm, interleaved round by round in ONE process on the same core; median (min .. max) in ms,
time.perf_counter around the Python call, every result in host memory (the verb synchronises).
ssp245 to 2100, a Saltelli design of k = 6 factors (S, q10_rh, beta and three dummies), 65 536 members
(n_base = 8192), global_tas over 1850-2100.

    python tools/prof/sobol_times.py [--members 65536] [--k 6] [--calls 10] [--json out.json]
    rocprofv3 --kernel-trace --stats -- python tools/prof/sobol_times.py --trace-only

Three arms: Core.sobol; Core.moments(var, dates) on the same core -- the one-read reduction of the
same rows, a yardstick for what the gathers cost; and the host route (what the parent commit offers):
fetchvars of the window into a reused buffer, then the sums of include/hector_amd.h in numpy.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import hector_amd                                   # noqa: E402
from hector_amd import ensemble                     # noqa: E402
from post_times import fetch_into, timed            # noqa: E402


def host_sobol(x, k, nb):
    """The header's sums on the copied rows, vectorised over the years -> Sobol."""
    ny = x.shape[0]
    g = x[:, :nb * (k + 2)].reshape(ny, nb, k + 2)
    on = ~np.isnan(g).any(axis=2)
    a, b = g[:, :, 0], g[:, :, 1]
    c = np.minimum(np.where(on, a, np.inf).min(axis=1), np.where(on, b, np.inf).min(axis=1))
    dA, dB = np.where(on, a - c[:, None], 0.0), np.where(on, b - c[:, None], 0.0)
    sums = np.empty((ny, 4 + 4 * k))
    sums[:, 0], sums[:, 1], sums[:, 2], sums[:, 3] = dA.sum(1), (dA * dA).sum(1), dB.sum(1), (dB * dB).sum(1)
    for i in range(k):
        t = np.where(on, a - g[:, :, 2 + i], 0.0) ** 2
        u = np.where(on, b - g[:, :, 2 + i], 0.0) ** 2
        sums[:, 4 + 4 * i], sums[:, 5 + 4 * i] = t.sum(1), (t * t).sum(1)
        sums[:, 6 + 4 * i], sums[:, 7 + 4 * i] = u.sum(1), (u * u).sum(1)
    return hector_amd.Sobol(k * [""], np.where(on.any(axis=1), c, np.nan), sums, on.sum(axis=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--trace-only", action="store_true",
                    help="10 calls of the two device arms and nothing else (for a kernel trace)")
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be at least 10")
    n, k = a.members, a.k
    nb = n // (k + 2)
    core = hector_amd.Core(n_members=n, device=0)
    u = np.zeros((n, k))
    u[:nb * (k + 2)] = ensemble.saltelli(nb, k)
    core.setvar("S", 1.5 + 4.5 * u[:, 0], "degC")
    if k > 1:
        core.setvar("q10_rh", 1.0 + 2.0 * u[:, 1])
    if k > 2:
        core.setvar("beta", 0.2 + 0.6 * u[:, 2])
    core.run(2100)
    print("## %d members, k = %d, n_base = %d (%s kernel, run %.1f ms)" %
          (n, k, nb, core.last_run_kernel(), core.last_run_ms()), flush=True)
    win = (1850, 2100)
    buf = np.empty((win[1] - win[0] + 1, n))
    arms = {
        "Core.sobol(global_tas, %d, 1850-2100)" % k: lambda: core.sobol("global_tas", k, win, n_base=nb),
        "Core.moments(global_tas, 1850-2100) on the same core": lambda: core.moments("global_tas", win),
        "host: fetchvars + numpy, the same sums": lambda: host_sobol(fetch_into(core, "global_tas", buf, win), k, nb),
        "host: the fetchvars alone": lambda: fetch_into(core, "global_tas", buf, win),
    }
    if a.trace_only:
        for _ in range(10):
            core.sobol("global_tas", k, win, n_base=nb)
            core.moments("global_tas", win)
        core.shutdown()
        return
    # the two routes answer the same question
    dev, ref = core.sobol("global_tas", k, win, n_base=nb), host_sobol(fetch_into(core, "global_tas", buf, win), k, nb)
    assert np.array_equal(dev.shift, ref.shift) and np.array_equal(dev.n_part, ref.n_part)
    print("max |sums(device) - sums(host)| / sums = %.2e" %
          np.max(np.abs(dev.sums - ref.sums) / np.where(ref.sums > 0, ref.sums, np.inf)))
    print("2100: first %s\n      total %s" % (np.round(dev.first[-1], 4), np.round(dev.total[-1], 4)))
    res = timed(arms, a.calls)
    for key, (med, lo, hi) in res.items():
        print("| %s | %.3f (%.3f .. %.3f) |" % (key, med, lo, hi), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    core.shutdown()


if __name__ == "__main__":
    main()
