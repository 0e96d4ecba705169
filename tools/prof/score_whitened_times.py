#!/usr/bin/env python3
"""Wall times of Core.score(..., whiten=W) against Core.score and against the host route it replaces,
by the protocol of profiles/post_summaries.md: a warm core, two untimed calls, then --calls timed calls
(at least 10) of every arm, interleaved round by round in ONE process on the same core; median
(min .. max) in ms, time.perf_counter around the Python call, every result in host memory (the verb
synchronises).  ssp245, S / q10_rh perturbed, 65 536 members, global_tas against 165 annual
pseudo-observations 1850-2014 (a held-out member plus AR(1) noise), baseline 1850-1900, W = whiten of
the AR(1) covariance with rho = 0.6.

    python tools/prof/score_whitened_times.py [--members 65536] [--calls 10] [--json out.json] [--lib lib.so]
    rocprofv3 --kernel-trace --stats -- python tools/prof/score_whitened_times.py --trace-only

Host route (what the parent commit offers): fetchvars of 1745-2014 into a reused buffer, the
baseline and the residuals in numpy, then W @ r (a BLAS dgemm on the host's cores) and the sum of
squares.  The device route's useful flops, n (n + 1) members (the triangle), over its time and the
MI355X fp64 matrix peak (78.6 Tflop/s) is printed as the achieved fraction of the whole call.
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

PEAK = 78.6e12   # fp64 matrix, MI355X


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--lib", help="a differently built library to time")
    ap.add_argument("--trace-only", action="store_true",
                    help="ten calls of the device arms, no timing (for a kernel trace)")
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be at least 10")
    n = a.members
    core = hector_amd.Core(n_members=n, device=0, **({"lib_path": a.lib} if a.lib else {}))
    S, q10 = ensemble.ecs_q10(n)
    core.setvar("S", S, "degC").setvar("q10_rh", q10)
    core.run(2105)
    print("## %d members (%s kernel, run %.1f ms)" % (n, core.last_run_kernel(), core.last_run_ms()), flush=True)
    base = (1850, 1900)
    rng = np.random.default_rng(5)
    cases = {}
    for years in (np.arange(1850, 2015), np.arange(1850, 2106)):
        ny = years.size
        sigma = np.full(ny, 0.1)
        C = sigma[:, None] * sigma[None, :] * 0.6 ** np.abs(years[:, None] - years[None, :])
        W, _ = hector_amd.whiten(C)
        t = core.fetchvars("global_tas", (1745, int(years[-1])))[:, 7]
        e = np.zeros(ny)
        for i in range(ny):
            e[i] = (0.6 * e[i - 1] if i else 0.0) + rng.normal() * 0.1 * (0.8 if i else 1.0)
        obs = t[years - 1745] - t[base[0] - 1745:base[1] - 1745 + 1].mean() + e
        cases[ny] = (years, obs, sigma, W)
    years, obs, sigma, W = cases[165]
    y2, obs2, _, W2 = cases[256]
    buf = np.empty((2014 - 1745 + 1, n))

    def host():
        x = fetch_into(core, "global_tas", buf, (1745, 2014))
        b = x[base[0] - 1745:base[1] - 1745 + 1].mean(axis=0)
        y = W @ ((x[years - 1745] - b) - obs[:, None])
        return np.einsum("ij,ij->j", y, y)

    arms = {
        "score(global_tas, 165 years, whiten=W)": lambda: core.score("global_tas", years, obs, baseline=base, whiten=W),
        "score(global_tas, 165 years, sigma): the independent score": lambda: core.score("global_tas", years, obs, sigma=sigma, baseline=base),
        "host: fetchvars + numpy W @ r, the same chi2": host,
        "host: the fetchvars of it alone": lambda: fetch_into(core, "global_tas", buf, (1745, 2014)),
        "score(global_tas, 256 years, whiten=W)": lambda: core.score("global_tas", y2, obs2, baseline=base, whiten=W2),
        "score(global_tas, 165 years, ar1=0.6, sigma): the factorisation included":
            lambda: core.score("global_tas", years, obs, sigma=sigma, baseline=base, ar1=0.6),
    }
    if a.trace_only:
        for _ in range(10):
            for k in list(arms)[:2] + list(arms)[4:5]:
                arms[k]()
        core.shutdown()
        return
    # the two routes answer the same question
    dev, ref = arms["score(global_tas, 165 years, whiten=W)"](), host()
    print("max |chi2(device) - chi2(host)| / chi2 = %.2e" % np.nanmax(np.abs(dev - ref) / ref))
    w = np.exp(-0.5 * (dev - dev.min()))
    wi = arms["score(global_tas, 165 years, sigma): the independent score"]()
    wi = np.exp(-0.5 * (wi - wi.min()))
    print("effective sample size of exp(-chi2 / 2): AR(1) %.0f, independent %.0f of %d" %
          (w.sum() ** 2 / (w * w).sum(), wi.sum() ** 2 / (wi * wi).sum(), n))
    res = timed(arms, a.calls)
    for k, (med, lo, hi) in res.items():
        print("| %s | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi), flush=True)
    for k, ny in (("score(global_tas, 165 years, whiten=W)", 165), ("score(global_tas, 256 years, whiten=W)", 256)):
        f = float(ny) * (ny + 1) * n
        print("%s: %.3g useful flop, %.2f %% of the fp64 matrix peak over the whole call" %
              (k, f, 100.0 * f / (res[k][0] * 1e-3) / PEAK))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    core.shutdown()


if __name__ == "__main__":
    main()
