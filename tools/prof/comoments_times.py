#!/usr/bin/env python3
"""Wall times of Core.comoments against the host route it replaces, by the protocol of
profiles/post_summaries.md: a warm core, two untimed calls, then --calls timed calls (at least 10) of
every arm, interleaved round by round in ONE process on the same core; median (min .. max) in ms,
time.perf_counter around the Python call, every result in host memory (the verb synchronises).
ssp245, S / q10_rh perturbed, 65 536 members, weights = exp(-chi2 / 2) of a CO2 score.

    python tools/prof/comoments_times.py [--members 65536] [--calls 10] [--json out.json] [--lib lib.so]

Two cases: the symmetric 1850-2100 matrix of global_tas (251 x 251), and global_tas 1980-2020 against
global_tas 2050-2100 (41 x 51).  Host route (what the parent commit offers): fetchvars of the
window(s) into reused buffers, then the weighted X_a^T diag(q) X_b about the weighted means in numpy
(a BLAS dgemm on the host's cores).  The device route's flops, 2 na nb n (in the symmetric call: those
of the 32 x 32 quadrants it computes, 36 of 64 for 251 rows), over its time and the MI355X fp64 matrix peak (78.6 Tflop/s) is
printed as the achieved fraction -- of the whole call, host work and copies included.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import hector_amd                                   # noqa: E402
from hector_amd import ensemble                     # noqa: E402
from post_times import fetch_into, score_weights, timed   # noqa: E402

PEAK = 78.6e12   # fp64 matrix, MI355X


def host_gram(xa, xb, w):
    """The weighted covariance of the copied rows: complete cases, weighted means, one dgemm."""
    ok = (w > 0) & ~np.isnan(xa).any(axis=0) & ~np.isnan(xb).any(axis=0)
    wn = w[ok] / w[ok].sum()
    a = xa[:, ok] - (xa[:, ok] @ wn)[:, None]
    b = a if xb is xa else xb[:, ok] - (xb[:, ok] @ wn)[:, None]
    return (a * wn) @ b.T


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--lib", help="a differently built library to time (A/B of the kernel's constants)")
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be at least 10")
    n = a.members
    core = hector_amd.Core(n_members=n, device=0, **({"lib_path": a.lib} if a.lib else {}))
    S, q10 = ensemble.ecs_q10(n)
    core.setvar("S", S, "degC").setvar("q10_rh", q10)
    core.run(2100)
    w = score_weights(core)
    print("## %d members (%s kernel, run %.1f ms)" % (n, core.last_run_kernel(), core.last_run_ms()), flush=True)
    sym, obs, fut = (1850, 2100), (1980, 2020), (2050, 2100)
    bs, bo, bf = (np.empty((y[1] - y[0] + 1, n)) for y in (sym, obs, fut))

    def host_sym():
        x = fetch_into(core, "global_tas", bs, sym)
        return host_gram(x, x, w)

    def host_cross():
        return host_gram(fetch_into(core, "global_tas", bo, obs), fetch_into(core, "global_tas", bf, fut), w)

    arms = {
        "comoments(global_tas, 1850-2100), symmetric, weighted": lambda: core.comoments("global_tas", sym, weights=w),
        "host: fetchvars + numpy, the same matrix": host_sym,
        "host: the fetchvars of it alone": lambda: fetch_into(core, "global_tas", bs, sym),
        "comoments(global_tas 1980-2020 x global_tas 2050-2100), weighted":
            lambda: core.comoments("global_tas", obs, "global_tas", fut, weights=w),
        "host: two fetchvars + numpy, the same matrix": host_cross,
        "host: the two fetchvars alone": lambda: (fetch_into(core, "global_tas", bo, obs),
                                                  fetch_into(core, "global_tas", bf, fut)),
    }
    # the two routes answer the same question
    cm = core.comoments("global_tas", sym, weights=w)
    ref = host_sym()
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    print("max |cov(device) - cov(host)| / sqrt(var_a var_b) = %.2e" % np.nanmax(np.abs(cm.cov - ref) / np.where(scale > 0, scale, np.nan)))
    res = timed(arms, a.calls)
    for k, (med, lo, hi) in res.items():
        print("| %s | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi), flush=True)
    keys = list(arms)
    blocks = (251 + 63) // 64
    # issued: 32 x 32 quadrants of the 64 x 64 blocks on or above the diagonal, less the diagonal blocks' lower one
    flops = {keys[0]: 2.0 * n * 32 * 32 * (4 * (blocks * (blocks + 1) // 2) - blocks), keys[3]: 2.0 * n * 41 * 51}
    for k, f in flops.items():
        print("%s: %.3g flop issued, %.2f %% of the fp64 matrix peak over the whole call" %
              (k, f, 100.0 * f / (res[k][0] * 1e-3) / PEAK))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    core.shutdown()


if __name__ == "__main__":
    main()
