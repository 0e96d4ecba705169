#!/usr/bin/env python3
"""Wall times of Core.project against the host route it replaces and against Core.score(whiten=W),
by the protocol of profiles/post_summaries.md: a warm core, two untimed calls, then --calls timed calls
(at least 10) of every arm, interleaved round by round in ONE process on the same core; median
(min .. max) in ms, time.perf_counter around the Python call, every result in host memory (the verb
synchronises).  ssp245 to 2300, S / q10_rh perturbed, 65 536 members, global_tas, baseline 1850-1900,
centre = the ensemble mean of every year, a seeded normal basis: 165 years (1850-2014) x m = 8 and
m = 64, and 556 years (1745-2300) x m = 16.

    python tools/prof/project_times.py [--members 65536] [--calls 10] [--json out.json] [--lib lib.so]
    rocprofv3 --kernel-trace --stats -- python tools/prof/project_times.py --trace-only

Host route (what the parent commit offers): fetchvars of the window (and the reference period) into a
reused buffer, the baseline and the residuals in numpy, then basis @ r (a BLAS dgemm on the host's
cores).  Core.score(whiten=W) at 165 years is the call that reads the same rows.  The device route's
flops, 2 n m members, over its time and the MI355X fp64 matrix peak (78.6 Tflop/s) is printed as the
achieved fraction of the whole call.
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
BASE = (1850, 1900)
SHAPES = ((165, 8), (165, 64), (556, 16))


def into_reused(core, years, B, center, out):
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    yr = np.ascontiguousarray(years, dtype=np.int32)
    args = (core._h, b"global_tas", yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), center.ctypes.data_as(dp),
            B.ctypes.data_as(dp), yr.size, B.shape[0], BASE[0], BASE[1], out.ctypes.data_as(dp))

    def call(keep=(yr, B, center, out)):
        core._ck(core._lib.hx_member_project(*args))
        return out
    return call


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
    core.run(2300)
    print("## %d members (%s kernel, run %.1f ms)" % (n, core.last_run_kernel(), core.last_run_ms()), flush=True)
    rng = np.random.default_rng(6)
    windows = {165: (1850, 2014), 556: (1745, 2300)}
    bufs = {165: np.empty((2014 - 1745 + 1, n)), 556: np.empty((556, n))}
    arms, flops, host_of = {}, {}, {}
    for ny, m in SHAPES:
        y0, y1 = windows[ny]
        years = np.arange(y0, y1 + 1)
        B = rng.normal(size=(m, ny))
        x = fetch_into(core, "global_tas", bufs[ny], (1745, y1))
        center = np.nanmean(x[years - 1745], axis=1) - np.nanmean(x[BASE[0] - 1745:BASE[1] - 1745 + 1])

        def residuals(years=years, center=center, buf=bufs[ny], y1=y1):
            x = fetch_into(core, "global_tas", buf, (1745, y1))
            b = x[BASE[0] - 1745:BASE[1] - 1745 + 1].mean(axis=0)
            return (x[years - 1745] - b) - center[:, None]

        def device(years=years, B=B, center=center):
            return core.project("global_tas", years, B, center=center, baseline=BASE)

        def host(B=B, residuals=residuals):
            return B @ residuals()

        name = "project(global_tas, %d years x %d rows)" % (ny, m)
        host_of[name] = "host: fetchvars + numpy basis @ r, %d years x %d rows" % (ny, m)
        arms[name] = device
        arms[host_of[name]] = host
        flops[name] = 2.0 * ny * m * n
        if ny == 165:
            center165 = center
        if m == 64:
            # Core.project returns a new [m, n_members] array every call (here 32 MiB, first touched
            # by the copy); a loop that keeps its result buffer calls the C ABI as this arm does
            arms["hx_member_project into a reused buffer, %d years x %d rows" % (ny, m)] = \
                into_reused(core, years, B, center, np.empty((m, n)))
        # the two routes answer the same question
        scale = np.abs(B) @ np.abs(residuals())
        print("%s: max |device - host| / s_j = %.2e" % (name, float(np.nanmax(np.abs(device() - host()) / scale))), flush=True)
    years = np.arange(1850, 2015)
    W = hector_amd.whiten(0.01 * 0.6 ** np.abs(years[:, None] - years[None, :]))[0]
    obs = center165
    arms["score(global_tas, 165 years, whiten=W): reads the same rows"] = \
        lambda: core.score("global_tas", years, obs, baseline=BASE, whiten=W)
    arms["host: the fetchvars of 1745-2014 alone"] = lambda: fetch_into(core, "global_tas", bufs[165], (1745, 2014))
    if a.trace_only:
        for _ in range(10):
            for k in arms:
                if not k.startswith("host"):
                    arms[k]()
        core.shutdown()
        return
    res = timed(arms, a.calls)
    for k, (med, lo, hi) in res.items():
        print("| %s | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi), flush=True)
    for k, f in flops.items():
        print("%s: %.3g flop, %.2f %% of the fp64 matrix peak over the whole call; device / host median %.3f"
              % (k, f, 100.0 * f / (res[k][0] * 1e-3) / PEAK, res[k][0] / res[host_of[k]][0]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    core.shutdown()


if __name__ == "__main__":
    main()
