#!/usr/bin/env python3
"""Wall times of Core.pair_metrics against the one-operand Core.metrics and against the host route it
replaces, by the protocol of profiles/post_summaries.md: a warm core, two untimed calls, then --calls
timed calls (at least 10) of every arm, interleaved round by round in ONE process on the same core;
median (min .. max) in ms, time.perf_counter around the Python call, every result in host memory (the
verb synchronises).  ssp245 to 2100, S / q10_rh perturbed, 65 536 members, a = global_tas,
b = CO2_concentration, the window 1850-2100.

    python tools/prof/pair_metric_times.py [--members 65536] [--calls 10] [--json out.json] [--lib lib.so]
    rocprofv3 --kernel-trace --stats -- python tools/prof/pair_metric_times.py --trace-only

Arms: one `slope` and eight mixed specifications (with a variable b and with a per-year vector b); the
parent's Core.metrics(Metric("slope")) on the same window -- one operand, one pass; and the host route
(what the parent commit offers): fetchvars of both variables into reused buffers plus the numpy
restatement of the slope.  The ONE timing condition: a `slope` call takes less time than fetchvars of
one of the two variables alone; it is printed and decides the exit status.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import hector_amd                                   # noqa: E402
from hector_amd import Metric, PairMetric, ensemble  # noqa: E402
from post_times import fetch_into, timed            # noqa: E402

WIN = (1850, 2100)
BASE = (1850, 1900)
A, B = "global_tas", "CO2_concentration"


def numpy_slope(xa, xb):
    """The header's two passes on the copied rows, vectorised over the members."""
    n = float(xa.shape[0])
    sa, sb = np.zeros(xa.shape[1]), np.zeros(xa.shape[1])
    for y in range(xa.shape[0]):
        sa = sa + xa[y]
        sb = sb + xb[y]
    ma, mb = sa / n, sb / n
    sab, sbb = np.zeros(xa.shape[1]), np.zeros(xa.shape[1])
    for y in range(xa.shape[0]):
        da, db = xa[y] - ma, xb[y] - mb
        sab = sab + db * da
        sbb = sbb + db * db
    return sab / sbb


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
    core.run(2100)
    print("## %d members (%s kernel, run %.1f ms)" % (n, core.last_run_kernel(), core.last_run_ms()), flush=True)
    ny = WIN[1] - WIN[0] + 1
    ba, bb = np.empty((ny, n)), np.empty((ny, n))
    years = np.arange(WIN[0], WIN[1] + 1)
    vec = (years, np.cumsum(np.linspace(0.5, 12.0, ny)))
    slope = [PairMetric("slope", WIN)]
    eight = [PairMetric("slope", WIN, baseline=BASE), PairMetric("intercept", WIN, baseline=BASE),
             PairMetric("r2", WIN), PairMetric("at_first_ge", WIN, threshold=450.0),
             PairMetric("at_max", WIN, baseline=BASE), PairMetric("at_min", (1900, 2000)),
             PairMetric("mean_where_ge", WIN, baseline=BASE, threshold=500.0), PairMetric("end_ratio", WIN, baseline=BASE)]

    def host():
        return numpy_slope(fetch_into(core, A, ba, WIN), fetch_into(core, B, bb, WIN))

    arms = {
        "pair_metrics(global_tas, CO2_concentration, one slope 1850-2100)": lambda: core.pair_metrics(A, B, slope),
        "pair_metrics(global_tas, CO2_concentration, eight mixed specifications)": lambda: core.pair_metrics(A, B, eight),
        "pair_metrics(global_tas, a per-year vector, one slope)": lambda: core.pair_metrics(A, vec, slope),
        "pair_metrics(global_tas, a per-year vector, eight mixed specifications)": lambda: core.pair_metrics(A, vec, eight),
        "metrics(global_tas, Metric(slope) 1850-2100): one operand, one pass": lambda: core.metrics(A, [Metric("slope", WIN)]),
        "host: fetchvars of both variables + the numpy restatement of the slope": host,
        "host: the fetchvars of global_tas alone": lambda: fetch_into(core, A, ba, WIN),
        "host: the fetchvars of CO2_concentration alone": lambda: fetch_into(core, B, bb, WIN),
    }
    keys = list(arms)
    # the two routes answer the same question, bit for bit
    same = np.array_equal(core.pair_metrics(A, B, slope)[0], host(), equal_nan=True)
    print("device slope == numpy restatement on fetchvars output, bit for bit: %s" % same, flush=True)
    if a.trace_only:
        for _ in range(10):
            for k in keys[:5]:
                arms[k]()
        core.shutdown()
        return 0
    res = timed(arms, a.calls)
    for k, (med, lo, hi) in res.items():
        print("| %s | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi), flush=True)
    one, fetch = res[keys[0]][0], min(res[keys[6]][0], res[keys[7]][0])
    held = one < fetch
    print("the timing condition -- one slope call (%.3f ms) below fetchvars of one variable alone (%.3f ms): %s, "
          "a factor of %.1f" % (one, fetch, "holds" if held else "MISSED", fetch / one))
    # the byte model: a, b read in two passes (no reference period) against one block over the host link
    blk = 8.0 * ny * n
    print("bytes: the slope kernel reads 4 x %.1f MB from HBM / L2, a fetch moves %.1f MB to the host" % (blk / 1e6, blk / 1e6))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(res, condition_holds=bool(held), bitwise=bool(same)), f, indent=1)
    core.shutdown()
    return 0 if held and same else 1


if __name__ == "__main__":
    sys.exit(main())
