#!/usr/bin/env python3
"""Wall times of the summary verbs, by the protocol of profiles/post_summaries.md: a warm core, two
untimed calls, then --calls timed calls (at least 15) of every arm, the arms interleaved round by
round in ONE process on the same core, the order of the arms rotated from round to round; median (min .. max) in ms, time.perf_counter around the Python
call, result in host memory.  ssp245, S / q10_rh / beta perturbed, 1745-2300.

    python tools/prof/post_times.py                       # every group, 65 536 and 131 072 members
    python tools/prof/post_times.py --groups moments --members 65536 --json out.json
    python tools/prof/post_times.py --groups moments --members 65536 --trace-only
        (ten calls of each moments arm and nothing else: what to put behind
         `rocprofv3 --kernel-trace --stats --` for kernel times)

Groups: moments (Core.moments with npred 0 / 3 / 8 against the fetchvars copy it replaces and the
numpy reduction of the copied rows), quantiles, metrics (metrics, probabilities, metric_quantiles,
metric_probabilities), series (derive + quantiles against two copies; sub, cumsum, runmean alone).
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

PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
PARAMS = ["S", "q10_rh", "beta"]
SPAN = (1745, 2300)


def make_core(n):
    core = hector_amd.Core(n_members=n, device=0)
    S, q10 = ensemble.ecs_q10(n)
    core.setvar("S", S, "degC").setvar("q10_rh", q10)
    core.setvar("beta", 0.2 + 0.6 * np.fmod(np.arange(n) * 0.7548776662466927, 1.0))
    core.run(2300)
    return core


def score_weights(core):
    years = np.arange(1850, 2015)
    rng = np.random.default_rng(5)
    truth = core.fetchvars("CO2_concentration", (1850, 2014))[:, 0]
    obs = truth + rng.normal(0.0, 1.0, years.size)
    chi2 = core.score("CO2_concentration", years, obs, sigma=np.full(years.size, 4.0))
    w = np.exp(-0.5 * (chi2 - chi2.min()))
    w[core.status() != 0] = 0.0
    return w


def fetch_into(core, var, buf, span=SPAN):
    """hx_fetchvars into a reused buffer (Core.fetchvars allocates a new one every call)."""
    import ctypes
    core._ck(core._lib.hx_fetchvars(core._h, var.encode(), span[0], span[1],
                                    buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return buf


def timed(arms, calls):
    """arms: {name: callable} -> {name: (median, min, max)} in ms, interleaved round by round."""
    for _ in range(2):
        for fn in arms.values():
            fn()
    t = {k: [] for k in arms}
    order = list(arms.items())
    for r in range(calls):
        # (rotated: no arm always runs behind the same neighbour, e.g. the 291 MB copy)
        for k, fn in order[r % len(order):] + order[:r % len(order)]:
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def eight(core):
    i = np.arange(core.n_members)
    return PARAMS + [("global_tas", Metric("mean", (1995, 2014), baseline=(1850, 1900))),
                     ("CO2_concentration", Metric("max", (1745, 2100))),
                     np.fmod(i * 0.6180339887498949, 1.0), np.cos(i * 0.001), (i % 97).astype(float)]


def numpy_moments(x, w, pred):
    """What a host does with the copied rows: weighted mean, variance and correlations per year."""
    wn = w / w.sum()
    mean = x @ wn
    xc = x - mean[:, None]
    var = (xc * xc) @ wn
    pc = pred - (pred @ wn)[:, None]
    cov = (xc * wn) @ pc.T
    return mean, var, cov / np.sqrt(var[:, None] * ((pc * pc) @ wn)[None, :])


def arms_moments(core, w):
    n = core.n_members
    buf = np.empty((SPAN[1] - SPAN[0] + 1, n))
    pred3 = np.stack([core.getvar(p) for p in PARAMS])
    # (against= as arrays: the timed call is the verb, not the getvar / metrics calls that resolve names)
    m8 = core.moments("global_tas", SPAN, weights=w, against=eight(core))
    pred8 = m8._pred
    x = fetch_into(core, "global_tas", buf).copy()
    return {
        "fetchvars(global_tas, 1745-2300) into a reused buffer": lambda: fetch_into(core, "global_tas", buf),
        "moments(global_tas, weights, against S / q10_rh / beta)": lambda: core.moments("global_tas", SPAN, weights=w, against=list(pred3)),
        "moments, unweighted, against S / q10_rh / beta": lambda: core.moments("global_tas", SPAN, against=list(pred3)),
        "moments, weighted, npred 0": lambda: core.moments("global_tas", SPAN, weights=w),
        "moments, weighted, npred 8": lambda: core.moments("global_tas", SPAN, weights=w, against=list(pred8)),
        "moments by name (getvar of 3 parameters included)": lambda: core.moments("global_tas", SPAN, weights=w, against=PARAMS),
        "numpy reduction of the copied rows (host, not the copy)": lambda: numpy_moments(x, w, pred3),
    }


def arms_quantiles(core, w):
    buf = np.empty((SPAN[1] - SPAN[0] + 1, core.n_members))
    return {
        "fetchvars(CO2_concentration, 1745-2300) into a reused buffer": lambda: fetch_into(core, "CO2_concentration", buf),
        "quantiles(CO2_concentration, 5 probs), unweighted": lambda: core.quantiles("CO2_concentration", PROBS, SPAN),
        "quantiles(CO2_concentration, 5 probs), weighted": lambda: core.quantiles("CO2_concentration", PROBS, SPAN, weights=w),
    }


def arms_metrics(core, w):
    specs = [Metric("mean", (2081, 2100), baseline=(1850, 1900)), Metric("max", (1850, 2300)),
             Metric("year_of_max", (1850, 2300)),
             Metric("first_ge", (1850, 2300), baseline=(1850, 1900), threshold=1.5)]
    edges = [1.0, 1.5, 2.0, 3.0]
    buf = np.empty((2300 - 1850 + 1, core.n_members))
    rows = core.metrics("global_tas", specs)
    return {
        "fetchvars(global_tas, 1850-2300) into a reused buffer": lambda: fetch_into(core, "global_tas", buf, (1850, 2300)),
        "metrics(global_tas, 4 specifications)": lambda: core.metrics("global_tas", specs),
        "probabilities(global_tas, 556 years x 4 edges), unweighted": lambda: core.probabilities("global_tas", edges, SPAN),
        "probabilities, weighted": lambda: core.probabilities("global_tas", edges, SPAN, weights=w),
        "quantiles(global_tas, 5 probs) of the same rows, unweighted": lambda: core.quantiles("global_tas", PROBS, SPAN),
        "quantiles of the same rows, weighted": lambda: core.quantiles("global_tas", PROBS, SPAN, weights=w),
        "metric_quantiles(4 specifications, 5 probs)": lambda: core.metric_quantiles("global_tas", specs, PROBS),
        "metric_probabilities(4 specifications, 4 edges)": lambda: core.metric_probabilities("global_tas", specs, edges),
        "host: np.nanquantile + np.histogram of the returned rows": lambda: (
            np.nanquantile(rows, PROBS, axis=1), [np.histogram(r[~np.isnan(r)], bins=[-np.inf] + edges + [np.inf]) for r in rows]),
    }


def arms_series(core, w):
    core.hold("held", "global_tas")
    b1, b2 = (np.empty((SPAN[1] - SPAN[0] + 1, core.n_members)) for _ in range(2))

    def a():
        core.derive("d", "sub", "global_tas", "held")
        return core.quantiles("d", PROBS, SPAN)

    def b():
        fetch_into(core, "global_tas", b1)
        fetch_into(core, "held", b2)

    return {
        "(a) derive(d, sub, global_tas, held) + quantiles(d, 5 probs)": a,
        "(b) two fetchvars into reused buffers": b,
        "derive(sub) alone": lambda: core.derive("d", "sub", "global_tas", "held"),
        "derive(cumsum)": lambda: core.derive("c", "cumsum", "global_tas"),
        "derive(runmean, width 20, centred)": lambda: core.derive("r", "runmean", "global_tas", width=20, align="centred"),
    }


GROUPS = {"moments": arms_moments, "quantiles": arms_quantiles, "metrics": arms_metrics, "series": arms_series}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, nargs="+", default=[65536, 131072])
    ap.add_argument("--groups", nargs="+", default=list(GROUPS), choices=list(GROUPS))
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--trace-only", action="store_true",
                    help="ten calls of every arm of the chosen groups, no timing (for a kernel trace)")
    a = ap.parse_args()
    if a.calls < 15:
        ap.error("--calls must be at least 15")
    out = {}
    for n in a.members:
        core = make_core(n)
        w = score_weights(core)
        print("## %d members (%s kernel, run %.1f ms)" % (n, core.last_run_kernel(), core.last_run_ms()), flush=True)
        for g in a.groups:
            arms = GROUPS[g](core, w)
            if a.trace_only:
                for fn in arms.values():
                    for _ in range(10):
                        fn()
                continue
            res = timed(arms, a.calls)
            out.setdefault(str(n), {})[g] = res
            for k, (med, lo, hi) in res.items():
                print("| %s | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi), flush=True)
        core.shutdown()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
