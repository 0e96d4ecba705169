#!/usr/bin/env python3
"""Wall times of the grouped summaries against the masked calls they replace, by the protocol of
profiles/post_summaries.md: a warm core, two untimed calls, then --calls timed calls (at least 15) of
every arm, the arms interleaved round by round in ONE process on the same core, the order rotated from
round to round; median (min .. max) in ms, time.perf_counter around the Python call, result in host
memory.  ssp245, S / q10_rh / beta perturbed, 1745-2300 (556 years), labels = member % G.

For every G and verb two arms: ONE call with groups=, and the G calls of the ungrouped verb with the
weights zeroed outside one group each (what a user does without groups=; there wmax is taken over
the masked vector, so the integer weights differ from group to group).

    python tools/prof/grouped_times.py                           # 65 536 members, G = 2, 8, 16
    python tools/prof/grouped_times.py --groups 8 --json out.json
    python tools/prof/grouped_times.py --groups 8 --trace-only
        (ten calls of each grouped arm and nothing else: what to put behind
         `rocprofv3 --kernel-trace --stats --` for kernel times)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from post_times import PARAMS, PROBS, SPAN, make_core, score_weights, timed   # noqa: E402

EDGES = [1.0, 1.5, 2.0, 3.0]
VAR = "global_tas"


def arms(core, w, G):
    n = core.n_members
    lab = (np.arange(n) % G).astype(np.int32)
    masked = [np.where(lab == g, w, 0.0) for g in range(G)]
    assert all(m.max() > 0 for m in masked)
    pred = [core.getvar(p) for p in PARAMS]   # (arrays: the timed call is the verb, not getvar)
    return {
        "quantiles, 5 probs, weighted: ONE grouped call": lambda: core.quantiles(VAR, PROBS, SPAN, weights=w, groups=(lab, G)),
        "quantiles: the G masked calls": lambda: [core.quantiles(VAR, PROBS, SPAN, weights=m) for m in masked],
        "probabilities, 4 edges, weighted: ONE grouped call": lambda: core.probabilities(VAR, EDGES, SPAN, weights=w, groups=(lab, G)),
        "probabilities: the G masked calls": lambda: [core.probabilities(VAR, EDGES, SPAN, weights=m) for m in masked],
        "moments against S / q10_rh / beta, weighted: ONE grouped call": lambda: core.moments(VAR, SPAN, weights=w, against=pred, groups=(lab, G)),
        "moments: the G masked calls": lambda: [core.moments(VAR, SPAN, weights=m, against=pred) for m in masked],
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--trace-only", action="store_true",
                    help="ten calls of every grouped arm, no timing (for a kernel trace)")
    a = ap.parse_args()
    if a.calls < 15:
        ap.error("--calls must be at least 15")
    core = make_core(a.members)
    w = score_weights(core)
    print("## %d members (%s kernel, run %.1f ms)" % (a.members, core.last_run_kernel(), core.last_run_ms()), flush=True)
    out = {}
    for G in a.groups:
        arm = arms(core, w, G)
        if a.trace_only:
            for k, fn in arm.items():
                if "ONE grouped call" in k:
                    for _ in range(10):
                        fn()
            continue
        res = timed(arm, a.calls)
        out[str(G)] = res
        print("### G = %d" % G, flush=True)
        for k, (med, lo, hi) in res.items():
            print("| %s | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi), flush=True)
        for verb in ("quantiles", "probabilities", "moments"):
            one = [v[0] for k, v in res.items() if k.startswith(verb) and "ONE" in k][0]
            many = [v[0] for k, v in res.items() if k.startswith(verb) and "masked" in k][0]
            print("%s: grouped / masked = %.3f (target <= 0.90 at G = 8)" % (verb, one / many), flush=True)
    core.shutdown()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
