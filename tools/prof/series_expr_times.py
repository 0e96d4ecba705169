#!/usr/bin/env python3
"""Wall times of Core.derive_expr (hx_series_eval) against the Core.derive calls and the host route
it replaces, by the protocol of profiles/post_summaries.md: a warm core, two untimed calls, then
--calls timed calls (at least 10) of every device arm, interleaved round by round in ONE process on
the same core; median (min .. max) in ms, time.perf_counter around the Python call -- every one of
these calls ends in a synchronise of the core's stream, and includes the allocation of the new
292 MB block and the release of the one it replaces.  ssp245 to 2300, S and q10_rh varied, 65 536
members x 556 years.
What the clock is: a host clock around work that ends in a device synchronise, not HIP events --
derive and derive_expr synchronise the core's stream themselves, so events around the call would
bracket the same work plus nothing; the ctypes marshalling and, in the text arm, the parse are in it.
The kernels' own times (and from them the bytes per second) come from the kernel trace.
What the yardstick is: Core.derive of THIS library.  hx_series_ew_kernel and hx_series_define are
unchanged from the parent commit, so no second library is loaded for them; --lib times an experiment
build of this library (tools/prof/build_variant.sh ... -DHXE_SMALL_ROWS=4) by the same protocol.

    python tools/prof/series_expr_times.py [--members 65536] [--calls 10] [--host-calls 3] [--json out.json] [--lib lib.so]
    rocprofv3 --kernel-trace --stats -- python tools/prof/series_expr_times.py --trace-only

  1. interpretive overhead: derive_expr("a + b") beside derive("add"): the same three blocks of traffic
  2. fusion: (CO2_concentration - 277.15) / CO2_concentration * global_tas as one expression beside
     the three-call derive chain (3 blocks moved against 8, two allocations fewer)
  3. the compound event (global_tas anomaly >= 2 K and pH < 8.0) and its probabilities per year,
     beside fetchvars of both variables + numpy
The kernel trace gives the kernels' own times; the bytes a kernel must move are printed here.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import hector_amd                                   # noqa: E402
from hector_amd import ensemble, expr               # noqa: E402
from post_times import fetch_into, timed            # noqa: E402

FUSED = "(CO2_concentration - 277.15) / CO2_concentration * global_tas"
EVENT = "(dT >= 2.0) & (pH < 8.0)"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--json", help="also write the figures to this file")
    ap.add_argument("--lib", help="an experiment build of the library (default: the product library)")
    ap.add_argument("--device-only", action="store_true", help="skip the host arm (fetchvars + numpy)")
    ap.add_argument("--trace-only", action="store_true",
                    help="10 calls of the device arms and nothing else (for a kernel trace)")
    a = ap.parse_args()
    if a.calls < 10:
        ap.error("--calls must be at least 10")
    n = a.members
    core = hector_amd.Core(n_members=n, device=0, **({"lib_path": a.lib} if a.lib else {}))
    S, q10 = ensemble.ecs_q10(n)
    core.setvar("S", S, "degC").setvar("q10_rh", q10)
    core.set_outputs(["CO2_concentration", "global_tas", "pH"])
    core.run(2300)
    y0, y1 = core.strtdate, 2300
    ny = y1 - y0 + 1
    block = 8.0 * ny * core.device_var("global_tas")[1]
    print("## %d members x %d years (%s kernel, run %.1f ms); one block %.1f MB"
          % (n, ny, core.last_run_kernel(), core.last_run_ms(), block / 1e6), flush=True)
    core.derive("dT", "anomaly", "global_tas", years=(1850, 1900))
    core.hold("pHs", "pH")     # (the combination as a series: neither arm pays for computing it)
    add = expr.compile("CO2_concentration + global_tas")
    fused = expr.compile(FUSED)
    event = expr.compile(EVENT, {"pH": "pHs"})

    def chain():
        core.derive("t1", "sub", "CO2_concentration", 277.15)
        core.derive("t2", "div", "t1", "CO2_concentration")
        core.derive("z3", "mul", "t2", "global_tas")

    def event_and_probabilities():
        core.derive_expr("ev", event)
        return core.probabilities("ev", [0.5], (y0, y1))

    arms = {
        'derive("z", "add", CO2_concentration, global_tas)': lambda: core.derive("z", "add", "CO2_concentration", "global_tas"),
        'derive_expr("ze", "CO2_concentration + global_tas")': lambda: core.derive_expr("ze", add),
        "the same from text (parsed every call)": lambda: core.derive_expr("ze", "CO2_concentration + global_tas"),
        "three derive calls: sub, div, mul": chain,
        'derive_expr("zf", "%s")' % FUSED: lambda: core.derive_expr("zf", fused),
        'derive_expr("ev", "%s") + probabilities(ev, [0.5])' % EVENT: event_and_probabilities,
    }
    if a.trace_only:
        for _ in range(10):
            for fn in arms.values():
                fn()
        return
    res = timed(arms, a.calls)
    # the results agree before their times are compared
    assert np.array_equal(core.fetchvars("z", (y0, y1)), core.fetchvars("ze", (y0, y1)), equal_nan=True)
    assert np.array_equal(core.fetchvars("z3", (y0, y1)), core.fetchvars("zf", (y0, y1)), equal_nan=True)
    if a.device_only:
        print("| call | ms: median (min .. max) |\n|---|---|")
        for k, (med, lo, hi) in res.items():
            print("| `%s` | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi))
        return
    bt, bp = np.empty((ny, n)), np.empty((ny, n))

    def host_event():
        t = fetch_into(core, "dT", bt, (y0, y1))
        p = fetch_into(core, "pHs", bp, (y0, y1))
        with np.errstate(invalid="ignore"):
            ind = (t >= 2.0) & (p < 8.0)
            ok = ~(np.isnan(t) | np.isnan(p))
            return ind.sum(axis=1) / ok.sum(axis=1)

    host = timed({"fetchvars(dT) + fetchvars(pH) into reused buffers + numpy": host_event}, max(a.host_calls, 1))
    dev = event_and_probabilities()[:, 1]
    ref = host_event()
    assert np.allclose(dev, ref, rtol=1e-14, atol=0.0, equal_nan=True), np.nanmax(np.abs(dev - ref))
    res.update(host)
    print("| call | ms: median (min .. max) |\n|---|---|")
    for k, (med, lo, hi) in res.items():
        print("| `%s` | %.3f (%.3f .. %.3f) |" % (k, med, lo, hi))
    keys = list(arms)
    r1 = res[keys[1]][0] / res[keys[0]][0]
    r2 = res[keys[4]][0] / res[keys[3]][0]
    print("\n1. derive_expr(a + b) / derive(add): %.3f of it (expected at most 1.15)" % r1)
    print("2. one expression / the three-call chain: %.3f of it (expected at most 0.6; the byte model 3 : 8 = 0.375)" % r2)
    print("3. the compound event + probabilities / fetchvars + numpy: %.4f of it" % (res[keys[5]][0] / list(host.values())[0][0]))
    print("bytes a kernel must move: add 3 blocks = %.1f MB (either route); the fused expression 3 blocks = %.1f MB; "
          "the chain 2 + 3 + 3 = 8 blocks = %.1f MB" % (3 * block / 1e6, 3 * block / 1e6, 8 * block / 1e6))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"members": n, "years": ny, "block_bytes": block, "ms": res, "ratio_add": r1, "ratio_fused": r2}, f,
                      indent=1)


if __name__ == "__main__":
    main()
