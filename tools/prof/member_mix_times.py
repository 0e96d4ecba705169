#!/usr/bin/env python3
"""Wall times and host memory of per-member emission series given as dense tables
(Core.setvar_dated_members, the path every earlier commit has) against the same values given as a
mix of shared year-vectors (Core.setvar_dated_mix), on one MI355X.  65 536 members, S / q10_rh
perturbed, ssp245; the five emission variables, 2030-2100, K = 3.

    python tools/prof/member_mix_times.py [--members 65536] [--out profiles/member_mix.md]

Each path runs in a fresh process of its own (ru_maxrss is a high-water mark), after one untimed plain
run to 2100.  time.perf_counter around the Python calls, the values prepared outside the timed span,
every figure the mean (min .. max) of 5 repetitions with new values each:
  (a) setvar_dated_members x 5 + reset + run(2100)                       -- the dense path, the baseline
  (b) the first setvar_dated_mix x 5 (no table on the device yet) + reset + run(2100)
  (c) setvar_dated_mix x 5 with new coefficients for the same years and basis + reset + run(2100)
and last_run_ms of every timed run, ru_maxrss before and after the timed part.  The mix path runs a
second time, in a third process, with a quarter of the members.  Three conditions are stated and
decide the exit status: (c) <= (a); the run kernel's time the same on both paths within the
run-to-run spread (the device tables hold the same bits: the two ranges overlap); the mix path's
growth of ru_maxrss does not scale with n_members x n_years -- from a quarter of the members to all
of them it rises by less than a quarter of what ONE such table rises by (the recipe is 15 doubles a
member, a table 556; the dense path holds five tables and a staging copy).
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

YEARS = np.arange(2030, 2101)
K, REPS, TO = 3, 5, 2100
# (unit, low, high of the large term's basis, amplitude of the small terms' basis)
VARS = {"ffi_emissions": ("Pg C/yr", 4.0, 10.0, 0.3), "daccs_uptake": ("Pg C/yr", 0.5, 2.0, 0.03),
        "luc_emissions": ("Pg C/yr", 0.5, 2.0, 0.03), "luc_uptake": ("Pg C/yr", 0.3, 1.0, 0.02),
        "CH4_emissions": ("Tg CH4", 150.0, 450.0, 10.0)}


def recipe(rng, n):
    """-> {name: (basis[K, year], coeff[K, member])}: one large positive term, small ones of both signs."""
    out = {}
    for name, (_, lo, hi, small) in VARS.items():
        basis = np.vstack([rng.uniform(lo, hi, (1, YEARS.size)), rng.uniform(-small, small, (K - 1, YEARS.size))])
        coeff = np.vstack([rng.uniform(0.7, 1.3, (1, n)), rng.uniform(-1.0, 1.0, (K - 1, n))])
        out[name] = (basis, coeff)
    return out


def dense_values(basis, coeff):
    s = coeff[0][None, :] * basis[0][:, None]
    for k in range(1, K):
        s = s + coeff[k][None, :] * basis[k][:, None]
    return s


def rss_mb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0


def arm(which, n):
    """One path in this process -> a dict of figures (printed as one JSON line)."""
    import hector_amd
    from hector_amd import ensemble
    core = hector_amd.Core(n_members=n, device=0)
    S, q10 = ensemble.ecs_q10(n)
    core.setvar("S", S, "degC").setvar("q10_rh", q10)
    core.run(TO)
    plain_ms = core.last_run_ms()
    rng = np.random.default_rng(5)
    rec = recipe(rng, n)
    res = {"arm": which, "members": n, "plain_run_ms": plain_ms, "rss_before_mb": rss_mb()}

    def timed(setter, prepare):
        wall, run_ms = [], []
        for _ in range(REPS):
            args = prepare()
            t0 = time.perf_counter()
            for name in VARS:
                setter(name, args[name])
            core.reset(core.strtdate)
            core.run(TO)
            wall.append(1e3 * (time.perf_counter() - t0))
            run_ms.append(core.last_run_ms())
        return wall, run_ms

    def new_coeff():
        return {name: c * rng.uniform(0.97, 1.03, c.shape) for name, (_, c) in rec.items()}

    if which == "dense":
        def prepare():
            w = new_coeff()
            return {name: dense_values(rec[name][0], w[name]) for name in VARS}
        res["a_wall_ms"], res["a_run_ms"] = timed(
            lambda name, v: core.setvar_dated_members(name, YEARS, v, VARS[name][0]), prepare)
    else:
        def set_mix(name, w):
            core.setvar_dated_mix(name, YEARS, rec[name][0], w, VARS[name][0])

        def first():
            for name in VARS:
                core.clear_mix(name)
            core.run(TO)          # (untimed: the tables leave the device, the plain kernel runs)
            return new_coeff()
        res["b_wall_ms"], res["b_run_ms"] = timed(set_mix, first)
        res["c_wall_ms"], res["c_run_ms"] = timed(set_mix, new_coeff)
    res["kernel"] = "%s/%d" % (core.last_run_kernel(), core.last_run_variant())
    assert (core.status() == 0).all()
    res["rss_after_mb"] = rss_mb()
    core.shutdown()
    print("MEMBER_MIX " + json.dumps(res), flush=True)


def stat(v):
    return "%.1f (%.1f .. %.1f)" % (np.mean(v), np.min(v), np.max(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--arm", choices=("dense", "mix"), help="(internal) run one path in this process")
    a = ap.parse_args()
    if a.arm:
        arm(a.arm, a.members)
        return 0
    got = {}
    n = a.members
    for which, members in (("dense", n), ("mix", n), ("mix/4", n // 4)):   # one after the other, each a fresh process
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", which.split("/")[0], "--members",
                            str(members)], stdout=subprocess.PIPE, text=True, check=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("MEMBER_MIX ")][-1]
        got[which] = json.loads(line[len("MEMBER_MIX "):])
    d, m, m4 = got["dense"], got["mix"], got["mix/4"]
    table_mb = 8.0 * n * 556 / 2**20
    grow_d, grow_m = d["rss_after_mb"] - d["rss_before_mb"], m["rss_after_mb"] - m["rss_before_mb"]
    grow_m4 = m4["rss_after_mb"] - m4["rss_before_mb"]
    c1 = np.mean(m["c_wall_ms"]) <= np.mean(d["a_wall_ms"])
    runs_d, runs_m = d["a_run_ms"], m["b_run_ms"] + m["c_run_ms"]
    c2 = min(runs_m) <= max(runs_d) and min(runs_d) <= max(runs_m)   # the two ranges overlap
    c3 = grow_m - grow_m4 < 0.25 * (table_mb - 8.0 * (n // 4) * 556 / 2**20)
    lines = [
        "# Per-member emission series: dense tables against mixes",
        "",
        "`tools/prof/member_mix_times.py --members %d`: %d members, ssp245 to %d, S / q10_rh perturbed, the five "
        "emission variables per member in 2030-2100, K = 3; kernel %s on both paths (a plain run without member "
        "series: %.1f ms).  Wall time in ms, mean (min .. max) of %d repetitions with new values each; each path in "
        "a fresh process." % (n, n, TO, d["kernel"], d["plain_run_ms"], REPS),
        "",
        "| what | wall time, ms | last_run_ms |",
        "|---|---|---|",
        "| (a) `setvar_dated_members` x 5 + `reset` + `run` (the dense path, unchanged: the baseline) | %s | %s |"
        % (stat(d["a_wall_ms"]), stat(d["a_run_ms"])),
        "| (b) the first `setvar_dated_mix` x 5 + `reset` + `run` | %s | %s |" % (stat(m["b_wall_ms"]), stat(m["b_run_ms"])),
        "| (c) new coefficients alone: `setvar_dated_mix` x 5 + `reset` + `run` | %s | %s |"
        % (stat(m["c_wall_ms"]), stat(m["c_run_ms"])),
        "",
        "| ru_maxrss, MB | before | after | growth |",
        "|---|---|---|---|",
        "| dense path | %.0f | %.0f | %.0f |" % (d["rss_before_mb"], d["rss_after_mb"], grow_d),
        "| mix path | %.0f | %.0f | %.0f |" % (m["rss_before_mb"], m["rss_after_mb"], grow_m),
        "| mix path, %d members | %.0f | %.0f | %.0f |" % (n // 4, m4["rss_before_mb"], m4["rss_after_mb"], grow_m4),
        "",
        "One table of n_members x n_years doubles is %.0f MB here; the dense path keeps five on the host." % table_mb,
        "",
        "The conditions:",
        "",
        "- (c) <= (a): %.1f ms against %.1f ms, a factor of %.1f -- **%s**"
        % (np.mean(m["c_wall_ms"]), np.mean(d["a_wall_ms"]), np.mean(d["a_wall_ms"]) / np.mean(m["c_wall_ms"]),
           "holds" if c1 else "MISSED"),
        "- `last_run_ms` the same on both paths within the run-to-run spread (the ranges %.2f .. %.2f ms dense and "
        "%.2f .. %.2f ms mix overlap) -- **%s**"
        % (min(runs_d), max(runs_d), min(runs_m), max(runs_m), "holds" if c2 else "MISSED"),
        "- the mix path's growth of ru_maxrss does not scale with n_members x n_years: %.0f MB with %d members, %.0f MB "
        "with %d, a rise of %.0f MB where ONE table rises by %.0f MB (the dense path grew by %.0f MB) -- **%s**"
        % (grow_m, n, grow_m4, n // 4, grow_m - grow_m4, 0.75 * table_mb, grow_d, "holds" if c3 else "MISSED"),
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if (c1 and c2 and c3) else 1


if __name__ == "__main__":
    sys.exit(main())
