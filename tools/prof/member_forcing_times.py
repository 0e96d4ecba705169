#!/usr/bin/env python3
"""What forcing efficacies per member cost on one MI355X (Core.enable_member_forcing: delta_co2,
delta_ch4, delta_n2o in the extended run kernels, rho_bc / rho_oc / rho_so2 / rho_nh3 in the aerosol
row of hx_slcf_mix_kernel).  65 536 members, S / q10_rh perturbed, ssp245, 1745-2300.

    python tools/prof/member_forcing_times.py [--members 65536] [--steps 12] [--parent-lib PATH]

Cores in ONE process take turns, step by step (reset + run + sync each), after two untimed steps each:
  (p)  no per-member efficacy, no diagnostic: the plain run kernel of this library
  (q)  the same core on --parent-lib, the library built from the parent commit: the plain kernels
       are unchanged code, the two ranges must overlap
  (x0) the extended kernel (NPP recorded, HECTOR_AMD_EXTENDED_CONS=1) without per-member efficacies
  (x3) ... with the three delta_* per member (24 B per member, read every year)
  (x7) ... with all seven per member (and the aerosol row, 8 B per member-year)
  (v7) all seven per member and nothing else that makes the run "extended": against (p) the cost of
       making the efficacies vary
last_run_ms of every step is printed, then mean (min .. max).  Then the pre-pass: new rho_* values on
(v7) -- hx_slcf_mix_kernel with its synchronise, from the library's HECTOR_AMD_TIMING lines -- and
the wall time of setvar x 7 + reset + run + sync minus that run's last_run_ms."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gas_mix_times import stat  # noqa: E402
from slcf_mix_times import Stderr  # noqa: E402

NAMES = ["delta_co2", "delta_ch4", "delta_n2o", "rho_bc", "rho_oc", "rho_so2", "rho_nh3"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--members", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--parent-lib", default=None, help="libhector_amd.so built from the parent commit")
    a = ap.parse_args()
    os.environ["HECTOR_AMD_EXTENDED_CONS"] = "1"
    import hector_amd
    from hector_amd import ensemble
    n = a.members
    S, q10 = ensemble.ecs_q10(n)
    rng = np.random.default_rng(11)

    def draw(base):
        return {k: (rng.uniform(-0.2, 0.2, n) if k.startswith("delta") else base[k] * rng.uniform(0.5, 1.5, n))
                for k in NAMES}

    def core(names=(), outs=(), **kw):
        c = hector_amd.Core(hector_amd.DEFAULT_SCENARIO, n, device=0, **kw)
        c.setvar("S", S, "degC").setvar("q10_rh", q10)
        if names:
            c.enable_member_forcing()
            base = {k: c.getvar(k)[0] for k in NAMES}
            for k, v in draw(base).items():
                if k in names:
                    c.setvar(k, v)
        if outs:
            c.set_outputs(["CO2_concentration", "global_tas"] + list(outs))
        return c

    arms = [("p", "(p) plain kernel, this library", core()),
            ("x0", "(x0) extended kernel, efficacies shared", core(outs=["NPP"])),
            ("x3", "(x3) extended kernel, three delta_* per member", core(NAMES[:3], outs=["NPP"])),
            ("x7", "(x7) extended kernel, all seven per member", core(NAMES, outs=["NPP"])),
            ("v7", "(v7) all seven per member, nothing else extended", core(NAMES))]
    if a.parent_lib:
        arms.insert(1, ("q", "(q) plain kernel, the parent's library", core(lib_path=a.parent_lib)))
    ms = {k: [] for k, _, _ in arms}

    def step(c):
        c.reset(c.strtdate)
        c.run(2300)
        c.sync()
        return c.last_run_ms()

    for i in range(a.steps + 2):
        for k, _, c in arms:
            t = step(c)
            if i >= 2:
                ms[k].append(t)
    print("%d members, 1745-2300, %d steps per arm, arms alternating in one process; last_run_ms" % (n, a.steps))
    for k, what, c in arms:
        print("| %s | %s/%d | %s | %s |" % (what, c.last_run_kernel(), c.last_run_variant(), stat(ms[k]),
                                            " ".join("%.3f" % x for x in ms[k])))
    cv = dict((k, c) for k, _, c in arms)["v7"]
    base = {k: float(np.median(cv.getvar(k))) for k in NAMES}
    rest, pre = [], []
    os.environ["HECTOR_AMD_TIMING"] = "1"
    for i in range(a.steps):
        vals = draw(base)
        with Stderr() as err:
            t0 = time.perf_counter()
            for k in NAMES:
                cv.setvar(k, vals[k])
            cv.reset(cv.strtdate); cv.run(2300); cv.sync()
            rest.append(1e3 * (time.perf_counter() - t0) - cv.last_run_ms())
        pre.append(sum(err.laps("slcf mix kernel + sync")))
    del os.environ["HECTOR_AMD_TIMING"]
    print("| new values of all seven: setvar x 7 + reset + run + sync, minus the run kernel | %s | %s |"
          % (stat(rest), " ".join("%.1f" % x for x in rest)))
    print("| ... of it hx_slcf_mix_kernel with its synchronise (per-member rho_*, no mix) | %s | %s |"
          % (stat(pre), " ".join("%.2f" % x for x in pre)))
    for _, _, c in arms:
        assert (c.status() == 0).all()
        c.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
