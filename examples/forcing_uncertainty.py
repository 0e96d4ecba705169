#!/usr/bin/env python3
"""A per-agent forcing-uncertainty ensemble in ONE launch.  Core.enable_member_forcing() lets setvar
take one value per member for the seven forcing efficacies: delta_co2, delta_ch4, delta_n2o scale the
CO2, CH4 and N2O forcing independently, rho_bc, rho_oc, rho_so2, rho_nh3 give every aerosol species
its own efficacy (aero_scalar can only move the four together).  They are drawn next to the climate
sensitivity `S`, the ocean heat diffusivity `diff` and `aero_scalar`.

Printed: the 2100 warming and total-forcing band, and how much of the 2100 spread each agent carries:
the squared standardised regression coefficients of all ten factors jointly (Moments.src()**2; the
factors are drawn independently, so they add up to about R^2).
Needs an MI355X:  python examples/forcing_uncertainty.py [members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402

EFFICACIES = ("delta_co2", "delta_ch4", "delta_n2o", "rho_bc", "rho_oc", "rho_so2", "rho_nh3")


def main(n=16384, **core_kwargs):
    rng = np.random.default_rng(1)
    core = hector_amd.Core(n_members=n, **core_kwargs)
    core.enable_member_forcing()
    draws = {"S": rng.uniform(2.0, 5.0, n), "diff": rng.uniform(0.8, 2.5, n),
             "aero_scalar": rng.uniform(0.7, 1.3, n)}
    for k in EFFICACIES:
        ini = core.getvar(k)[0]
        # the reference's delta_* are fractions of the stratospheric-adjusted forcing, the rho_* W/m2
        # per unit of emissions: +-0.15 around the INI value, x 0.5..1.5 of it
        draws[k] = ini + rng.uniform(-0.15, 0.15, n) if k.startswith("delta") else ini * rng.uniform(0.5, 1.5, n)
    for k, v in draws.items():
        core.setvar(k, v)
    core.set_outputs(["CO2_concentration", "global_tas", "RF_tot"])
    core.run(2100)
    assert (core.status() == 0).all()

    print("%d members, ten factors, one launch (kernel %s/%d, %.2f ms)"
          % (n, core.last_run_kernel(), core.last_run_variant(), core.last_run_ms()))
    for var, unit in (("global_tas", "K"), ("RF_tot", "W/m2")):
        q = core.quantiles(var, (0.05, 0.5, 0.95), dates=(2100, 2100))[0]
        print("  %-10s 2100: median %.2f (5-95 %%: %.2f .. %.2f) %s" % (var, q[1], q[0], q[2], unit))
    # the eight-entry limit of `against`: the seven efficacies and S for the forcing and the warming;
    # diff and aero_scalar, which RF_tot does not see / sees through the aerosols, in a second call
    first = list(EFFICACIES) + ["S"]
    print("share of the 2100 variance, src^2 of the factors jointly:")
    print("  %-12s %10s %10s" % ("factor", "global_tas", "RF_tot"))
    mt, mf = (core.moments(v, [2100], against=first) for v in ("global_tas", "RF_tot"))
    st, sf = mt.src()[0] ** 2, mf.src()[0] ** 2
    for j, k in enumerate(first):
        print("  %-12s %9.1f%% %9.1f%%" % (k, 100 * st[j], 100 * sf[j]))
    rest = core.moments("global_tas", [2100], against=["diff", "aero_scalar"]).src()[0] ** 2
    for j, k in enumerate(("diff", "aero_scalar")):
        print("  %-12s %9.1f%%" % (k, 100 * rest[j]))
    core.shutdown()
    return st, sf


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
