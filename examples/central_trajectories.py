#!/usr/bin/env python3
"""Ranks of the members within every year, on the GPU (Core.rank_series, Core.crps, Core.spearman),
and what they give a perturbed-parameter ensemble:

- the central trajectories.  A member's mid-PIT z within a year is the share of the ensemble below it;
  z - z^2 is largest for the member in the middle, and its mean over the years is the member's
  modified band depth.  The deepest member is the ensemble's median TRAJECTORY, and the envelope of the
  deepest half its central 50 % of trajectories -- which is not the year-wise 25-75 % band of
  Core.quantiles: a trajectory that stays inside that band in every year is rarer than one that does so
  in a typical year.
- a proper score.  The CRPS of the ensemble against an observed record, and the rank histogram of the
  observations' own PIT (flat for a calibrated ensemble, a hump for an under-confident one, a U for an
  over-confident one), for the prior and for the score-weighted ensemble.
- Spearman sensitivities.  The model is monotone but not linear in S, q10_rh, beta and diff; the rank
  correlation measures the monotone dependence, Core.moments(...).corr only its linear part.

The "observations" are pseudo-observations as in constrained_projection.py: a held-out member's record
plus noise.  Needs an MI355X:  python examples/central_trajectories.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd import Metric, ensemble              # noqa: E402

PARAMS = (("S", 1.5, 6.0, "degC"), ("q10_rh", 1.0, 3.0, "(unitless)"), ("beta", 0.2, 0.8, "(unitless)"),
          ("diff", 1.0, 4.0, "cm2/s"))
SIGMA = 0.12                                          # K: the noise of the pseudo-observations


def main(n=20000, truth=0, **core_kwargs):
    rng = np.random.default_rng(2)
    idx = np.arange(n, dtype=np.uint64)
    core = hector_amd.Core(n_members=n, **core_kwargs)   # packaged SSP2-4.5
    for i, (name, lo, hi, units) in enumerate(PARAMS):
        core.setvar(name, lo + (hi - lo) * ensemble.uniform01(idx, i), units)
    core.run(2100)
    names = [p[0] for p in PARAMS]
    win = (1850, 2100)
    core.derive("tas", "anomaly", "global_tas", years=(1850, 1900))   # warming relative to 1850-1900

    # --- the central trajectories ---------------------------------------------------------------
    core.rank_series("pit", "tas", win)
    core.derive("depth", "mul", "pit", "pit").derive("depth", "sub", "pit", "depth")   # z - z^2
    mbd = core.metrics("depth", [Metric("mean", win)])[0]               # modified band depth / 2
    ok = core.status() == 0
    mbd = np.where(ok, mbd, -np.inf)
    deepest = int(np.argmax(mbd))
    half = mbd >= np.median(mbd[ok])
    tas = core.fetchvars("tas", win)                                    # (for the envelope only)
    env_lo, env_hi = tas[:, half].min(axis=1), tas[:, half].max(axis=1)
    band = core.quantiles("tas", (0.25, 0.5, 0.75), win)
    print("deepest member %d: S %.2f q10_rh %.2f beta %.2f diff %.2f; 2100 warming %.2f K (year-wise median %.2f K)"
          % ((deepest,) + tuple(core.getvar(p)[deepest] for p in names) + (tas[-1, deepest], band[-1, 1])))
    for y in (1950, 2000, 2050, 2100):
        r = y - win[0]
        print("  %d  envelope of the deepest half %.2f .. %.2f K   year-wise 25-75 %% band %.2f .. %.2f K"
              % (y, env_lo[r], env_hi[r], band[r, 0], band[r, 2]))
    inside = ((tas >= band[:, :1]) & (tas <= band[:, 2:])).all(axis=0)
    print("  members inside the year-wise band in EVERY year: %.1f %% (the deepest half: 50 %%)" % (100 * inside.mean()))

    # --- CRPS and the rank histogram of the observations ---------------------------------------------
    years = np.arange(1850, 2015)
    obs = tas[:years.size, truth] + rng.normal(0.0, SIGMA, years.size)
    chi2 = core.score("tas", years, obs, sigma=SIGMA)
    keep = ok.copy()
    keep[truth] = False                                                 # held out
    weights = np.where(keep, np.exp(-0.5 * (chi2 - chi2[keep].min())), 0.0)
    for title, w in (("prior", np.where(keep, 1.0, 0.0)), ("score-weighted", weights)):
        crps, pit = core.crps("tas", years, obs, weights=w, return_pit=True)
        hist = np.histogram(pit, bins=5, range=(0.0, 1.0))[0]
        print("%-15s mean CRPS 1850-2014 %.4f K   rank histogram of the observations (fifths) %s"
              % (title, crps.mean(), hist))

    # --- Spearman against Pearson -----------------------------------------------------------------
    rho = core.spearman("tas", names, (2100, 2100))[0]
    lin = core.moments("tas", (2100, 2100), against=names).corr[0]
    print("2100 warming against   " + "  ".join("%8s" % p for p in names))
    print("  Spearman             " + "  ".join("%8.4f" % v for v in rho))
    print("  Pearson              " + "  ".join("%8.4f" % v for v in lin))
    core.shutdown()
    return deepest, rho, lin


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:2]))
