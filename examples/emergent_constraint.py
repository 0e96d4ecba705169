#!/usr/bin/env python3
"""An emergent constraint and the EOFs of an ensemble, without a trajectory leaving the GPU
(Core.comoments): which observable years of global_tas tell most about the warming in 2100 -- the
correlation map of 1980-2020 against 2100, over the prior ensemble and over the ensemble weighted by
its score against an observed record -- what a degree of observed warming in such a year is worth in
2100 (the regression slope), and how many patterns the 1850-2100 trajectories really have (the
variance share of the first three EOFs of the year x year covariance matrix).  The "observations" are
pseudo-observations: one held-out member plus seeded noise.
Needs an MI355X:  python examples/emergent_constraint.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, CONCENTRATIONS_CO2, GLOBAL_TAS  # noqa: E402

SIGMA_CO2 = 2.0          # ppmv: the noise of the pseudo-observations


def main(n=20000, truth=0, **core_kwargs):
    rng = np.random.default_rng(1)
    core = hector_amd.newcore(None, n_members=n, **core_kwargs)   # packaged SSP2-4.5
    hector_amd.setvar(core, None, ECS(), rng.uniform(1.5, 6.0, n), "degC")
    hector_amd.setvar(core, None, Q10_RH(), rng.uniform(1.0, 3.0, n), "(unitless)")
    hector_amd.setvar(core, None, BETA(), rng.uniform(0.1, 0.9, n), "(unitless)")
    hector_amd.run(core, 2100)

    # score-weights from the held-out member's CO2 record: the constraint leaves the sensitivity open
    years = np.arange(1850, 2015)
    obs = core.fetchvars(CONCENTRATIONS_CO2(), (1850, 2014))[:, truth] + rng.normal(0.0, SIGMA_CO2, years.size)
    chi2 = core.score(CONCENTRATIONS_CO2(), years, obs, sigma=SIGMA_CO2)
    ok = core.status() == 0
    ok[truth] = False
    weights = np.where(ok, np.exp(-0.5 * (chi2 - chi2[ok].min())), 0.0)

    # the 2100 warming relative to 1850-1900 as a series on the device; then two 41 x 1 matrices
    core.derive("warming", "anomaly", GLOBAL_TAS(), years=(1850, 1900))
    prior = core.comoments(GLOBAL_TAS(), (1980, 2020), "warming", (2100, 2100))
    post = core.comoments(GLOBAL_TAS(), (1980, 2020), "warming", (2100, 2100), weights=weights)
    print("correlation of global_tas in an observable year with the warming in 2100, and K in 2100 per K then")
    print("year   prior corr  slope    score-weighted corr  slope")
    for i in range(0, 41, 5):
        print("%d   %9.4f  %6.3f   %18.4f  %6.3f" % (prior.years_a[i], prior.corr[i, 0], prior.slope[i, 0],
                                                      post.corr[i, 0], post.slope[i, 0]))
    best = int(np.nanargmax(np.abs(post.corr[:, 0])))
    print("%d members took part in the prior, %d carry weight; the most telling year under the constraint is %d"
          % (prior.n_part, post.n_part, post.years_a[best]))

    # EOFs of the trajectories: the symmetric call computes the blocks on or above the diagonal only
    for label, w in (("prior", None), ("score-weighted", weights)):
        cm = core.comoments(GLOBAL_TAS(), (1850, 2100), weights=w)
        val, share, pat = cm.pca(3)
        print("%-15s EOFs of global_tas 1850-2100: variance shares %.4f %.4f %.4f (sum %.6f); EOF 1 peaks in %d"
              % (label, share[0], share[1], share[2], share.sum(), cm.years_a[int(np.argmax(pat[0]))]))
    hector_amd.shutdown(core)
    return prior, post


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
