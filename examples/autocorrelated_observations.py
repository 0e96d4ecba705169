#!/usr/bin/env python3
"""Scoring against a record whose errors are correlated from year to year.

The pseudo-observations are one held-out member's temperature anomaly plus seeded AR(1) noise (lag-one
correlation RHO): 165 annual values that carry far fewer than 165 independent pieces of evidence.  The
independent score, chi2 = sum (r / sigma)^2, counts them as 165 and exp(-chi2 / 2) collapses onto a
handful of members; Core.score(..., ar1=RHO) scores the same record with the covariance it has,
chi2 = r^T C^-1 r, on the device (hx_member_score_whitened).  Printed: the effective sample size of
the weights and the constrained 2100 band under both, and the same chi2 from a W factorised once
(hector_amd.whiten), the form a calibration loop uses.
Needs an MI355X:  python examples/autocorrelated_observations.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, GLOBAL_TAS  # noqa: E402

PROBS = (0.05, 0.5, 0.95)
SIGMA, RHO = 0.12, 0.6          # K and the lag-one correlation of the pseudo-observations' noise
BASE = (1850, 1900)


def main(n=20000, truth=0, **core_kwargs):
    rng = np.random.default_rng(1)
    core = hector_amd.newcore(None, n_members=n, **core_kwargs)   # packaged SSP2-4.5
    hector_amd.setvar(core, None, ECS(), rng.uniform(1.5, 6.0, n), "degC")
    hector_amd.setvar(core, None, Q10_RH(), rng.uniform(1.0, 3.0, n), "(unitless)")
    hector_amd.setvar(core, None, BETA(), rng.uniform(0.1, 0.9, n), "(unitless)")
    hector_amd.run(core, 2100)

    years = np.arange(1850, 2015)
    tas = core.fetchvars(GLOBAL_TAS(), (1850, 2014))[:, truth]
    noise = np.zeros(years.size)
    for i in range(years.size):     # stationary AR(1): variance SIGMA^2 in every year
        noise[i] = rng.normal(0.0, SIGMA) if i == 0 else \
            RHO * noise[i - 1] + rng.normal(0.0, SIGMA * np.sqrt(1.0 - RHO * RHO))
    obs = tas - tas[:51].mean() + noise

    ok = core.status() == 0
    ok[truth] = False                                  # held out
    actual = core.fetchvars(GLOBAL_TAS(), (2100, 2100))[0, truth]
    prior = core.quantiles(GLOBAL_TAS(), PROBS, (2100, 2100))[0]
    print("%-22s 2100 %s %.2f (%.2f-%.2f) K   held-out member %.2f" % ("prior", GLOBAL_TAS(), prior[1], prior[0],
                                                                      prior[2], actual))
    out = {}
    for name, kw in (("independent errors", dict(sigma=SIGMA)), ("AR(1) errors, rho %.1f" % RHO, dict(sigma=SIGMA, ar1=RHO))):
        chi2 = core.score(GLOBAL_TAS(), years, obs, baseline=BASE, **kw)
        weights = np.where(ok, np.exp(-0.5 * (chi2 - chi2[ok].min())), 0.0)
        n_eff = weights.sum() ** 2 / (weights ** 2).sum()
        post = core.quantiles(GLOBAL_TAS(), PROBS, (2100, 2100), weights=weights)[0]
        print("%-22s 2100 %s %.2f (%.2f-%.2f) K   effective sample size %.1f of %d"
              % (name, GLOBAL_TAS(), post[1], post[0], post[2], n_eff, n))
        out[name] = (chi2, weights, n_eff)

    # a calibration loop factorises once and hands W over; logdet is the other half of the Gaussian
    # log-likelihood, needed when sigma or rho are themselves calibrated
    C = SIGMA * SIGMA * RHO ** np.abs(years[:, None] - years[None, :])
    W, logdet = hector_amd.whiten(C)
    again = core.score(GLOBAL_TAS(), years, obs, baseline=BASE, whiten=W)
    assert np.array_equal(again, out["AR(1) errors, rho %.1f" % RHO][0])
    loglik = -0.5 * (again + logdet + years.size * np.log(2.0 * np.pi))
    print("log-likelihood of the best member %.1f (chi2 %.1f for %d years, log det C %.1f)"
          % (loglik[ok].max(), again[ok].min(), years.size, logdet))
    hector_amd.shutdown(core)
    return out


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
