#!/usr/bin/env python3
"""One step of an ensemble smoother with multiple data assimilation (ES-MDA) without the trajectories
ever leaving the device.

The pseudo-observations are one held-out member's temperature anomaly 1850-2014 (relative to
1850-1900) plus seeded noise of standard deviation SIGMA.  With y a member's 165 simulated anomalies
and theta its parameters (S, q10_rh, beta), a step with inflation ALPHA moves every member by

    theta <- theta + K (obs + sqrt(ALPHA) eps - y),    K = C_theta_y (C_yy + ALPHA R)^-1,  R = SIGMA^2 I

Core.moments(against=...) gives C_theta_y, Core.comoments gives C_yy, the 3 x 165 gain is a small solve
on the host, and Core.project(..., K, center=obs) -- hx_member_project -- applies it to every member's
residuals y - obs on the fp64 matrix pipe.  K sqrt(ALPHA) eps is drawn directly in parameter space
(three numbers a member, covariance ALPHA K R K^T).  The update goes back with setvar, then reset and
run.  Printed: the spread of the 2100 warming before and after the step, and how the first three
principal-component scores of the anomalies (CoMoments.scores) correlate with S.
A full ES-MDA repeats the step N times with inflations whose reciprocals add up to 1 (here: the first
of four steps with ALPHA = 4).
Needs an MI355X:  python examples/ensemble_smoother.py [n_members]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import hector_amd                                    # noqa: E402
from hector_amd.capabilities import ECS, Q10_RH, BETA, GLOBAL_TAS  # noqa: E402

SIGMA, ALPHA = 0.12, 4.0
BASE = (1850, 1900)
PRIOR = ((ECS, 1.5, 6.0, "degC"), (Q10_RH, 1.0, 3.0, "(unitless)"), (BETA, 0.1, 0.9, "(unitless)"))


def spread(core, label):
    q = core.quantiles(GLOBAL_TAS(), (0.05, 0.5, 0.95), (2100, 2100))[0]
    sd = float(core.moments(GLOBAL_TAS(), (2100, 2100)).sd[0])
    print("%-18s 2100 %s %.2f (%.2f-%.2f) K, standard deviation %.3f K" % (label, GLOBAL_TAS(), q[1], q[0], q[2], sd))
    return sd


def main(n=20000, truth=0, **core_kwargs):
    rng = np.random.default_rng(2)
    core = hector_amd.newcore(None, n_members=n, **core_kwargs)   # packaged SSP2-4.5
    theta = np.stack([rng.uniform(lo, hi, n) for _, lo, hi, _ in PRIOR])
    for (cap, _, _, unit), values in zip(PRIOR, theta):
        hector_amd.setvar(core, None, cap(), values, unit)
    hector_amd.run(core, 2100)
    sd_prior = spread(core, "prior")

    years = np.arange(1850, 2015)
    core.derive("tas_anom", "anomaly", GLOBAL_TAS(), years=BASE)      # y: every member's anomalies, on the device
    obs = core.fetchvars("tas_anom", (1850, 2014))[:, truth] + rng.normal(0.0, SIGMA, years.size)

    # the principal components of the simulated record, and what they know about the sensitivity
    co = core.comoments("tas_anom", (1850, 2014))
    scores = co.scores(core, "tas_anom", 3)
    ok = np.isfinite(scores).all(axis=0)
    share = co.pca(3)[1]
    for i in range(3):
        print("PC %d: %4.1f %% of the variance, correlation of its score with S %+.3f"
              % (i + 1, 100.0 * share[i], np.corrcoef(scores[i, ok], theta[0, ok])[0, 1]))

    # the gain from the two covariance verbs, and the update of every member from the projection
    c_y_theta = core.moments("tas_anom", (1850, 2014), against=list(theta)).cov     # [165, 3]
    gain = np.linalg.solve(co.cov + ALPHA * SIGMA ** 2 * np.eye(years.size), c_y_theta).T   # [3, 165]
    shift = core.project("tas_anom", years, gain, center=obs)                       # K (y - obs) [3, n]
    noise = np.linalg.cholesky(ALPHA * SIGMA ** 2 * gain @ gain.T) @ rng.normal(size=(3, n))
    new = np.where(np.isfinite(shift), theta - shift + noise, theta)
    for i, (cap, lo, hi, unit) in enumerate(PRIOR):
        new[i] = np.clip(new[i], lo, hi)
        print("%-8s prior %.3f +- %.3f   after the step %.3f +- %.3f   held-out member %.3f"
              % (cap(), theta[i].mean(), theta[i].std(), new[i].mean(), new[i].std(), theta[i, truth]))
        hector_amd.setvar(core, None, cap(), new[i], unit)
    hector_amd.reset(core)
    hector_amd.run(core, 2100)
    sd_post = spread(core, "after one step")
    core.drop_series("tas_anom")
    hector_amd.shutdown(core)
    return sd_prior, sd_post, theta, new


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
