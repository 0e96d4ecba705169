"""Series and derived diagnostics under the ensemble-wide verbs, on the GPU: the emissions what-if
difference, its weighted quantiles and class probabilities, and the quantiles of a crossing year of
a centred 20-year running mean -- on the pair kernel, the one-wavefront kernel, its two-wave flavour
and a core of two shards -- against numpy on fetched data.

References: `numpy_series` / `numpy_metric` of tests/test_device_series.py (the literal definitions
of include/hector_amd.h), and, restated here, the weighted inverted-CDF `checker` and the exact
integer `bin_reference` that tests/test_gpu_quantiles.py and tests/test_gpu_metrics_probabilities.py
define.  Everything is compared with `==`.
"""
import math

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import SCENARIO
from test_device_series import numpy_series, numpy_metric, DERIVED

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
RUN_TO = 2100


def quantise(w):
    return np.rint(w / w.max() * 2.0 ** 32).astype(np.uint64)


def checker(x, q, probs):
    """x[n] values, q[n] uint64 weights -> (quantiles[len(probs)], members taking part)."""
    part = ~np.isnan(x) & (q > 0)
    v, w = x[part], q[part]
    if v.size == 0:
        return np.full(len(probs), np.nan), 0
    order = np.argsort(v, kind="stable")
    vs, cum = v[order], np.cumsum(w[order], dtype=np.uint64)
    W = int(cum[-1])
    assert W <= 2 ** 52
    out = np.empty(len(probs))
    for j, p in enumerate(probs):
        t = max(1, math.ceil(p * float(W)))
        out[j] = vs[int(np.searchsorted(cum, np.uint64(t), side="left"))]
    return out, int(v.size)


def bin_reference(x, q, edges):
    """x[n], q[n] uint64 -> (sums[len(edges) + 1] uint64, members taking part)."""
    part = ~np.isnan(x) & (q > 0)
    sums = np.zeros(len(edges) + 1, dtype=np.uint64)
    np.add.at(sums, np.searchsorted(np.asarray(edges, dtype=np.float64), x[part], side="right"), q[part])
    return sums, int(part.sum())


def check_quantile_rows(x, got, npart, weights, probs, what):
    q = np.ones(x.shape[1], dtype=np.uint64) if weights is None else quantise(weights)
    for y in range(x.shape[0]):
        ref, cnt = checker(x[y], q, probs)
        assert npart[y] == cnt, (what, y, npart[y], cnt)
        if cnt == 0:
            assert np.isnan(got[y]).all(), (what, y, got[y])
        else:
            assert (got[y] == ref).all(), (what, y, got[y], ref)


def check_bin_rows(x, res, weights, edges, what):
    prob, npart, sums = res
    q = np.ones(x.shape[1], dtype=np.uint64) if weights is None else quantise(weights)
    assert prob.shape == sums.shape == (x.shape[0], len(edges) + 1) and sums.dtype == np.uint64
    for y in range(x.shape[0]):
        ref, cnt = bin_reference(x[y], q, edges)
        assert npart[y] == cnt, (what, y, npart[y], cnt)
        assert (sums[y] == ref).all(), (what, y, sums[y], ref)
        if cnt == 0:
            assert np.isnan(prob[y]).all(), (what, y, prob[y])
        else:
            assert (prob[y] == ref.astype(np.float64) / float(int(ref.sum(dtype=np.uint64)))).all(), (what, y)


def _core(n, hip_lib, pair_limit=None, two_wave=None, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    c.setvar("beta", 0.2 + 0.6 * np.fmod(np.arange(n) * 0.7548776662466927, 1.0))
    if pair_limit is not None:
        c.set_pair_kernel_limit(pair_limit)
    if two_wave is not None:
        c.set_two_wave_from(two_wave)
    return c


def _score_weights(core):
    """exp(-chi2 / 2) of CO2 1850-2014 against member 0 plus seeded noise, as a calibration does."""
    years = np.arange(1850, 2015)
    rng = np.random.default_rng(5)
    truth = core.fetchvars("CO2_concentration", (1850, 2014))[:, 0]
    obs = truth + rng.normal(0.0, 1.0, years.size)
    chi2 = core.score("CO2_concentration", years, obs, sigma=np.full(years.size, 4.0))
    w = np.exp(-0.5 * (chi2 - chi2.min()))
    w[core.status() != 0] = 0.0
    return w


def _whatif(core, kernel):
    """Hold global_tas, cut the emissions from 2030 on, run again: the per-member avoided warming,
    its band and classes, and when a centred 20-year mean of the new warming crosses 1.5 degC."""
    y0 = core.strtdate
    core.run(RUN_TO)
    assert kernel is None or core.last_run_kernel() == kernel
    w = _score_weights(core)
    assert (quantise(w) == 0).any() and (quantise(w) > 0).sum() > 10
    before = core.fetchvars("global_tas", (y0, RUN_TO))
    core.hold("base", "global_tas")
    yrs = np.arange(2030, RUN_TO + 1)
    core.setvar_dated("ffi_emissions", yrs, np.full(yrs.size, 2.0), "Pg C/yr")
    core.reset(0)
    core.run(RUN_TO)
    after = core.fetchvars("global_tas", (y0, RUN_TO))
    assert np.array_equal(core.fetchvars("base", (y0, RUN_TO)), before)
    core.derive("d", "sub", "global_tas", "base")
    d = core.fetchvars("d", (y0, RUN_TO))
    assert np.array_equal(d, after - before, equal_nan=True) and np.nanmedian(d[-1]) < 0
    rows = (RUN_TO - 5, RUN_TO)
    x = d[rows[0] - y0:]
    edges = tuple(float(v) for v in np.nanquantile(x[-1], [0.2, 0.5, 0.8]))
    for weights in (None, w):
        got, npart = core.quantiles("d", PROBS, rows, weights=weights, counts=True)
        check_quantile_rows(x, got, npart, weights, PROBS, ("d", weights is not None))
        res = core.probabilities("d", edges, rows, weights=weights, counts=True, sums=True)
        check_bin_rows(x, res, weights, edges, ("d", weights is not None))
    # the crossing year of the centred 20-year mean of the anomaly against 1850-1900
    core.derive("anom", "anomaly", "global_tas", years=(1850, 1900))
    core.derive("rm", "runmean", "anom", width=20, align="centred")
    ref = numpy_series("runmean", numpy_series("anomaly", after, y0=y0, years=(1850, 1900)), y0=y0,
                       width=20, align="centred")
    assert np.array_equal(core.fetchvars("rm", (y0, RUN_TO)), ref, equal_nan=True)
    spec = Metric("first_ge", (1900, RUN_TO - 10), threshold=1.5)
    m = numpy_metric(ref, y0, spec)
    assert 0 < np.isnan(m).mean() < 1                # some members cross, some do not
    assert np.array_equal(core.metrics("rm", [spec])[0], m, equal_nan=True)
    for weights in (None, w):
        got, npart = core.metric_quantiles("rm", [spec], PROBS, weights=weights, counts=True)
        check_quantile_rows(m[None, :], got, npart, weights, PROBS, ("crossing year", weights is not None))
        res = core.metric_probabilities("rm", [spec], (2030.0, 2050.0), weights=weights, counts=True, sums=True)
        check_bin_rows(m[None, :], res, weights, (2030.0, 2050.0), ("crossing classes", weights is not None))
    assert core.series() == {"base": RUN_TO, "d": RUN_TO, "anom": RUN_TO, "rm": RUN_TO}
    core.shutdown()


def test_whatif_on_the_pair_kernel(hip_lib):
    _whatif(_core(1024, hip_lib), "pair")


def test_whatif_on_the_one_wavefront_kernel(hip_lib):
    _whatif(_core(65536, hip_lib), "run")


def test_whatif_on_the_two_wave_flavour(hip_lib):
    _whatif(_core(131072, hip_lib), "run2")


def test_whatif_on_a_core_of_two_shards(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    core = _core(2 * 512 + 5, hip_lib, pair_limit=0, devices=[0, 0])
    assert core.shards()[1] == [0, 515, 1029]
    _whatif(core, None)


def test_ensemble_wide_verbs_on_derived_diagnostics(hip_lib):
    n = 1000
    core = _core(n, hip_lib)
    core.set_outputs(["CO2_concentration", "global_tas"] + list(DERIVED))
    core.run(RUN_TO)
    y0 = core.strtdate
    w = _score_weights(core)
    rows = (2040, 2050)
    for name in DERIVED:
        full = core.fetchvars(name, (y0, RUN_TO))
        x = full[rows[0] - y0:rows[1] - y0 + 1]
        edges = tuple(float(v) for v in np.nanquantile(x[-1], [0.3, 0.7]))
        for weights in (None, w):
            got, npart = core.quantiles(name, PROBS, rows, weights=weights, counts=True)
            check_quantile_rows(x, got, npart, weights, PROBS, (name, weights is not None))
            res = core.probabilities(name, edges, rows, weights=weights, counts=True, sums=True)
            check_bin_rows(x, res, weights, edges, (name, weights is not None))
        spec = Metric("mean", (2081, RUN_TO), baseline=(1986, 2005))
        got, npart = core.metric_quantiles(name, [spec], PROBS, counts=True)
        check_quantile_rows(numpy_metric(full, y0, spec)[None, :], got, npart, None, PROBS, (name, "metric"))
        # {count, sum, sum of squares, min, max}: count, min and max exactly; the sums are reduced in
        # another order than numpy's: n terms, each rounding at most eps relative to the sum of |x|
        st = core.ensemble_stats([name], rows)[0]
        eps = np.finfo(np.float64).eps
        assert (st[:, 0] == n).all() and (st[:, 3] == x.min(axis=1)).all() and (st[:, 4] == x.max(axis=1)).all()
        assert (np.abs(st[:, 1] - x.sum(axis=1)) <= n * eps * np.abs(x).sum(axis=1)).all()
        assert (np.abs(st[:, 2] - (x * x).sum(axis=1)) <= 2 * n * eps * (x * x).sum(axis=1)).all()
    # a recorded output: every verb returns exactly what it did before an unrelated series existed
    spec = [Metric("max", (1950, RUN_TO), baseline=(1850, 1900))]

    def verbs():
        return (core.quantiles("global_tas", PROBS, rows, weights=w), core.probabilities("global_tas", (1.5, 2.0), rows, weights=w),
                core.metrics("global_tas", spec), core.metric_quantiles("global_tas", spec, PROBS, weights=w),
                core.metric_probabilities("global_tas", spec, (1.5, 2.0), weights=w),
                core.ensemble_stats(["global_tas"], rows), core.fetchvars("global_tas", rows))
    ref = verbs()
    core.derive("unrelated", "mul", "CO2_concentration", -7.0)
    for a, b in zip(verbs(), ref):
        assert np.array_equal(a, b, equal_nan=True)
    core.shutdown()
