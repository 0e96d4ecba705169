"""Core.metric_quantiles, Core.probabilities and Core.metric_probabilities on the GPU.

Authorities, all numpy on the host and all integer where sums are concerned:
  * `checker` (the one of tests/test_gpu_quantiles.py, copied): the weighted inverted-CDF quantile of
    a row, applied here to the rows Core.metrics() returns;
  * `bin_reference`: np.searchsorted(edges, x, side="right") and np.add.at on uint64 with the
    quantised weights q = rint(w / wmax * 2^32).
Everything is compared with `==`; prob is compared with sums / sums.sum() evaluated in double.
"""
import ctypes
import math

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import SCENARIO

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
EDGES = (1.5, 2.0, 3.0)
BASE = (1850, 1900)


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
        print("quantile row", what, y, "members", npart[y], cnt)
        assert npart[y] == cnt, (what, y, npart[y], cnt)
        if cnt == 0:
            assert np.isnan(got[y]).all(), (what, y, got[y])
        else:
            assert (got[y] == ref).all(), (what, y, got[y], ref)


def check_bin_rows(x, res, weights, edges, what):
    """x[rows, n]; res = (prob, counts, sums) of a probabilities call."""
    prob, npart, sums = res
    q = np.ones(x.shape[1], dtype=np.uint64) if weights is None else quantise(weights)
    assert prob.shape == sums.shape == (x.shape[0], len(edges) + 1) and sums.dtype == np.uint64
    for y in range(x.shape[0]):
        ref, cnt = bin_reference(x[y], q, edges)
        assert npart[y] == cnt, (what, y, npart[y], cnt)
        assert (sums[y] == ref).all(), (what, y, sums[y], ref)
        if cnt == 0:
            assert np.isnan(prob[y]).all() and (sums[y] == 0).all(), (what, y, prob[y])
        else:
            W = int(ref.sum(dtype=np.uint64))
            assert (prob[y] == ref.astype(np.float64) / float(W)).all(), (what, y, prob[y])
            assert prob[y].sum() == pytest.approx(1.0, abs=1e-12)


def _core(n, hip_lib, pair_limit=None, two_wave=None, beta=True, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    if beta:
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


def _specs(y0, y1):
    """The user's numbers: end-of-window warming, peak and its year, crossing year, years above,
    trend -- relative to 1850-1900 -- and a plain one-year mean."""
    return [Metric("mean", (y1 - 19, y1), baseline=BASE),
            Metric("max", (y0, y1), baseline=BASE),
            Metric("year_of_max", (y0, y1), baseline=BASE),
            Metric("first_ge", (y0, y1), baseline=BASE, threshold=1.5),
            Metric("count_ge", (y0, y1), baseline=BASE, threshold=2.0),
            Metric("slope", (y0, min(y0 + 35, y1)), baseline=BASE),
            Metric("min", (y0, y1)),
            Metric("mean", y1)]


def _check_flavour(core, years, row_years):
    """metric_quantiles / metric_probabilities over _specs(*years) and probabilities over the rows
    row_years, unweighted and with score weights some of which quantise to 0."""
    w = _score_weights(core)
    assert (quantise(w) == 0).any() and (quantise(w) > 0).sum() > 10
    specs = _specs(*years)
    m = core.metrics("global_tas", specs)
    x = core.fetchvars("global_tas", row_years)
    for weights in (None, w):
        tag = (core.last_run_kernel(), weights is not None)
        got, npart = core.metric_quantiles("global_tas", specs, PROBS, weights=weights, counts=True)
        assert got.shape == (len(specs), len(PROBS))
        check_quantile_rows(m, got, npart, weights, PROBS, tag)
        # a one-year mean without a baseline is that year's row: quantiles() must agree exactly
        assert np.array_equal(got[-1], core.quantiles("global_tas", PROBS, (years[1], years[1]), weights=weights)[0])
        check_bin_rows(m, core.metric_probabilities("global_tas", specs, EDGES, weights=weights, counts=True,
                                                    sums=True), weights, EDGES, tag)
        check_bin_rows(x, core.probabilities("global_tas", EDGES, row_years, weights=weights, counts=True,
                                             sums=True), weights, EDGES, tag)
        # edges some members sit on exactly: the value lies in the upper bin
        q = np.ones(core.n_members, dtype=np.uint64) if weights is None else quantise(weights)
        part = ~np.isnan(m[0]) & (q > 0)
        held = m[0][part]
        on = tuple(np.unique(held[[1, held.size // 2, held.size - 2]]))
        res = core.metric_probabilities("global_tas", specs[:1], on, weights=weights, counts=True, sums=True)
        check_bin_rows(m[:1], res, weights, on, tag)
        below = int(q[part & (m[0] < on[0])].sum(dtype=np.uint64))
        at_or_above = int(q[part & (m[0] >= on[0])].sum(dtype=np.uint64))   # the members ON on[0] included
        assert int(res[2][0][0]) == below and int(res[2][0][1:].sum(dtype=np.uint64)) == at_or_above
    # the plain return values
    assert np.array_equal(core.probabilities("global_tas", EDGES, row_years),
                          core.probabilities("global_tas", EDGES, row_years, counts=True)[0])


def test_pair_kernel_ensemble(hip_lib):
    core = _core(1000, hip_lib)
    core.run(2300)
    assert core.last_run_kernel() == "pair"
    _check_flavour(core, (1850, 2300), (1745, 2300))
    core.shutdown()


def test_full_size_ensemble_on_the_one_wavefront_kernel(hip_lib):
    core = _core(65536, hip_lib)
    core.run(2300)
    assert core.last_run_kernel() == "run"
    _check_flavour(core, (1850, 2300), (1745, 2300))
    core.shutdown()


def test_two_wave_ensemble(hip_lib):
    core = _core(131072, hip_lib, beta=False)
    core.run(2300)
    assert core.last_run_kernel() == "run2"
    _check_flavour(core, (1850, 2300), (2250, 2300))
    core.shutdown()


def _hip_runtime():
    """The HIP runtime that is already in the process (the library's own)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in the process")


def _write_row(core, var, year, values, pad_value):
    """values[n_members] (member order) into the recorded row of `year`, through the device
    pointer of hx_device_var; the padding lanes get pad_value (they never take part)."""
    ptr, npad = core.device_var(var)
    assert core.strtdate <= year <= core.current_date and npad >= core.n_members
    row = np.full(npad, pad_value)
    row[core.lane_of_member()] = values
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    dst = ptr + (year - core.strtdate) * npad * 8
    assert hip.hipMemcpy(ctypes.c_void_p(dst), row.ctypes.data_as(ctypes.c_void_p), npad * 8, 1) == 0


def test_hostile_rows(hip_lib):
    n = 777   # 13 wavefronts, 55 padding lanes
    core = _core(n, hip_lib)
    core.run(1800)
    rng = np.random.default_rng(3)
    tiny = 5e-324
    e31 = np.linspace(-3.0, 3.0, 31)
    e7 = np.array([-1e300, -1.0, -tiny, 0.0, tiny, 1.0, 1e300])
    rows = {
        "all equal": np.full(n, 3.25),
        "both zeros, an edge at 0.0": rng.choice([-0.0, 0.0, -tiny, tiny, -1.0, 1.0], n),
        "denormals": rng.integers(-40, 40, n) * tiny,
        "infinities": rng.choice([-np.inf, np.inf, 0.0, 1.0, -1.0], n),
        "NaN-laced": np.where(rng.random(n) < 0.4, np.nan, rng.normal(0, 1, n)),
        "all NaN": np.full(n, np.nan),
        "one value among NaN": np.where(np.arange(n) == 500, -7.0, np.nan),
        "exactly on every one of 31 edges": e31[rng.integers(0, 31, n)],
        "exactly on every one of 7 edges": e7[rng.integers(0, 7, n)],
        "full range": rng.normal(0, 1, n) * 10.0 ** rng.integers(-300, 300, n),
    }
    w_wide = 2.0 ** -rng.uniform(0, 40, n)      # some quantise to 0
    w_wide[rng.integers(0, n)] = 1.0
    w_one = np.zeros(n)
    w_one[123] = 0.7                            # one participating member
    assert (quantise(w_wide) == 0).any()
    edge_sets = (e31, e7, np.array([0.0]), np.array([3.25]), np.array([-40 * tiny, 0.0, 39 * tiny]))
    for k, (name, values) in enumerate(rows.items()):
        year = 1750 + k
        _write_row(core, "global_tas", year, values, pad_value=-1e300 if k % 2 else np.nan)
        x = core.fetchvars("global_tas", (year, year))
        assert np.array_equal(x[0], values, equal_nan=True)
        # the same row as a metric: a one-year mean without a baseline returns it (0.0 + x) / 1.0
        spec = [Metric("mean", year)]
        m = core.metrics("global_tas", spec)
        assert np.array_equal(m[0], values, equal_nan=True)
        for weights in (None, w_wide, w_one):
            tag = (name, None if weights is None else weights.max())
            for edges in edge_sets:
                check_bin_rows(x, core.probabilities("global_tas", edges, (year, year), weights=weights,
                                                     counts=True, sums=True), weights, edges, tag)
                check_bin_rows(m, core.metric_probabilities("global_tas", spec, edges, weights=weights,
                                                            counts=True, sums=True), weights, edges, tag)
            got, npart = core.metric_quantiles("global_tas", spec, PROBS, weights=weights, counts=True)
            check_quantile_rows(m, got, npart, weights, PROBS, tag)
    # all of them in one call, next to untouched rows; a hostile window through every metric
    x = core.fetchvars("global_tas", (1745, 1800))
    for weights in (None, w_wide):
        check_bin_rows(x, core.probabilities("global_tas", e31, weights=weights, counts=True, sums=True),
                       weights, e31, "all rows")
    specs = [Metric(op, (1745, 1800), threshold=0.0) for op in
             ("mean", "min", "max", "year_of_min", "year_of_max", "first_ge", "count_ge", "slope")]
    m = core.metrics("global_tas", specs)
    assert np.isnan(m).all()    # the all-NaN row lies in every member's window
    specs = [Metric(op, (1750, 1753), threshold=0.0) for op in ("min", "max", "count_ge", "first_ge")]
    m = core.metrics("global_tas", specs)
    assert np.array_equal(m[0], x[5:9].min(axis=0)) and np.array_equal(m[1], x[5:9].max(axis=0))
    check_bin_rows(m, core.metric_probabilities("global_tas", specs, e7, counts=True, sums=True), None, e7, "window")
    core.shutdown()


@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_core_equals_one_core(hip_lib, monkeypatch, shards):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    n = shards * 512 + 5
    one = _core(n, hip_lib, pair_limit=0)
    many = _core(n, hip_lib, pair_limit=0, devices=[0] * shards)
    for c in (one, many):
        c.run(1900, wait=False)
    x = one.fetchvars("global_tas", (1745, 1900))
    assert np.array_equal(x, many.fetchvars("global_tas", (1745, 1900)))
    rng = np.random.default_rng(shards)
    w = rng.random(n) ** 12
    w[:700] = 0.0                    # (the whole first shard of eight, and more, left out)
    w[n - 1] = 5.0                   # the largest weight lives on the last shard
    specs = [Metric("mean", (1881, 1900), baseline=(1745, 1800)), Metric("max", (1745, 1900)),
             Metric("year_of_max", (1745, 1900)), Metric("first_ge", (1745, 1900), threshold=float(np.median(x.max(axis=0)))),
             Metric("slope", (1850, 1900)), Metric("mean", 1900)]
    edges = tuple(np.quantile(x[-1], [0.2, 0.5, 0.9])) + (float(x[-1][n - 1]),)
    edges = tuple(sorted(set(edges)))
    m = one.metrics("global_tas", specs)
    assert np.array_equal(m, many.metrics("global_tas", specs), equal_nan=True)
    for weights in (None, w):
        a, na = one.metric_quantiles("global_tas", specs, PROBS, weights=weights, counts=True)
        b, nb = many.metric_quantiles("global_tas", specs, PROBS, weights=weights, counts=True)
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(na, nb)
        check_quantile_rows(m, b, nb, weights, PROBS, (shards, weights is not None))
        ra = one.probabilities("global_tas", edges, (1745, 1900), weights=weights, counts=True, sums=True)
        rb = many.probabilities("global_tas", edges, (1745, 1900), weights=weights, counts=True, sums=True)
        assert all(np.array_equal(p, r, equal_nan=True) for p, r in zip(ra, rb))
        check_bin_rows(x, rb, weights, edges, (shards, weights is not None))
        ra = one.metric_probabilities("global_tas", specs, edges, weights=weights, counts=True, sums=True)
        rb = many.metric_probabilities("global_tas", specs, edges, weights=weights, counts=True, sums=True)
        assert all(np.array_equal(p, r, equal_nan=True) for p, r in zip(ra, rb))
        check_bin_rows(m, rb, weights, edges, (shards, weights is not None))
    one.shutdown(); many.shutdown()


def test_errors_name_their_function_and_leave_the_core_usable(hip_lib):
    n = 512
    core = _core(n, hip_lib)
    fresh = _core(n, hip_lib)
    ok = [Metric("mean", (1800, 1850))]
    E = hector_amd.HectorAmdError
    for fn, call in (("hx_member_metrics", lambda c: c.metrics("global_tas", [Metric("mean", c.strtdate)])),
                     ("hx_metric_quantiles", lambda c: c.metric_quantiles("global_tas", [Metric("mean", c.strtdate)], [0.5])),
                     ("hx_ensemble_probabilities", lambda c: c.probabilities("global_tas", [1.0])),
                     ("hx_metric_probabilities", lambda c: c.metric_probabilities("global_tas", [Metric("mean", c.strtdate)], [1.0]))):
        with pytest.raises(E, match=fn + ".*run the core first"):
            call(fresh)
    core.run(1850)
    before = core.fetchvars("global_tas", (1745, 1850))
    status, ms = core.status(), core.last_run_ms()
    w = np.ones(n)
    from hector_amd.core import _HxMetric

    def raw(*fields):
        class Raw(Metric):
            def _c(self):
                return _HxMetric(*fields)
        return [Raw("mean", 1800)]

    bad_specs = [("not enabled", "RF_tot", ok), ("nspecs", "global_tas", []), ("nspecs", "global_tas", ok * 33),
                 ("unknown op", "global_tas", raw(8, 1800, 1850, 1, 0, 0, 0.0)),
                 ("year1 < year0", "global_tas", raw(0, 1850, 1800, 1, 0, 0, 0.0)),
                 ("window", "global_tas", [Metric("mean", (1800, 1851))]),
                 ("window", "global_tas", [Metric("mean", (1744, 1850))]),
                 ("reference period", "global_tas", [Metric("mean", (1800, 1850), baseline=(1745, 1851))]),
                 ("threshold", "global_tas", [Metric("first_ge", (1800, 1850))]),
                 ("threshold", "global_tas", [Metric("count_ge", (1800, 1850))])]
    bad_weights = [("negative", np.where(np.arange(n) == 3, -1.0, w)), ("NaN", np.where(np.arange(n) == 3, np.nan, w)),
                   ("infinite", np.where(np.arange(n) == 3, np.inf, w)), ("all zero", np.zeros(n))]
    bad_edges = [("nedges", []), ("nedges", np.arange(32.0)), ("ascending", [1.0, 1.0]), ("ascending", [2.0, 1.0]),
                 ("finite", [0.0, np.inf]), ("finite", [np.nan]), ("finite", [-np.inf, 0.0])]
    bad_probs = [[], np.linspace(0, 1, 17), [1.5], [float("nan")]]
    for msg, var, specs in bad_specs:
        for fn, call in (("hx_member_metrics", lambda: core.metrics(var, specs)),
                         ("hx_metric_quantiles", lambda: core.metric_quantiles(var, specs, [0.5])),
                         ("hx_metric_probabilities", lambda: core.metric_probabilities(var, specs, [1.0]))):
            with pytest.raises(E, match=fn + ".*" + msg):
                call()
    for msg, wt in bad_weights:
        for fn, call in (("hx_metric_quantiles", lambda: core.metric_quantiles("global_tas", ok, [0.5], weights=wt)),
                         ("hx_ensemble_probabilities", lambda: core.probabilities("global_tas", [1.0], weights=wt)),
                         ("hx_metric_probabilities", lambda: core.metric_probabilities("global_tas", ok, [1.0], weights=wt))):
            with pytest.raises(E, match=fn + ".*" + msg):
                call()
    for msg, ed in bad_edges:
        for fn, call in (("hx_ensemble_probabilities", lambda: core.probabilities("global_tas", ed)),
                         ("hx_metric_probabilities", lambda: core.metric_probabilities("global_tas", ok, ed))):
            with pytest.raises(E, match=fn + ".*" + msg):
                call()
    for pr in bad_probs:
        with pytest.raises(E, match="hx_metric_quantiles"):
            core.metric_quantiles("global_tas", ok, pr)
    with pytest.raises(E, match="hx_ensemble_probabilities.*not enabled"):
        core.probabilities("RF_tot", [1.0])
    with pytest.raises(E, match="hx_ensemble_probabilities.*current date"):
        core.probabilities("global_tas", [1.0], dates=(1745, 1851))
    # the verbs themselves, and the refused calls, changed nothing
    good = core.metric_quantiles("global_tas", ok, PROBS, weights=w)
    assert np.array_equal(good, core.metric_quantiles("global_tas", ok, PROBS))
    core.probabilities("global_tas", [0.1, 0.2])
    core.metric_probabilities("global_tas", ok, [0.1, 0.2])
    assert np.array_equal(before, core.fetchvars("global_tas", (1745, 1850)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    # ... and the core goes on as a fresh one does
    core.run(1900)
    fresh.run(1850)
    fresh.run(1900)
    assert np.array_equal(core.fetchvars("global_tas", (1745, 1900)), fresh.fetchvars("global_tas", (1745, 1900)))
    core.shutdown(); fresh.shutdown()
