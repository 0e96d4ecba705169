"""hx_ensemble_moments / hx_metric_moments (Core.moments, Core.metric_moments) on the GPU.

The authority is `checker` below: with q = quantise(w) as in tests/test_gpu_quantiles.py it applies the
participation rule of include/hector_amd.h (q > 0, value not NaN, every predictor finite), takes c_y
and c_k as exact minima, forms d = x - c_y and e_k = p_k - c_k in float64 (that rounding is part of
the definition) and accumulates the five kinds of sums in np.longdouble.

Exact (`==`): n_part, wsum, shift; rows whose participants are all equal (every sum 0, var 0); two
identical calls; weights=None against weights of all ones.

Sums: |S - S_ref| <= (n_part + 8) 2^-53 S_ref.  Every term is >= 0 and carries at most three
roundings (q d, then d or e_k; the product with q e_k likewise), and a sum of n non-negative terms in
ANY order is within (n - 1) 2^-53 of the exact sum, relatively: the bound holds for every summation
order, lane order and shard split.

Derived statistics (mean, var, cov, corr) against numpy's weighted formulas on the raw fetchvars data
in longdouble, relative tolerance 4 kappa (n_part + 8) 2^-53, where kappa = (B/W) / var is the
cancellation in var = B/W - (A/W)^2 (mean and var), and kappa_x kappa_p, with kappa_p = (D/W) / pvar,
for cov and corr: |E/W| <= sqrt(B/W D/W), so the cancellation in cov is bounded by the product.  Rows
whose reference var is 0 are left out of these comparisons -- at most the first two years of the
range -- and kappa <= 3e4 is asserted over all others.  global_tas is the one variable here whose
members stay identical for longer: the temperature component sees no forcing before 1751, so the six
rows 1745-1750 are all-equal rows.  Its range for the derived comparisons is therefore 1749-2300
(`first=4`): exactly its first two years, 1749 and 1750, must be the zero-variance rows, and the four
rows before the range, 1745-1748, are held to the exact all-equal check (every sum 0, var 0) instead.
"""
import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import SCENARIO

pytestmark = pytest.mark.gpu

E = hector_amd.HectorAmdError
U = 2.0 ** -53
KAPPA_MAX = 3e4
PARAMS = ("S", "q10_rh", "beta")
LD = np.longdouble


def quantise(w):
    return np.rint(w / w.max() * 2.0 ** 32).astype(np.uint64)


def _q(n, weights):
    return np.ones(n, dtype=np.uint64) if weights is None else quantise(np.asarray(weights, dtype=np.float64))


def checker(x, q, pred):
    """x[ny, n], q[n] uint64, pred[K, n] -> dict of shift[ny], wsum[ny], n_part[ny], sums[ny, 2 + 3K]
    (longdouble), pshift[K], ok[n]."""
    ny, n = x.shape
    k = pred.shape[0]
    ok = (q > 0) & (np.isfinite(pred).all(axis=0) if k else np.ones(n, dtype=bool))
    pshift = pred[:, ok].min(axis=1) if ok.any() else np.full(k, np.nan)
    shift = np.full(ny, np.nan)
    wsum, npart = np.zeros(ny, dtype=np.uint64), np.zeros(ny, dtype=np.int64)
    sums = np.zeros((ny, 2 + 3 * k), dtype=LD)
    idx = np.flatnonzero(ok)
    wl_all = q[idx].astype(LD)
    e_all = [(pred[j, idx] - pshift[j]) for j in range(k)]          # float64: one IEEE subtraction
    for y in range(ny):
        xv = x[y, idx]
        part = ~np.isnan(xv)
        if not part.any():
            continue
        full = part.all()
        xp = xv if full else xv[part]
        wl = wl_all if full else wl_all[part]
        shift[y] = xp.min()
        d = xp - shift[y]                                            # float64: one IEEE subtraction
        assert (d >= 0).all()
        wsum[y] = np.uint64(int(q[idx].sum(dtype=np.uint64)) if full else int(q[idx][part].sum(dtype=np.uint64)))
        npart[y] = xp.size
        dl = d.astype(LD)
        wd = wl * dl
        sums[y, 0], sums[y, 1] = wd.sum(), (wd * dl).sum()
        for j in range(k):
            el = (e_all[j] if full else e_all[j][part]).astype(LD)
            we = wl * el
            sums[y, 2 + 3 * j], sums[y, 3 + 3 * j], sums[y, 4 + 3 * j] = we.sum(), (we * el).sum(), (wd * el).sum()
    return dict(shift=shift, wsum=wsum, n_part=npart, sums=sums, pshift=pshift, ok=ok)


def check_raw(m, x, q, pred, what):
    """The exact fields with ==, every sum within the derived bound -> the checker's record."""
    ref = checker(x, q, pred)
    assert m.sums.shape == ref["sums"].shape, what
    assert np.array_equal(m.n_part, ref["n_part"]), (what, "n_part")
    assert np.array_equal(m.wsum, ref["wsum"]), (what, "wsum")
    assert np.array_equal(m.shift, ref["shift"], equal_nan=True), (what, "shift")
    assert np.array_equal(m.pshift, ref["pshift"], equal_nan=True), (what, "pshift")
    got = m.sums.astype(LD)
    bound = (ref["n_part"].astype(LD)[:, None] + 8) * LD(U) * ref["sums"]
    err = np.abs(got - ref["sums"])
    worst = float(np.max(np.where(ref["sums"] > 0, err / np.where(ref["sums"] > 0, bound, 1), 0)))
    print("%s: worst sum error / bound %.3g" % (what, worst))
    assert (err <= bound).all(), (what, worst, np.argwhere(err > bound)[:5])
    # rows whose participants are all equal: every sum exactly 0, var exactly 0
    for y in range(x.shape[0]):
        if ref["n_part"][y] and ref["sums"][y, 0] == 0 and ref["sums"][y, 1] == 0:
            k = pred.shape[0]
            assert (m.sums[y, [0, 1] + [4 + 3 * j for j in range(k)]] == 0).all() and m.var[y] == 0.0, (what, y)
    empty = ref["n_part"] == 0
    assert (m.sums[empty] == 0).all() and np.isnan(m.shift[empty]).all() and (m.wsum[empty] == 0).all()
    return ref


def check_derived(m, x, q, pred, ref, what, first=0):
    """mean, var, cov, corr against numpy's weighted formulas on the raw data in longdouble, over
    the rows from `first` on.  first > 0 (global_tas): the rows before it must be all-equal rows and
    the zero-variance rows of the range exactly its first two."""
    assert (ref["sums"][:first, :2] == 0).all() and (m.var[:first] == 0).all(), what
    ok = ref["ok"]
    idx = np.flatnonzero(ok)
    k = pred.shape[0]
    wl = q[idx].astype(LD)
    zero_rows, kmax = [], 0.0
    mean, var, cov, corr = m.mean, m.var, m.cov, m.corr
    for y in range(first, x.shape[0]):
        xv = x[y, idx]
        part = ~np.isnan(xv)
        assert part.any(), (what, y)
        w = wl[part] / wl[part].sum()
        xl = xv[part].astype(LD)
        rmean = (w * xl).sum()
        rvar = (w * (xl - rmean) ** 2).sum()
        if rvar == 0:
            zero_rows.append(y)
            continue
        W = LD(int(ref["wsum"][y]))
        kx = float((ref["sums"][y, 1] / W) / rvar)
        tol = 4.0 * (ref["n_part"][y] + 8) * U
        kmax = max(kmax, kx)
        assert abs(LD(mean[y]) - rmean) <= tol * kx * abs(rmean), (what, y, "mean", mean[y], rmean)
        assert abs(LD(var[y]) - rvar) <= tol * kx * rvar, (what, y, "var", var[y], rvar, kx)
        for j in range(k):
            pl = pred[j, idx][part].astype(LD)
            pmean = (w * pl).sum()
            pvar = (w * (pl - pmean) ** 2).sum()
            assert pvar > 0, (what, y, j)
            rcov = (w * (xl - rmean) * (pl - pmean)).sum()
            rcorr = rcov / np.sqrt(rvar * pvar)
            kk = kx * float((ref["sums"][y, 3 + 3 * j] / W) / pvar)
            kmax = max(kmax, kk)
            assert abs(LD(cov[y, j]) - rcov) <= tol * kk * abs(rcov), (what, y, j, "cov", cov[y, j], rcov, kk)
            assert abs(LD(corr[y, j]) - rcorr) <= tol * kk * abs(rcorr), (what, y, j, "corr", corr[y, j], rcorr, kk)
    print("%s: max kappa %.4g, zero-variance rows %r" % (what, kmax, zero_rows))
    assert len(zero_rows) <= 2 and all(y < first + 2 for y in zero_rows), (what, zero_rows)
    if first:
        assert zero_rows == [first, first + 1], (what, zero_rows)
    assert kmax <= KAPPA_MAX, (what, kmax)


def same_bits(a, b):
    return (np.array_equal(a.shift, b.shift, equal_nan=True) and np.array_equal(a.sums, b.sums) and
            np.array_equal(a.wsum, b.wsum) and np.array_equal(a.n_part, b.n_part))


def within_bound(a, b, what):
    """Two lane orders / shard layouts of the same members: exact fields equal, sums within twice
    the bound of each against the exact sum."""
    assert np.array_equal(a.n_part, b.n_part) and np.array_equal(a.wsum, b.wsum), what
    assert np.array_equal(a.shift, b.shift, equal_nan=True), what
    lim = 2 * (a.n_part[:, None] + 8) * U * np.maximum(a.sums, b.sums)
    assert (np.abs(a.sums - b.sums) <= lim).all(), what


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


def _score_weights(core, sigma=4.0):
    """exp(-chi2 / 2) of CO2 1850-2014 against member 0 plus seeded noise, as a calibration does."""
    years = np.arange(1850, 2015)
    rng = np.random.default_rng(5)
    truth = core.fetchvars("CO2_concentration", (1850, 2014))[:, 0]
    obs = truth + rng.normal(0.0, 1.0, years.size)
    chi2 = core.score("CO2_concentration", years, obs, sigma=np.full(years.size, sigma))
    w = np.exp(-0.5 * (chi2 - chi2.min()))
    w[core.status() != 0] = 0.0
    return w


def _params(core, names=PARAMS):
    return np.stack([core.getvar(p) for p in names])


def _eight(core):
    """Eight predictors: the three parameters, two metrics, three arrays."""
    n = core.n_members
    i = np.arange(n)
    arrays = [np.fmod(i * 0.6180339887498949, 1.0), np.cos(i * 0.001) * 3.0 - 40.0, (i % 97).astype(np.float64)]
    mets = [("global_tas", Metric("mean", (1995, 2014), baseline=(1850, 1900))),
            ("CO2_concentration", Metric("max", (1745, 2100)))]
    against = list(PARAMS) + mets + arrays
    pred = np.concatenate([_params(core), core.metrics(*mets[0])[:1], core.metrics(*mets[1])[:1], np.stack(arrays)])
    return against, pred


def test_full_size_ensemble_on_the_one_wavefront_kernel(hip_lib):
    n = 65536
    core = _core(n, hip_lib)
    core.run(2300)
    assert core.last_run_kernel() == "run"
    w = _score_weights(core)
    assert (quantise(w) == 0).any() and (quantise(w) > 0).sum() > 10
    pred = _params(core)
    for var in ("CO2_concentration", "global_tas"):
        x = core.fetchvars(var, (1745, 2300))
        for weights in (None, w):
            what = (var, "weighted" if weights is not None else "unweighted")
            m = core.moments(var, (1745, 2300), weights=weights, against=list(PARAMS))
            assert m.names == list(PARAMS) and m.sums.shape == (556, 11)
            ref = check_raw(m, x, _q(n, weights), pred, what)
            check_derived(m, x, _q(n, weights), pred, ref, what, first=4 if var == "global_tas" else 0)
            assert same_bits(m, core.moments(var, (1745, 2300), weights=weights, against=list(PARAMS))), what
        # no predictors; weights=None is weights of all ones: the same statistics bit for bit, the raw
        # sums scaled by exactly 2^32 (q = 1 against q = 2^32)
        m0 = core.moments(var, (1745, 2300))
        ref0 = check_raw(m0, x, _q(n, None), np.empty((0, n)), (var, "npred 0"))
        check_derived(m0, x, _q(n, None), np.empty((0, n)), ref0, (var, "npred 0"),
                      first=4 if var == "global_tas" else 0)
        m1 = core.moments(var, (1745, 2300), weights=np.ones(n))
        assert np.array_equal(m1.sums, m0.sums * 2.0 ** 32) and np.array_equal(m1.wsum, m0.wsum << np.uint64(32))
        assert np.array_equal(m1.shift, m0.shift) and np.array_equal(m1.n_part, m0.n_part)
        for f in ("mean", "var"):
            assert np.array_equal(getattr(m0, f), getattr(m1, f), equal_nan=True), (var, f)
        a3, b3 = core.moments(var, (2000, 2100), against=list(PARAMS)), \
            core.moments(var, (2000, 2100), weights=np.ones(n), against=list(PARAMS))
        for f in ("mean", "var", "pmean", "pvar", "cov", "corr", "slope"):
            assert np.array_equal(getattr(a3, f), getattr(b3, f), equal_nan=True), (var, f)
        assert np.array_equal(a3.src(), b3.src(), equal_nan=True)
    # eight predictors, two of them metrics
    against, pred8 = _eight(core)
    x = core.fetchvars("global_tas", (2000, 2100))
    for weights in (None, w):
        m8 = core.moments("global_tas", (2000, 2100), weights=weights, against=against)
        assert m8.sums.shape == (101, 26) and len(m8.names) == 8
        ref8 = check_raw(m8, x, _q(n, weights), pred8, ("npred 8", weights is not None))
        check_derived(m8, x, _q(n, weights), pred8, ref8, ("npred 8", weights is not None))
        assert np.isfinite(m8.src()).all()
    core.shutdown()


def _small_checks(core, years, w, what):
    n = core.n_members
    pred = _params(core)
    out = {}
    for var in ("CO2_concentration", "global_tas"):
        x = core.fetchvars(var, years)
        for weights in (None, w):
            m = core.moments(var, years, weights=weights, against=list(PARAMS))
            check_raw(m, x, _q(n, weights), pred, (what, var, weights is not None))
            assert same_bits(m, core.moments(var, years, weights=weights, against=list(PARAMS)))
            out[(var, weights is not None)] = (x, m)
    return out


def test_pair_kernel_ensemble(hip_lib):
    core = _core(1000, hip_lib)
    core.run(2300)
    assert core.last_run_kernel() == "pair"
    _small_checks(core, (1745, 2300), _score_weights(core), "pair")
    core.shutdown()


def test_two_wave_ensemble(hip_lib):
    core = _core(131072, hip_lib, beta=False)
    core.run(2300)
    assert core.last_run_kernel() == "run2"
    _small_checks(core, (2250, 2300), _score_weights(core), "two-wave")
    core.shutdown()


@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_core_against_one_core(hip_lib, monkeypatch, shards):
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
    w[:700] = 0.0                    # a weight vector that zeroes whole shards (the first of two, more of eight)
    w[n - 1] = 5.0                   # the largest weight lives on the last shard
    pred = _params(one)
    for weights in (None, w):
        for against, p in ((list(PARAMS), pred), (None, np.empty((0, n)))):
            a = one.moments("global_tas", (1745, 1900), weights=weights, against=against)
            b = many.moments("global_tas", (1745, 1900), weights=weights, against=against)
            within_bound(a, b, (shards, weights is not None))
            check_raw(a, x, _q(n, weights), p, ("one", shards, weights is not None))
            check_raw(b, x, _q(n, weights), p, ("many", shards, weights is not None))
            assert same_bits(b, many.moments("global_tas", (1745, 1900), weights=weights, against=against))
    specs = [Metric("mean", (1880, 1900), baseline=(1750, 1800)), Metric("slope", (1850, 1900))]
    a = one.metric_moments("global_tas", specs, weights=w, against=list(PARAMS))
    b = many.metric_moments("global_tas", specs, weights=w, against=list(PARAMS))
    within_bound(a, b, (shards, "metrics"))
    check_raw(b, one.metrics("global_tas", specs), _q(n, w), pred, (shards, "metrics"))
    one.shutdown(); many.shutdown()


def test_member_sorting_on_and_off(hip_lib):
    res = []
    for sorting in (True, False):
        core = _core(3000, hip_lib, pair_limit=0)
        core.set_member_sorting(sorting)
        core.run(1900)
        rng = np.random.default_rng(11)
        w = rng.random(3000) ** 8
        x = core.fetchvars("global_tas", (1745, 1900))
        m = core.moments("global_tas", (1745, 1900), weights=w, against=list(PARAMS))
        check_raw(m, x, _q(3000, w), _params(core), ("sorting", sorting))
        res.append((x, m))
        core.shutdown()
    if np.array_equal(res[0][0], res[1][0]):   # (the same trajectories: then the same sums within the bound)
        within_bound(res[0][1], res[1][1], "sorting on against off")


def test_derived_diagnostic_series_metrics_and_nan_predictors(hip_lib):
    n = 2000
    core = _core(n, hip_lib, pair_limit=0)
    core.run(2100)
    rng = np.random.default_rng(23)
    w = rng.random(n) ** 6
    pred = _params(core)
    q = _q(n, w)
    # a derived diagnostic and a series as the variable
    core.derive("warming", "anomaly", "global_tas", years=(1850, 1900))
    for var, years in (("slr", (1900, 2100)), ("warming", (1850, 2100))):
        x = core.fetchvars(var, years)
        m = core.moments(var, years, weights=w, against=list(PARAMS))
        check_raw(m, x, q, pred, var)
    # metric_moments against metrics() + the checker
    specs = [Metric("mean", (2081, 2100), baseline=(1850, 1900)), Metric("max", (1745, 2100)),
             Metric("first_ge", (1850, 2100), baseline=(1850, 1900), threshold=2.0),
             Metric("slope", (2000, 2100)), Metric("year_of_max", (1745, 2100))]
    rows = core.metrics("global_tas", specs)
    assert np.isnan(rows[2]).any() and not np.isnan(rows[2]).all()
    for weights in (None, w):
        mm = core.metric_moments("global_tas", specs, weights=weights, against=list(PARAMS))
        assert mm.sums.shape == (5, 11)
        ref = check_raw(mm, rows, _q(n, weights), pred, ("metric_moments", weights is not None))
        assert ref["n_part"][2] == ((_q(n, weights) > 0) & ~np.isnan(rows[2])).sum() < ref["n_part"][0]
        assert np.isnan(mm.src()[2]).all() and np.isfinite(mm.src()[0]).all()
    # a metric predictor that is NaN for some members: n_part drops by exactly those members
    crossing = ("global_tas", specs[2])
    x = core.fetchvars("global_tas", (2000, 2100))
    base = core.moments("global_tas", (2000, 2100), weights=w, against=["S"])
    m = core.moments("global_tas", (2000, 2100), weights=w, against=["S", crossing])
    lost = int(((q > 0) & np.isnan(rows[2])).sum())
    assert lost > 0 and (base.n_part - m.n_part == lost).all()
    check_raw(m, x, q, np.stack([pred[0], rows[2]]), "NaN metric predictor")
    # infinities count as not finite; all predictors bad: nobody takes part
    p = pred[0].copy()
    p[5], p[6] = np.inf, -np.inf
    m = core.moments("global_tas", (2000, 2010), against=[p])
    assert (m.n_part == n - 2).all()
    check_raw(m, x[:11], _q(n, None), p[None, :], "infinite predictor")
    m = core.moments("global_tas", (2000, 2010), against=[np.full(n, np.nan)])
    assert (m.n_part == 0).all() and np.isnan(m.shift).all() and (m.sums == 0).all() and (m.wsum == 0).all()
    assert np.isnan(m.mean).all() and np.isnan(m.src()).all()
    core.shutdown()


def test_every_documented_error_and_nothing_changes(hip_lib):
    n = 512
    core = _core(n, hip_lib)
    fresh = _core(n, hip_lib)
    for fn, call in (("hx_ensemble_moments", lambda: fresh.moments("global_tas", (1745, 1745))),
                     ("hx_metric_moments", lambda: fresh.metric_moments("global_tas", [Metric("mean", 1745)]))):
        with pytest.raises(E, match=fn + ".*run the core first"):
            call()
    fresh.shutdown()
    core.run(1850)
    core.hold("held", "global_tas")
    before = core.fetchvars("global_tas", (1745, 1850))
    held = core.fetchvars("held", (1745, 1850))
    status, ms = core.status(), core.last_run_ms()
    w = np.ones(n)
    ok = [Metric("mean", (1800, 1850))]
    bad = [dict(weights=np.where(np.arange(n) == 3, -1.0, w)), dict(weights=np.where(np.arange(n) == 3, np.nan, w)),
           dict(weights=np.where(np.arange(n) == 3, np.inf, w)), dict(weights=np.zeros(n))]
    for kw in bad:
        with pytest.raises(E, match="hx_ensemble_moments"):
            core.moments("global_tas", against=["S"], **kw)
        with pytest.raises(E, match="hx_metric_moments"):
            core.metric_moments("global_tas", ok, against=["S"], **kw)
    for dates in ((1745, 1851), (1700, 1800)):
        with pytest.raises(E, match="hx_ensemble_moments.*current date"):
            core.moments("global_tas", dates)
    with pytest.raises(E, match="hx_ensemble_moments.*not enabled"):
        core.moments("RF_tot")
    with pytest.raises(E, match="hx_metric_moments.*not enabled"):
        core.metric_moments("RF_tot", ok)
    with pytest.raises(E, match="hx_ensemble_moments"):
        core.moments("no_such_variable")
    with pytest.raises(E, match="hx_metric_moments.*current date"):
        core.metric_moments("global_tas", [Metric("mean", (1800, 1851))])
    with pytest.raises(E, match="hx_metric_moments.*nspecs"):
        core.metric_moments("global_tas", [])
    # npred and predictors, through the C ABI (the binding refuses more than 8 entries itself)
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    shift, sums = np.empty(106), np.empty((106, 29))
    p9 = np.zeros((9, n))
    arr = (type(ok[0]._c()) * 1)(ok[0]._c())
    for npred, pp in ((9, p9.ctypes.data_as(dp)), (-1, p9.ctypes.data_as(dp)), (1, None)):
        rc = core._lib.hx_ensemble_moments(core._h, b"global_tas", 1745, 1850, None, pp, npred,
                                           shift.ctypes.data_as(dp), sums.ctypes.data_as(dp), None, None)
        assert rc != 0 and "hx_ensemble_moments" in core._lib.hx_last_error().decode()
        assert ("npred" if pp is not None else "NULL") in core._lib.hx_last_error().decode()
        rc = core._lib.hx_metric_moments(core._h, b"global_tas", ctypes.byref(arr), 1, None, pp, npred,
                                         shift.ctypes.data_as(dp), sums.ctypes.data_as(dp), None, None)
        assert rc != 0 and "hx_metric_moments" in core._lib.hx_last_error().decode()
    # the calls and the refused calls changed nothing
    good = core.moments("global_tas", weights=w, against=list(PARAMS))
    core.metric_moments("held", ok, against=["S"])
    assert np.array_equal(good.corr, core.moments("global_tas", against=list(PARAMS)).corr, equal_nan=True)
    assert np.array_equal(before, core.fetchvars("global_tas", (1745, 1850)))
    assert np.array_equal(held, core.fetchvars("held", (1745, 1850)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    # ... and the core goes on as a fresh one does
    core.run(1900)
    other = _core(n, hip_lib)
    other.run(1850)
    other.run(1900)
    assert np.array_equal(core.fetchvars("global_tas", (1745, 1900)), other.fetchvars("global_tas", (1745, 1900)))
    core.shutdown(); other.shutdown()
    # (the refusal of a communicator of several processes needs one GPU per rank: Fleet::refuse_processes,
    #  the same call the quantile and probability verbs make, is not exercised on a one-GPU box)
