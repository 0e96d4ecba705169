"""hx_member_pair_metrics (Core.pair_metrics): one number per member from a window of TWO series of
that member -- a regression of one output on another, or one output sampled where the other crosses
a threshold, peaks or bottoms out.

include/hector_amd.h fixes the order of every operation, in IEEE double without fused multiply-add,
so `numpy_pair_metric` below -- a Python loop over the years, vectorised over the members, on
fetchvars output, following those definitions literally -- reproduces the device result bit for bit:
no tolerance anywhere.  The kernel exchanges nothing between lanes, so the host-emulation build runs
it faithfully (CPU part); the same body runs on the GPU against the product library.
"""
import glob
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, PairMetric
from conftest import ROOT

RUN_TO = 2100
VAR_A, VAR_B = "CO2_concentration", "global_tas"
OPS = ("slope", "intercept", "r2", "at_first_ge", "at_max", "at_min", "mean_where_ge", "end_ratio")
BATCH = 8   # HXP_BATCH of hx_dev_post.h: rows of each operand a lane holds in flight
E = hector_amd.HectorAmdError


def _params(n):
    u = (np.arange(n) + 0.5) / n
    S = 1.5 + 4.5 * u
    q10 = 1.0 + 2.0 * np.fmod(np.arange(n) * 0.6180339887498949, 1.0)
    beta = 0.1 + 0.8 * np.fmod(np.arange(n) * 0.7548776662466927, 1.0)
    return S, q10, beta


def _core(n, lib, **kw):
    if lib is None:
        c = hector_amd.Core(n_members=n, device=0, **kw)
    else:
        c = hector_amd.Core(n_members=n, lib_path=lib, allow_emulation=True, **kw)
    S, q10, beta = _params(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10).setvar("beta", beta)
    return c


def _base(x, y0, period, bad):
    s = np.zeros(x.shape[1])
    for y in range(period[0], period[1] + 1):
        s = s + x[y - y0]
        bad |= np.isnan(x[y - y0])
    return s / float(period[1] - period[0] + 1)


def numpy_pair_metric(xa, xb, y0, m):
    """The exact sequence of include/hector_amd.h on xa, xb[year - y0, member] for one PairMetric
    (a vector b is passed broadcast to the members)."""
    n = xa.shape[1]
    bad = np.zeros(n, dtype=bool)
    base_a = _base(xa, y0, m.baseline, bad) if m.baseline is not None else None
    base_b = _base(xb, y0, m.baseline_b, bad) if m.baseline_b is not None else None
    year0, year1 = m.years

    def a_of(y):
        return xa[y - y0] - base_a if base_a is not None else xa[y - y0]

    def b_of(y):
        return xb[y - y0] - base_b if base_b is not None else xb[y - y0]

    thr = m.threshold
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if m.op == "end_ratio":
            for y in (year0, year1):
                bad |= np.isnan(xa[y - y0]) | np.isnan(xb[y - y0])
            out = (a_of(year1) - a_of(year0)) / (b_of(year1) - b_of(year0))
            return np.where(bad, np.nan, out)
        for y in range(year0, year1 + 1):
            bad |= np.isnan(xa[y - y0]) | np.isnan(xb[y - y0])
        if m.op in ("slope", "intercept", "r2"):
            cnt = float(year1 - year0 + 1)
            sa, sb = np.zeros(n), np.zeros(n)
            for y in range(year0, year1 + 1):
                sa = sa + a_of(y)
                sb = sb + b_of(y)
            ma, mb = sa / cnt, sb / cnt
            sab, sbb, saa = np.zeros(n), np.zeros(n), np.zeros(n)
            for y in range(year0, year1 + 1):
                da = a_of(y) - ma
                db = b_of(y) - mb
                pab = db * da
                pbb = db * db
                paa = da * da
                sab = sab + pab
                sbb = sbb + pbb
                saa = saa + paa
            slope = sab / sbb
            if m.op == "slope":
                out = slope
            elif m.op == "intercept":
                p = slope * mb
                out = ma - p
            else:
                num = sab * sab
                den = sbb * saa
                out = num / den
        elif m.op == "at_first_ge":
            out = np.full(n, np.nan)
            found = np.zeros(n, dtype=bool)
            for y in range(year0, year1 + 1):
                take = ~found & (b_of(y) >= thr)
                out = np.where(take, a_of(y), out)
                found |= take
        elif m.op in ("at_max", "at_min"):
            best, out = b_of(year0).copy(), a_of(year0).copy()
            for y in range(year0 + 1, year1 + 1):
                b = b_of(y)
                take = b > best if m.op == "at_max" else b < best
                best = np.where(take, b, best)
                out = np.where(take, a_of(y), out)
        else:   # mean_where_ge
            s, c = np.zeros(n), np.zeros(n)
            for y in range(year0, year1 + 1):
                ge = b_of(y) >= thr
                s = np.where(ge, s + a_of(y), s)
                c = np.where(ge, c + 1.0, c)
            out = s / c
    return np.where(bad, np.nan, out)


def _vec_block(years, values, y0, ny, n):
    """A caller's vector as an [ny, n] block on the core's rows (NaN outside its years)."""
    xb = np.full((ny, n), np.nan)
    for y, v in zip(years, values):
        if 0 <= y - y0 < ny:
            xb[y - y0] = v
    return xb


def _check(core, var_a, b, specs, xa=None, xb=None):
    y0 = core.strtdate
    if xa is None:
        xa = core.fetchvars(var_a, (y0, core.current_date))
    if xb is None:
        xb = core.fetchvars(b, (y0, core.current_date)) if isinstance(b, str) else \
            _vec_block(b[0], b[1], y0, xa.shape[0], xa.shape[1])
    got = core.pair_metrics(var_a, b, specs)
    assert got.shape == (len(specs), core.n_members)
    for k, m in enumerate(specs):
        ref = numpy_pair_metric(xa, xb, y0, m)
        assert np.array_equal(got[k], ref, equal_nan=True), (var_a, m, np.nanmax(np.abs(got[k] - ref)))
    return got


def _check_all_ops(core, xa, xb):
    y0 = core.strtdate
    win = (1950, RUN_TO)
    for base_a, base_b in ((None, None), ((1850, 1900), (1850, 1900))):
        # the ensemble median of the window maximum of b, from numpy alone: it splits this ensemble
        b = xb[win[0] - y0:win[1] - y0 + 1]
        if base_b is not None:
            b = b - _base(xb, y0, base_b, np.zeros(xb.shape[1], dtype=bool))
        thr = float(np.median(b.max(axis=0)))
        crosses = (b >= thr).any(axis=0)
        assert crosses.mean() >= 0.1 and (~crosses).mean() >= 0.1, crosses.mean()
        specs = [PairMetric(op, win, baseline=base_a, baseline_b=base_b, threshold=thr) for op in OPS]
        got = _check(core, VAR_A, VAR_B, specs, xa, xb)
        for op in OPS:
            if op in ("at_first_ge", "mean_where_ge"):
                assert np.array_equal(np.isnan(got[OPS.index(op)]), ~crosses), op
            else:
                assert np.isfinite(got[OPS.index(op)]).all(), op
        # the operands the other way round
        _check(core, VAR_B, VAR_A, [PairMetric(op, win, baseline=base_a, baseline_b=base_b, threshold=400.0)
                                    for op in OPS], xb, xa)


def _check_window_shapes(core, xa, xb):
    y0 = core.strtdate
    thr = float(np.median(xb[-1]))
    # every op on windows of 1, 2, batch - 1, batch, batch + 1 and 2 batch + 1 years, from startDate, from
    # inside the record, and ending at the current date
    for length in (1, 2, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1):
        for start in (y0, 1900, RUN_TO - length + 1):
            specs = [PairMetric(op, (start, start + length - 1), threshold=thr) for op in OPS]
            got = _check(core, VAR_A, VAR_B, specs, xa, xb)
            if length == 1:   # 0 / 0: no special case
                for op in ("slope", "intercept", "r2", "end_ratio"):
                    assert np.isnan(got[OPS.index(op)]).all(), op
                assert np.array_equal(got[OPS.index("at_max")], xa[start - y0])
    # reference periods for a only, for b only, for both, overlapping the window and disjoint from it, of
    # every length around the batch
    specs = [PairMetric("slope", (y0, RUN_TO), baseline=(1850, 1900)),
             PairMetric("intercept", (1950, 2000), baseline_b=(1850, 1900)),
             PairMetric("r2", (1950, 2000), baseline=(1960, 1960 + BATCH), baseline_b=(1990, 2010)),
             PairMetric("at_first_ge", (2000, RUN_TO), baseline=(y0, y0), baseline_b=(1850, 1900), threshold=1.5),
             PairMetric("at_first_ge", (2000, RUN_TO), baseline_b=(1850, 1900), threshold=2.0),
             PairMetric("at_max", (y0, RUN_TO), baseline=(RUN_TO - BATCH + 1, RUN_TO)),
             PairMetric("at_min", (y0, y0 + 2 * BATCH), baseline_b=(y0, y0 + BATCH - 2)),
             PairMetric("mean_where_ge", (1900, RUN_TO), baseline=(1850, 1900), baseline_b=(1850, 1900), threshold=1.0),
             PairMetric("end_ratio", (1850, RUN_TO), baseline=(1850, 1900), baseline_b=(1986, 2005)),
             PairMetric("end_ratio", (y0, RUN_TO))]
    _check(core, VAR_A, VAR_B, specs, xa, xb)
    # 32 specifications in one call
    many = [PairMetric(OPS[k % 8], (1760 + 7 * k, 1760 + 7 * k + (k * 5) % 50 + (17 if k % 3 else 0)),
                       baseline=None if k % 4 == 0 else (1850 + k, 1880 + 2 * k),
                       baseline_b=None if k % 3 == 0 else (1800 + 2 * k, 1800 + 3 * k), threshold=0.3 + 0.02 * k)
            for k in range(32)]
    _check(core, VAR_A, VAR_B, many, xa, xb)
    # one specification as a bare PairMetric
    assert core.pair_metrics(VAR_A, VAR_B, PairMetric("at_max", 2000)).shape == (1, core.n_members)


def _check_vector_b(core, xa):
    y0 = core.strtdate
    n = core.n_members
    # the years themselves: at_first_ge with threshold Y is the row of year Y
    years = np.arange(y0, RUN_TO + 1)
    for Y in (y0, 1850, 2014, RUN_TO):
        got = core.pair_metrics(VAR_A, (years, years.astype(float)), [PairMetric("at_first_ge", (y0, RUN_TO), threshold=Y)])
        assert np.array_equal(got[0], xa[Y - y0])
    # a vector that covers part of the record only, and starts before startDate
    part = np.arange(y0 - 5, 2051)
    vals = np.cumsum(np.linspace(0.0, 12.0, part.size))   # "cumulative emissions"
    specs = [PairMetric(op, (1850, 2050), baseline=(1850, 1900), baseline_b=(y0, y0 + BATCH), threshold=500.0)
             for op in OPS] + [PairMetric("slope", (y0, y0 + 1)), PairMetric("end_ratio", (y0, 2050))]
    got = _check(core, VAR_A, (part, vals), specs, xa)
    assert np.isfinite(got[:3]).all()
    # a plateau that holds the maximum twice and the minimum twice: the first occurrence counts
    py = np.arange(1900, 1912)
    pv = np.array([3.0, 1.0, 5.0, 2.0, 9.0, 9.0, 4.0, -2.0, 0.0, -2.0, 9.0, 1.0])
    got = _check(core, VAR_A, (py, pv), [PairMetric("at_max", (1900, 1911)), PairMetric("at_min", (1900, 1911)),
                                         PairMetric("at_max", (1905, 1911)), PairMetric("at_min", (1908, 1911))], xa)
    assert np.array_equal(got[0], xa[1904 - y0]) and np.array_equal(got[1], xa[1907 - y0])
    assert np.array_equal(got[2], xa[1905 - y0]) and np.array_equal(got[3], xa[1909 - y0])
    assert got.shape == (4, n)


def _check_identities(core, xa):
    """What does not depend on the restatement: b the same variable as a, with the same baseline."""
    y0 = core.strtdate
    for base in (None, (1850, 1900)):
        win = (1950, RUN_TO)
        kw = dict(baseline=base, baseline_b=base)
        got = core.pair_metrics(VAR_A, VAR_A, [PairMetric("slope", win, **kw), PairMetric("r2", win, **kw),
                                               PairMetric("intercept", win, **kw), PairMetric("at_max", win, **kw),
                                               PairMetric("mean_where_ge", win, threshold=-np.inf, **kw)])
        ref = core.metrics(VAR_A, [Metric("max", win, baseline=base), Metric("mean", win, baseline=base)])
        assert (got[0] == 1.0).all() and (got[1] == 1.0).all() and (got[2] == 0.0).all()
        assert np.array_equal(got[3], ref[0]) and np.array_equal(got[4], ref[1])
    # a b that is constant over the window
    core.derive("pm_zero", "mul", VAR_A, 0.0)
    got = core.pair_metrics(VAR_A, "pm_zero", [PairMetric(op, (1950, 2000)) for op in ("slope", "intercept", "r2", "at_max")])
    assert np.isnan(got[:3]).all() and np.array_equal(got[3], xa[1950 - y0])
    core.drop_series("pm_zero")


def _check_nan_handling(core, xa, xb):
    """Series whose edge rows are NaN, as a and, separately, as b."""
    y0 = core.strtdate
    W, L = 11, 5
    core.derive("pm_run", "runmean", VAR_A, width=W, align="centred")   # NaN in y0 .. y0+4 and RUN_TO-4 .. RUN_TO
    core.derive("pm_delta", "delta", VAR_B, lag=L)                       # NaN in y0 .. y0+4
    lo, hi = y0 + (W - 1) // 2, RUN_TO - W // 2
    xr = core.fetchvars("pm_run", (y0, RUN_TO))
    xd = core.fetchvars("pm_delta", (y0, RUN_TO))
    assert np.isnan(xr[:lo - y0]).all() and np.isnan(xr[hi - y0 + 1:]).all() and np.isfinite(xr[lo - y0:hi - y0 + 1]).all()
    assert np.isnan(xd[:L]).all() and np.isfinite(xd[L:]).all()
    cases = []   # (specification, the years it reads)
    for op in OPS:
        for win, ba, bb in (((lo, hi), None, None), ((lo - 1, hi), None, None), ((lo, hi + 1), None, None),
                            ((1900, 1950), (lo, lo + 3), None), ((1900, 1950), (lo - 1, lo + 3), None),
                            ((1900, 1950), None, (hi - 2, hi)), ((1900, 1950), None, (hi - 2, hi + 1)),
                            ((lo - 2, hi + 2), None, None), ((y0 + L, 1800), None, None), ((y0 + L - 1, 1800), None, None)):
            rows = {win[0], win[1]} if op == "end_ratio" else set(range(win[0], win[1] + 1))
            read = [rows | (set(range(p[0], p[1] + 1)) if p is not None else set()) for p in (ba, bb)]   # of a, of b
            cases.append((PairMetric(op, win, baseline=ba, baseline_b=bb, threshold=-1e30), read))
    specs = [c[0] for c in cases[:32]], [c[0] for c in cases[32:64]], [c[0] for c in cases[64:]]
    run_nan, delta_nan = set(range(y0, lo)) | set(range(hi + 1, RUN_TO + 1)), set(range(y0, y0 + L))
    for a, b, xa_, xb_, which, nan_years in (("pm_run", VAR_B, xr, xb, 0, run_nan), (VAR_A, "pm_run", xa, xr, 1, run_nan),
                                             (VAR_A, "pm_delta", xa, xd, 1, delta_nan),
                                             ("pm_delta", VAR_B, xd, xb, 0, delta_nan)):
        got = np.concatenate([_check(core, a, b, s, xa_, xb_) for s in specs if s])
        for k, (m, read) in enumerate(cases):
            if read[which] & nan_years:
                assert np.isnan(got[k]).all(), (a, b, m)
            elif m.op not in ("slope", "intercept", "r2", "end_ratio") or m.years[1] > m.years[0]:
                assert np.isfinite(got[k]).all(), (a, b, m)
    core.drop_series("pm_run").drop_series("pm_delta")
    # a NaN INSIDE the window (a * v / v with v = 0 in 1920, 1 elsewhere): end_ratio does not read it
    years = np.arange(y0, RUN_TO + 1)
    v = np.where(years == 1920, 0.0, 1.0)
    core.derive("pm_hole", "mul", VAR_A, v, first_year=y0).derive("pm_hole", "div", "pm_hole", v, first_year=y0)
    xh = core.fetchvars("pm_hole", (y0, RUN_TO))
    assert np.isnan(xh[1920 - y0]).all() and np.array_equal(np.delete(xh, 1920 - y0, 0), np.delete(xa, 1920 - y0, 0))
    specs = [PairMetric(op, (1900, 1950), baseline=(1850, 1860), threshold=-1e30) for op in OPS] + \
            [PairMetric("end_ratio", (1920, 1950)), PairMetric("end_ratio", (1900, 1950), baseline=(1915, 1925)),
             PairMetric("end_ratio", (1900, 1950), baseline_b=(1915, 1925))]
    for a, b, xa_, xb_, ref_nan in (("pm_hole", VAR_B, xh, xb, (True, False)), (VAR_B, "pm_hole", xb, xh, (False, True))):
        got = _check(core, a, b, specs, xa_, xb_)
        k = OPS.index("end_ratio")
        assert np.isnan(np.delete(got[:len(OPS)], k, 0)).all() and np.isfinite(got[k]).all()
        assert np.isnan(got[len(OPS)]).all()
        assert np.isnan(got[len(OPS) + 1]).all() == ref_nan[0] and np.isnan(got[len(OPS) + 2]).all() == ref_nan[1]
        assert np.isfinite(got[len(OPS) + 1]).all() != ref_nan[0] and np.isfinite(got[len(OPS) + 2]).all() != ref_nan[1]
    core.drop_series("pm_hole")


def _raw(*fields):
    from hector_amd.core import _HxPairMetric

    class Raw(PairMetric):
        def _c(self):
            return _HxPairMetric(*fields)
    return [Raw("slope", 1900)]


def _check_errors(core):
    ok = PairMetric("slope", (1900, 1950))
    years = np.arange(1850, 2001)
    vec = (years, np.linspace(0.0, 1.0, years.size))
    fn = "hx_member_pair_metrics"
    bad = [("not enabled", "RF_tot", VAR_B, [ok]),
           ("not enabled", VAR_A, "RF_tot", [ok]),
           ("nspecs", VAR_A, VAR_B, []),
           ("nspecs", VAR_A, VAR_B, [ok] * 33),
           ("unknown op", VAR_A, VAR_B, _raw(8, 1900, 1950, 1, 0, 1, 0, 0, 0.0)),
           ("unknown op", VAR_A, VAR_B, _raw(-1, 1900, 1950, 1, 0, 1, 0, 0, 0.0)),
           ("year1 < year0", VAR_A, VAR_B, _raw(0, 1950, 1900, 1, 0, 1, 0, 0, 0.0)),
           ("window", VAR_A, VAR_B, [ok, PairMetric("at_max", (1900, RUN_TO + 1))]),
           ("window", VAR_A, VAR_B, [PairMetric("at_max", (core.strtdate - 1, 1900))]),
           ("window", VAR_A, vec, [PairMetric("at_max", (1849, 1900))]),
           ("window", VAR_A, vec, [PairMetric("at_max", (1900, 2001))]),
           ("reference period of a", VAR_A, VAR_B, [PairMetric("slope", (1900, 1950), baseline=(1850, RUN_TO + 1))]),
           ("reference period of a", VAR_A, VAR_B, [PairMetric("slope", (1900, 1950), baseline=(1700, 1900))]),
           ("reference period of b", VAR_A, VAR_B, [PairMetric("slope", (1900, 1950), baseline_b=(1850, RUN_TO + 1))]),
           ("reference period of b", VAR_A, vec, [PairMetric("slope", (1900, 1950), baseline_b=(1849, 1900))]),
           ("reference period of b", VAR_A, vec, [PairMetric("slope", (1900, 1950), baseline_b=(1990, 2001))]),
           ("threshold", VAR_A, VAR_B, [PairMetric("at_first_ge", (1900, 1950))]),
           ("threshold", VAR_A, VAR_B, [PairMetric("mean_where_ge", (1900, 1950))]),
           ("not finite in 1852", VAR_A, (years, np.where(years == 1852, np.nan, 1.0)), [ok]),
           ("not finite in 2000", VAR_A, (years, np.where(years == 2000, np.inf, 1.0)), [ok])]
    for msg, a, b, specs in bad:
        with pytest.raises(E, match=fn + ".*" + msg):
            core.pair_metrics(a, b, specs)
    # a series that ends before the current date: the window is held to the range where both are valid
    core.derive("pm_copy", "copy", VAR_B)
    core.pair_metrics(VAR_A, "pm_copy", [PairMetric("slope", (1900, RUN_TO))])
    core.drop_series("pm_copy")
    # both or neither of cap_b / b_vec: through the C function
    import ctypes
    from hector_amd.core import _HxPairMetric
    dp = ctypes.POINTER(ctypes.c_double)
    arr = (_HxPairMetric * 1)(ok._c())
    out = np.empty((1, core.n_members))
    v = np.ascontiguousarray(vec[1])
    lib = core._lib
    for cap_b, b_vec, what in ((VAR_B.encode(), v.ctypes.data_as(dp), "both"), (None, None, "neither")):
        rc = lib.hx_member_pair_metrics(core._h, VAR_A.encode(), cap_b, b_vec, 1850, 2000, ctypes.byref(arr), 1,
                                        out.ctypes.data_as(dp))
        msg = lib.hx_last_error().decode()
        assert rc != 0 and msg.startswith(fn) and "exactly one of cap_b" in msg and what in msg, msg
    rc = lib.hx_member_pair_metrics(core._h, VAR_A.encode(), VAR_B.encode(), None, 0, 0, ctypes.byref(arr), 1, None)
    assert rc != 0 and lib.hx_last_error().decode().startswith(fn + ": null argument")
    # what the binding refuses itself
    with pytest.raises(E, match="unknown op"):
        PairMetric("median", 1900)
    with pytest.raises(E, match="PairMetric objects"):
        core.pair_metrics(VAR_A, VAR_B, [Metric("mean", 1900)])
    assert core.current_date == RUN_TO


def _check_block_verbs_refused(core, lib):
    """The emulation build refuses the three ensemble-wide verbs by name, AFTER checking their arguments."""
    if lib is None:
        return
    ok = [PairMetric("slope", (1900, 1950))]
    calls = (("hx_pair_metric_quantiles", lambda a, b, s: core.pair_metric_quantiles(a, b, s, [0.5])),
             ("hx_pair_metric_probabilities", lambda a, b, s: core.pair_metric_probabilities(a, b, s, [0.0, 1.0])),
             ("hx_pair_metric_moments", lambda a, b, s: core.pair_metric_moments(a, b, s)))
    for fn, call in calls:
        for msg, a, b, s in (("not enabled", "RF_tot", VAR_B, ok), ("nspecs", VAR_A, VAR_B, []),
                             ("window", VAR_A, VAR_B, [PairMetric("r2", (1900, RUN_TO + 1))]),
                             ("threshold", VAR_A, VAR_B, [PairMetric("at_first_ge", (1900, 1950))]),
                             ("not finite in 1901", VAR_A, ((1900, 1901), (0.0, np.nan)), [PairMetric("slope", (1900, 1901))])):
            with pytest.raises(E, match=fn + ".*" + msg):
                call(a, b, s)
        with pytest.raises(E, match=fn + " is not available in the host-emulation build"):
            call(VAR_A, VAR_B, ok)
    with pytest.raises(E, match="hx_pair_metric_quantiles.*nprobs"):
        core.pair_metric_quantiles(VAR_A, VAR_B, ok, [])
    with pytest.raises(E, match="hx_pair_metric_probabilities.*ascending"):
        core.pair_metric_probabilities(VAR_A, VAR_B, ok, [1.0, 1.0])
    with pytest.raises(E, match="hx_pair_metric_moments.*negative"):
        core.pair_metric_moments(VAR_A, VAR_B, ok, weights=-np.ones(core.n_members))


def _body(n, lib):
    core = _core(n, lib)
    fresh = _core(3, lib)
    with pytest.raises(E, match="hx_member_pair_metrics.*run the core first"):
        fresh.pair_metrics(VAR_A, VAR_B, [PairMetric("at_max", fresh.strtdate)])
    fresh.shutdown()
    core.run(RUN_TO)
    y0 = core.strtdate
    before = {v: core.fetchvars(v, (y0, RUN_TO)) for v in (VAR_A, VAR_B)}
    xa, xb = before[VAR_A], before[VAR_B]
    status, ms = core.status(), core.last_run_ms()
    _check_all_ops(core, xa, xb)
    _check_window_shapes(core, xa, xb)
    _check_vector_b(core, xa)
    _check_identities(core, xa)
    _check_nan_handling(core, xa, xb)
    _check_errors(core)
    _check_block_verbs_refused(core, lib)
    # pair metrics read results: they change none of them, and neither do the refused calls
    for v in (VAR_A, VAR_B):
        assert np.array_equal(before[v], core.fetchvars(v, (y0, RUN_TO)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    specs = [PairMetric(op, (1950, RUN_TO), baseline=(1850, 1900), baseline_b=(1850, 1900), threshold=0.9) for op in OPS]
    sorted_lanes = core.pair_metrics(VAR_A, VAR_B, specs)
    core.shutdown()
    # another lane order, the same members: the same bits
    plain = _core(n, lib)
    plain.set_member_sorting(False)
    plain.run(RUN_TO)
    assert np.array_equal(plain.lane_of_member(), np.arange(n))
    got = _check(plain, VAR_A, VAR_B, specs)
    if all(np.array_equal(plain.fetchvars(v, (y0, RUN_TO)), before[v]) for v in (VAR_A, VAR_B)):
        assert np.array_equal(got, sorted_lanes, equal_nan=True)
    plain.shutdown()


def test_pair_metrics_equal_numpy_bit_for_bit_in_the_emulation(emul_lib):
    _body(200, emul_lib)


@pytest.mark.gpu
def test_pair_metrics_equal_numpy_bit_for_bit_on_the_gpu(hip_lib):
    _body(4096 + 37, None)


def test_nan_rule_of_the_checker_matches_the_definition():
    """The NaN rule on synthetic rows (no core): a NaN of a or b in the window or in a reference period
    makes every operation NaN (end_ratio: only in an end row or a reference period), one outside does not."""
    rng = np.random.default_rng(1)
    xa, xb = rng.normal(0, 1, (30, 8)), rng.normal(0, 1, (30, 8))
    xa[3, 1] = np.nan     # a's reference period 0..9 only
    xa[15, 2] = np.nan    # inside the window 10..19, not an end row
    xa[25, 3] = np.nan    # outside everything
    xb[22, 4] = np.nan    # b's reference period 20..24 only
    xb[19, 5] = np.nan    # the window's last row
    xb[3, 6] = np.nan     # a's reference period, but of b: not read
    for op in OPS:
        r = numpy_pair_metric(xa, xb, 0, PairMetric(op, (10, 19), baseline=(0, 9), baseline_b=(20, 24), threshold=-9.0))
        nan = {1, 4, 5} | (set() if op == "end_ratio" else {2})
        assert set(np.flatnonzero(np.isnan(r))) == nan, (op, r)
        r = numpy_pair_metric(xa, xb, 0, PairMetric(op, (10, 19), threshold=-9.0))
        assert set(np.flatnonzero(np.isnan(r))) == {5} | (set() if op == "end_ratio" else {2}), (op, r)


def test_sharded_core_pair_metrics_equal_the_single_core(emul_lib):
    n = 11   # 4 + 4 + 3
    one = _core(n, emul_lib)
    many = _core(n, emul_lib, devices=[0, 0, 0])
    for c in (one, many):
        c.run(2020)
    years = np.arange(1850, 2021)
    vec = (years, np.cumsum(np.linspace(0.5, 10.0, years.size)))
    specs = [PairMetric(op, (1900, 2020), baseline=(1850, 1900), baseline_b=(1850, 1900), threshold=0.5) for op in OPS] + \
            [PairMetric("at_max", 2020), PairMetric("slope", (1850, 2020))]
    for b in (VAR_B, vec):
        p, q = one.pair_metrics(VAR_A, b, specs), many.pair_metrics(VAR_A, b, specs)
        assert p.shape == q.shape == (len(specs), n) and np.array_equal(p, q, equal_nan=True)
        _check(many, VAR_A, b, specs)
    with pytest.raises(E, match="hx_member_pair_metrics.*window"):
        many.pair_metrics(VAR_A, VAR_B, [PairMetric("at_max", 2021)])
    with pytest.raises(E, match="hx_member_pair_metrics.*nspecs"):
        many.pair_metrics(VAR_A, VAR_B, [])
    for fn, call in (("hx_pair_metric_quantiles", lambda: many.pair_metric_quantiles(VAR_A, VAR_B, specs, [0.5])),
                     ("hx_pair_metric_probabilities", lambda: many.pair_metric_probabilities(VAR_A, vec, specs, [1.0])),
                     ("hx_pair_metric_moments", lambda: many.pair_metric_moments(VAR_A, VAR_B, specs))):
        with pytest.raises(E, match=fn + " is not available in the host-emulation build"):
            call()
    assert np.array_equal(one.status(), many.status())   # the refused calls poisoned nothing
    assert np.array_equal(one.pair_metrics(VAR_A, VAR_B, specs), many.pair_metrics(VAR_A, VAR_B, specs), equal_nan=True)
    one.shutdown(); many.shutdown()


def test_two_derived_diagnostics_stand_at_once(emul_lib):
    """a and b both derived on the device from recorded outputs: resolving b must not give up a's block."""
    c = _core(6, emul_lib)
    c.set_outputs(["global_tas", "CO2_concentration", "HL_pH", "LL_pH", "sst"])
    c.run(1900)
    specs = [PairMetric(op, (1800, 1900), baseline_b=(1745, 1760), threshold=0.0) for op in OPS]
    for other in ("HL_sst", "LL_sst"):   # both kept blocks taken by other diagnostics first
        c.metrics(other, [Metric("mean", 1900)])
    got = c.pair_metrics("pH", "ocean_tas", specs)
    xa = c.fetchvars("pH", (1745, 1900))
    xb = c.fetchvars("ocean_tas", (1745, 1900))
    for k, m in enumerate(specs):
        assert np.array_equal(got[k], numpy_pair_metric(xa, xb, 1745, m), equal_nan=True), m
    c.shutdown()


def test_pair_metric_kernel_has_no_contracted_multiply_add():
    """fp contraction is off for the pair-metric kernels: db * da and sab + p are a v_mul_f64 and a
    v_add_f64.  The only fused multiply-adds belong to the compiler's correctly rounded expansion of
    the fp64 divisions (v_div_scale .. v_div_fmas, v_div_fixup), ahead of their v_div_fixup."""
    files = glob.glob(os.path.join(ROOT, "hector_amd", "build", "hx_post-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not files:
        pytest.skip("no assembly in hector_amd/build (the library was not built in this tree)")
    text = open(files[0], errors="replace").read()
    names = re.findall(r"^(_Z\d+hx_pair_metric_kernel\w*):", text, flags=re.M)
    assert len(names) == 2   # BVEC false and true
    for name in names:
        k = text.index(name + ":")
        body = text[k:text.index(".Lfunc_end", k)]
        ops = re.findall(r"^\s+(v_\w+_f64\w*)", body, flags=re.M)
        assert "v_mul_f64" in ops and "v_add_f64" in ops
        # a division is two v_div_scale .. one v_div_fixup; the scheduler interleaves two of them (ma, mb)
        scales = fixups = 0
        for op in ops:
            if op.startswith("v_div_scale"):
                scales += 1
            elif op.startswith("v_div_fixup"):
                fixups += 1
            elif op.startswith("v_fma") or op.startswith("v_mac") or op.startswith("v_pk_fma"):
                assert scales > 2 * fixups, "a fused multiply-add outside a division: %r" % ops
        assert scales == 2 * fixups and fixups >= 2
