"""hx_group_quantiles / hx_group_probabilities / hx_group_moments (the groups= keyword of the summary
verbs of Core, hector_amd.GroupedMoments): the parts that need no GPU.

The kernels are cooperative (LDS atomics, cross-lane reductions), so the host-emulation build refuses
the three functions by name after the argument checks; the argument checks of the binding are raised
before the library is called.  The arithmetic of `GroupedMoments` is held against numpy's weighted
formulas in longdouble on hand-built sums.  The GPU part is tests/test_gpu_grouped_summaries.py.

Tolerances of the arithmetic test: the raw sums are handed over rounded to float64 (one rounding,
2^-53 each), and mean, var, between and within are each a handful of float64 operations on them; the
data are drawn so that the cancellation var = B/W - (A/W)^2 loses less than a factor 1e3 (asserted as
kappa below), hence rel 1e-12 on the variances and the partition, and 1e-14 on means and shares.
"""
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import GroupedMoments, Metric, Moments, ensemble
from conftest import ROOT, SCENARIO

E = hector_amd.HectorAmdError
LD = np.longdouble
FNS = ("hx_group_quantiles", "hx_group_probabilities", "hx_group_moments")


def test_the_symbols_are_declared_documented_and_exported(emul_lib):
    from hector_amd import _lib
    lib = _lib.load(emul_lib, allow_emulation=True)
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert "#define HX_GROUP_MAX 16" in text
    for fn in FNS:
        assert fn in _lib.ABI_SYMBOLS
        getattr(lib, fn)
        assert re.search(r"\bint %s\(hx_core \*core, const char \*capability, int year0, int year1, "
                         r"const hx_metric \*specs,\s+int nspecs, const int \*labels, int ngroups" % fn, text)
    assert hector_amd.core.GROUP_MAX == 16


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def _calls(c, lab):
    spec = [Metric("max", (1750, 1760))]
    w = np.linspace(0.1, 1.0, c.n_members)
    return (("hx_group_quantiles", lambda: c.quantiles("global_tas", (0.1, 0.9), (1750, 1760), groups=lab)),
            ("hx_group_quantiles", lambda: c.metric_quantiles("global_tas", spec, 0.5, weights=w, groups=(lab, 4))),
            ("hx_group_probabilities", lambda: c.probabilities("global_tas", [0.1], weights=w, groups=lab)),
            ("hx_group_probabilities", lambda: c.metric_probabilities("global_tas", spec, [0.1, 0.2], groups=lab)),
            ("hx_group_moments", lambda: c.moments("global_tas", (1750, 1760), groups=lab)),
            ("hx_group_moments", lambda: c.moments("global_tas", weights=w, against=["S", "q10_rh"], groups=lab)),
            ("hx_group_moments", lambda: c.metric_moments("global_tas", spec, against="S", groups=(lab, 3))))


def test_every_verb_is_refused_by_name_in_the_emulation(emul_lib):
    lab = np.array([0, 1, 2, -1, 0, 1, 2, 0])
    for devices in (None, [0, 0]):
        c = _core(8, emul_lib, devices=devices)
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        for fn, call in _calls(c, lab):
            with pytest.raises(E, match="^" + fn + " is not available in the host-emulation build"):
                call()
        # the library's own argument checks come first and name the function
        with pytest.raises(E, match="hx_group_quantiles: a probability outside \\[0, 1\\]"):
            c.quantiles("global_tas", 1.5, groups=lab)
        with pytest.raises(E, match="hx_group_quantiles: no member has a label >= 0"):
            c.quantiles("global_tas", 0.5, groups=(np.full(8, -1), 2))
        with pytest.raises(E, match="hx_group_probabilities: the edges are not strictly ascending"):
            c.probabilities("global_tas", [1.0, 1.0], groups=lab)
        with pytest.raises(E, match="hx_group_moments: dates must lie between startDate and the current date"):
            c.moments("global_tas", (1750, 1900), groups=lab)
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_argument_errors_are_raised_before_the_call(emul_lib):
    c = _core(8, emul_lib)   # (not run: a call that reached the library would say so, or refuse by name)
    spec = [Metric("mean", (1750, 1760))]
    good = np.arange(8) % 2
    verbs = (("quantiles", lambda g: c.quantiles("global_tas", 0.5, groups=g)),
             ("metric_quantiles", lambda g: c.metric_quantiles("global_tas", spec, 0.5, groups=g)),
             ("probabilities", lambda g: c.probabilities("global_tas", [0.0], groups=g)),
             ("metric_probabilities", lambda g: c.metric_probabilities("global_tas", spec, [0.0], groups=g)),
             ("moments", lambda g: c.moments("global_tas", groups=g)),
             ("metric_moments", lambda g: c.metric_moments("global_tas", spec, groups=g)))
    for what, call in verbs:
        with pytest.raises(E, match="^%s: groups must have n_members labels" % what):
            call(np.zeros(7, dtype=np.int32))
        with pytest.raises(E, match="^%s: groups must have n_members labels" % what):
            call(np.zeros((8, 1), dtype=np.int32))
        with pytest.raises(E, match="^%s: the labels of groups must be integers" % what):
            call(np.zeros(8))
        with pytest.raises(E, match="^%s: the labels of groups must be integers" % what):
            call(good.astype(bool))
        with pytest.raises(E, match="^%s: label -2 lies outside -1..1" % what):
            call(np.where(np.arange(8) == 3, -2, good))
        with pytest.raises(E, match="^%s: label 5 lies outside -1..2" % what):
            call((np.where(np.arange(8) == 3, 5, good), 3))
        with pytest.raises(E, match="^%s: the number of groups must lie in 1..16 \\(it is 17\\)" % what):
            call(np.arange(8) * 2 + 2)
        with pytest.raises(E, match="^%s: the number of groups must lie in 1..16 \\(it is 17\\)" % what):
            call((good, 17))
        with pytest.raises(E, match="^%s: the number of groups must lie in 1..16 \\(it is 0\\)" % what):
            call(np.full(8, -1))
        with pytest.raises(E, match="^%s: the number of groups must be an integer" % what):
            call((good, 2.0))
        # a call that passes the binding reaches the library: the core has not run
        with pytest.raises(E, match="hx_group_(quantiles|probabilities|moments): "):
            call(good)
    with pytest.raises(E, match="^moments: weights must have n_members entries"):
        c.moments("global_tas", weights=np.ones(3), groups=good)
    with pytest.raises(E, match="^quantiles: probs must be one-dimensional"):
        c.quantiles("global_tas", np.zeros((2, 2)), groups=good)
    c.shutdown()


# ---- the arithmetic of GroupedMoments ---------------------------------------------------------------

def _hand(x, q, lab, G, pred):
    """The definition of include/hector_amd.h by hand: x[R, n], q[n] uint64, lab[n], pred[K, n] ->
    (shift[G, R], sums[G, R, 2 + 3 K] longdouble, wsum, n_part, pshift[G, K])."""
    R, n = x.shape
    K = pred.shape[0]
    shift = np.full((G, R), np.nan)
    sums = np.zeros((G, R, 2 + 3 * K), dtype=LD)
    wsum = np.zeros((G, R), dtype=np.uint64)
    npart = np.zeros((G, R), dtype=np.int64)
    pshift = np.full((G, K), np.nan)
    for g in range(G):
        ok = (lab == g) & (q > 0) & np.isfinite(pred).all(axis=0)
        if ok.any():
            pshift[g] = pred[:, ok].min(axis=1)
        for r in range(R):
            on = ok & ~np.isnan(x[r])
            if not on.any():
                continue
            shift[g, r] = x[r, on].min()
            d = (x[r, on] - shift[g, r]).astype(LD)
            w = q[on].astype(LD)
            wsum[g, r] = q[on].sum(dtype=np.uint64)
            npart[g, r] = on.sum()
            sums[g, r, 0], sums[g, r, 1] = (w * d).sum(), (w * d * d).sum()
            for k in range(K):
                e = (pred[k, on] - pshift[g, k]).astype(LD)
                sums[g, r, 2 + 3 * k:5 + 3 * k] = (w * e).sum(), (w * e * e).sum(), (w * d * e).sum()
    return shift, sums, wsum, npart, pshift


def _data():
    rng = np.random.default_rng(77)
    n, G = 600, 4
    lab = rng.integers(-1, G, n)
    q = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    q[rng.random(n) < 0.1] = 0
    x = np.stack([rng.normal(3.0, 1.0, n) + 0.8 * lab,            # groups differ in the mean
                  rng.normal(-2.0, 0.5, n),                       # ... or do not
                  np.where(lab == 2, np.nan, rng.normal(0, 1, n)),   # group 2 takes no part
                  np.full(n, 1.75),                               # zero variance everywhere
                  np.where(lab == 1, 4.0, 2.0).astype(np.float64),   # zero variance INSIDE the groups only
                  np.full(n, np.nan)])                            # nobody
    pred = np.stack([rng.normal(0, 1, n), rng.uniform(5, 6, n)])
    pred[1, 5] = np.nan
    return x, q, lab, G, pred


def test_grouped_moments_against_numpy_in_longdouble():
    x, q, lab, G, pred = _data()
    R = x.shape[0]
    shift, sums, wsum, npart, pshift = _hand(x, q, lab, G, pred)
    gm = GroupedMoments(shift, sums.astype(np.float64), wsum, npart, ["p0", "p1"], pshift, q, pred, lab)
    assert len(gm) == gm.n_groups == G and "GroupedMoments" in repr(gm)
    assert (npart[2, 2] == 0) and (npart[:, 5] == 0).all() and (npart[:, :2] > 0).all()
    ok = (q > 0) & np.isfinite(pred).all(axis=0) & (lab >= 0)
    kappa = 0.0
    for r in range(R):
        on = ok & ~np.isnan(x[r])
        if not on.any():
            for f in (gm.weight_share[:, r], gm.pooled_mean[r], gm.pooled_var[r], gm.between[r], gm.within[r],
                      gm.eta2[r]):
                assert np.isnan(f).all(), r
            continue
        w = q[on].astype(LD)
        xl = x[r, on].astype(LD)
        W = w.sum()
        mean = (w * xl).sum() / W
        var = (w * (xl - mean) ** 2).sum() / W                    # the variance of the union
        between = within = LD(0)
        for g in range(G):
            og = on & (lab == g)
            share = q[og].astype(LD).sum() / W
            assert gm.weight_share[g, r] == pytest.approx(float(share), rel=1e-14, abs=0)
            if not og.any():
                assert gm.weight_share[g, r] == 0 and np.isnan(gm[g].mean[r])
                continue
            wg, xg = q[og].astype(LD), x[r, og].astype(LD)
            mg = (wg * xg).sum() / wg.sum()
            vg = (wg * (xg - mg) ** 2).sum() / wg.sum()
            between += share * (mg - mean) ** 2
            within += share * vg
            assert gm[g].mean[r] == pytest.approx(float(mg), rel=1e-14)
            if vg > 0:
                kappa = max(kappa, float((sums[g, r, 1] / wg.sum()) / vg))
                assert gm[g].var[r] == pytest.approx(float(vg), rel=1e-12)
            else:
                assert gm[g].var[r] == 0.0
        assert float(abs(between + within - var)) <= 1e-15 * float(var) + 1e-300   # the law of total variance
        assert gm.pooled_mean[r] == pytest.approx(float(mean), rel=1e-14)
        assert gm.between[r] == pytest.approx(float(between), rel=1e-12, abs=1e-28)
        assert gm.within[r] == pytest.approx(float(within), rel=1e-12, abs=1e-28)
        assert gm.pooled_var[r] == pytest.approx(float(var), rel=1e-12, abs=1e-28)
        assert gm.between[r] + gm.within[r] == gm.pooled_var[r]
        if var > 0:
            assert gm.eta2[r] == pytest.approx(float(between / var), rel=1e-12, abs=1e-26)
        else:
            assert np.isnan(gm.eta2[r])
    assert kappa < 1e3
    assert np.isnan(gm.eta2[3]) and gm.pooled_var[3] == 0.0          # zero variance: undefined
    assert gm.within[4] == 0.0 and gm.eta2[4] == 1.0                 # all of it between the groups
    assert 0.2 < gm.eta2[0] < 0.8 and gm.eta2[1] < 0.05
    assert np.isclose(np.nansum(gm.weight_share, axis=0)[:5], 1.0).all()


def test_a_group_is_a_moments_with_its_own_shifts_weights_and_predictors():
    x, q, lab, G, pred = _data()
    shift, sums, wsum, npart, pshift = _hand(x, q, lab, G, pred)
    gm = GroupedMoments(shift, sums.astype(np.float64), wsum, npart, ["p0", "p1"], pshift, q, pred, lab)
    for g in range(G):
        m = gm[g]
        assert isinstance(m, Moments) and m.names == ["p0", "p1"]
        assert np.array_equal(m.pshift, pshift[g]) and np.array_equal(m.wsum, wsum[g])
        qg = np.where(lab == g, q, 0).astype(np.uint64)
        # the same object built by hand from the masked weights, as G masked calls would return it
        ref = Moments(shift[g], sums[g].astype(np.float64), wsum[g], npart[g], ["p0", "p1"], pshift[g], qg, pred)
        assert np.array_equal(m.src(), ref.src(), equal_nan=True)
        og = (qg > 0) & np.isfinite(pred).all(axis=0)
        rows = npart[g] == og.sum()
        assert rows.any() and np.isfinite(m.src()[rows][:2]).all()   # the two rows with a spread inside the group
        wl = qg[og].astype(LD)
        pm = (wl * pred[0, og].astype(LD)).sum() / wl.sum()
        assert m.pmean[0, 0] == pytest.approx(float(pm), rel=1e-13)
    with pytest.raises(IndexError):
        gm[G]
    with pytest.raises(E, match="2 \\+ 3 \\* len\\(names\\)"):
        GroupedMoments(shift, sums.astype(np.float64), wsum, npart, ["p0"])
    with pytest.raises(E, match="\\[groups, rows\\]"):
        GroupedMoments(shift[0], sums[0].astype(np.float64), wsum[0], npart[0], ["p0", "p1"])
