"""Python face of the ensemble core, named after the reference's R API
(R/hector.R:57-189, R/messages.R:46-140, R/biome.R:61-130): newcore(), run(),
reset(), shutdown(), setvar(), fetchvars(), split_biome() -- with a member axis.
Everything here is a thin ctypes veneer over the C ABI (include/hector_amd.h);
the numerics live in the HIP kernels.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import HectorAmdError, DEFAULT_SCENARIO

# (the R-style capability accessors -- ECS(), BETA(biome) ... -- live in hector_amd.capabilities)


METRIC_OPS = {"mean": 0, "min": 1, "max": 2, "year_of_min": 3, "year_of_max": 4, "first_ge": 5,
              "count_ge": 6, "slope": 7}    # HX_MET_* of include/hector_amd.h


SERIES_OPS = {"copy": 0, "add": 1, "sub": 2, "mul": 3, "div": 4, "anomaly": 5, "cumsum": 6,
              "runmean": 7, "delta": 8}     # HX_SER_* of include/hector_amd.h


RANK_KINDS = {"pit": 0, "numerator": 1}     # HX_RANK_* of include/hector_amd.h


_SCORE_WHITENED_MAX = 256   # HX_SCORE_WHITENED_MAX
_PROJECT_MAX_OUT, _PROJECT_MAX_YEARS = 64, 1024   # HX_PROJECT_MAX_OUT, HX_PROJECT_MAX_YEARS


def _whiten(cov, who):
    C = np.asarray(cov, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 1:
        raise HectorAmdError("%s: the covariance must be a square matrix" % who)
    if not np.isfinite(C).all():
        raise HectorAmdError("%s: the covariance has a NaN or infinite entry" % who)
    if not (C == C.T).all():
        raise HectorAmdError("%s: the covariance is not symmetric" % who)
    try:
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError:
        raise HectorAmdError("%s: the covariance is not positive definite" % who) from None
    n = C.shape[0]
    W = np.tril(np.linalg.solve(L, np.eye(n)))
    return W, 2.0 * float(np.sum(np.log(np.diag(L))))


def whiten(cov):
    """-> (W, logdet) of an error covariance C = L L^T (Cholesky): W = L^-1, lower-triangular with an
    exact zero above the diagonal, so that r^T C^-1 r = |W r|^2 -- what Core.score(..., whiten=W)
    and hx_member_score_whitened take -- and logdet = log det C = 2 sum log diag L, the other half of
    the Gaussian log-likelihood.  C must be square, finite, symmetric and positive definite."""
    return _whiten(cov, "whiten")


class _HxSeriesOp(ctypes.Structure):   # hx_series_op
    _fields_ = [("op", ctypes.c_int), ("year0", ctypes.c_int), ("year1", ctypes.c_int),
                ("width", ctypes.c_int), ("align", ctypes.c_int), ("lag", ctypes.c_int),
                ("b_kind", ctypes.c_int), ("b_first_year", ctypes.c_int), ("b_n", ctypes.c_int),
                ("reserved", ctypes.c_int), ("b_scalar", ctypes.c_double), ("b", ctypes.c_char_p),
                ("b_values", ctypes.POINTER(ctypes.c_double))]


class _HxMetric(ctypes.Structure):   # hx_metric
    _fields_ = [("op", ctypes.c_int), ("year0", ctypes.c_int), ("year1", ctypes.c_int),
                ("base_year0", ctypes.c_int), ("base_year1", ctypes.c_int), ("reserved", ctypes.c_int),
                ("threshold", ctypes.c_double)]


class Metric:
    """One number per member from a window of a recorded output (hx_metric in include/hector_amd.h).
    op: "mean", "min", "max", "year_of_min", "year_of_max", "first_ge", "count_ge" or "slope";
    years = (year0, year1) or one year; baseline = (year0, year1): the member's own mean over those
    years is subtracted first; threshold: for "first_ge" and "count_ge"."""

    def __init__(self, op, years, baseline=None, threshold=float("nan")):
        if op not in METRIC_OPS:
            raise HectorAmdError("Metric: unknown op %r (one of %s)" % (op, ", ".join(METRIC_OPS)))
        y = np.atleast_1d(np.asarray(years)).astype(np.int64)
        if y.size < 1:
            raise HectorAmdError("Metric: years must be a year or (year0, year1)")
        self.op = op
        self.years = (int(y.min()), int(y.max()))
        self.baseline = None if baseline is None else (int(baseline[0]), int(baseline[1]))
        self.threshold = float(threshold)

    def __repr__(self):
        return "Metric(%r, %r, baseline=%r, threshold=%r)" % (self.op, self.years, self.baseline, self.threshold)

    def _c(self):
        b0, b1 = (1, 0) if self.baseline is None else self.baseline
        return _HxMetric(METRIC_OPS[self.op], self.years[0], self.years[1], b0, b1, 0, self.threshold)


class _HxPairMetric(ctypes.Structure):   # hx_pair_metric
    _fields_ = [("op", ctypes.c_int), ("year0", ctypes.c_int), ("year1", ctypes.c_int),
                ("base_a0", ctypes.c_int), ("base_a1", ctypes.c_int), ("base_b0", ctypes.c_int),
                ("base_b1", ctypes.c_int), ("reserved", ctypes.c_int), ("threshold", ctypes.c_double)]


PAIR_METRIC_OPS = {"slope": 0, "intercept": 1, "r2": 2, "at_first_ge": 3, "at_max": 4, "at_min": 5,
                   "mean_where_ge": 6, "end_ratio": 7}   # HX_PMET_*


class PairMetric:
    """One number per member from a window of TWO series of that member, a (reported / dependent) and
    b (condition / independent) (hx_pair_metric in include/hector_amd.h).
    op: "slope", "intercept", "r2" (the regression of a on b), "at_first_ge" (a in the first year with
    b >= threshold), "at_max", "at_min" (a in the first year that holds the largest / smallest b),
    "mean_where_ge" (the mean of a over the years with b >= threshold) or "end_ratio"
    ((a_year1 - a_year0) / (b_year1 - b_year0));
    years = (year0, year1) or one year; baseline / baseline_b = (year0, year1): the member's own mean
    of a / of b over those years is subtracted first; threshold: for the two "_ge" operations."""

    def __init__(self, op, years, baseline=None, baseline_b=None, threshold=float("nan")):
        if op not in PAIR_METRIC_OPS:
            raise HectorAmdError("PairMetric: unknown op %r (one of %s)" % (op, ", ".join(PAIR_METRIC_OPS)))
        y = np.atleast_1d(np.asarray(years)).astype(np.int64)
        if y.size < 1:
            raise HectorAmdError("PairMetric: years must be a year or (year0, year1)")
        self.op = op
        self.years = (int(y.min()), int(y.max()))
        for name, b in (("baseline", baseline), ("baseline_b", baseline_b)):
            if b is not None and (len(b) != 2 or int(b[1]) < int(b[0])):
                raise HectorAmdError("PairMetric: %s must be (year0, year1) with year0 <= year1" % name)
        self.baseline = None if baseline is None else (int(baseline[0]), int(baseline[1]))
        self.baseline_b = None if baseline_b is None else (int(baseline_b[0]), int(baseline_b[1]))
        self.threshold = float(threshold)

    def __repr__(self):
        return "PairMetric(%r, %r, baseline=%r, baseline_b=%r, threshold=%r)" % (
            self.op, self.years, self.baseline, self.baseline_b, self.threshold)

    def _c(self):
        a0, a1 = (1, 0) if self.baseline is None else self.baseline
        b0, b1 = (1, 0) if self.baseline_b is None else self.baseline_b
        return _HxPairMetric(PAIR_METRIC_OPS[self.op], self.years[0], self.years[1], a0, a1, b0, b1, 0,
                             self.threshold)


MOMENTS_MAX_AGAINST = 8   # HX_MOM_MAX_PRED


class Moments:
    """What hx_ensemble_moments / hx_metric_moments return, and the statistics they define
    (include/hector_amd.h), all in float64.  R rows (years or metrics), K predictors.
    Raw: shift[R] = c_y, the smallest participating value of the row; sums[R, 2 + 3 K] = A, B, then
    C_k, D_k, E_k per predictor; wsum[R] = W (uint64); n_part[R]; names[K]; pshift[K] = c_k.
    Derived:  mean = shift + A/W;  var = B/W - (A/W)**2 (population);  pmean = pshift + C/W and
    pvar = D/W - (C/W)**2, [R, K];  cov = E/W - (A/W)(C/W);  corr = cov / sqrt(var * pvar);
    slope = cov / pvar.  corr is NaN where var or pvar is 0, slope where pvar is 0; a row nobody takes
    part in is NaN throughout.  wsum and sums scale with the quantisation of the weights (weights=None
    is q = 1, weights of all ones q = 2**32: wsum and sums exactly 2**32 times larger); only the
    derived statistics do not depend on the scale of the weights."""

    def __init__(self, shift, sums, wsum, n_part, names=(), pshift=None, q=None, predictors=None):
        self.shift = np.asarray(shift, dtype=np.float64)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(self.shift.size, -1)
        self.wsum = np.asarray(wsum, dtype=np.uint64)
        self.n_part = np.asarray(n_part, dtype=np.int64)
        self.names = list(names)
        k = len(self.names)
        if self.sums.shape[1] != 2 + 3 * k:
            raise HectorAmdError("Moments: sums must have 2 + 3 * len(names) columns")
        self.pshift = np.zeros(k) if pshift is None else np.asarray(pshift, dtype=np.float64)
        self._q = None if q is None else np.asarray(q, dtype=np.uint64)
        self._pred = None if predictors is None else np.asarray(predictors, dtype=np.float64).reshape(k, -1)

    def _over_w(self, cols):
        w = self.wsum.astype(np.float64)
        w = np.where(w > 0, w, np.nan)
        with np.errstate(invalid="ignore"):
            return cols / (w if cols.ndim == 1 else w[:, None])

    @property
    def mean(self):
        return self.shift + self._over_w(self.sums[:, 0])

    @property
    def var(self):
        a = self._over_w(self.sums[:, 0])
        return self._over_w(self.sums[:, 1]) - a * a

    @property
    def sd(self):
        with np.errstate(invalid="ignore"):
            return np.sqrt(self.var)

    @property
    def pmean(self):
        return self.pshift[None, :] + self._over_w(self.sums[:, 2::3])

    @property
    def pvar(self):
        c = self._over_w(self.sums[:, 2::3])
        return self._over_w(self.sums[:, 3::3]) - c * c

    @property
    def cov(self):
        return self._over_w(self.sums[:, 4::3]) - self._over_w(self.sums[:, 0])[:, None] * self._over_w(self.sums[:, 2::3])

    @property
    def corr(self):
        v = self.var[:, None] * self.pvar
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(v > 0, self.cov / np.sqrt(np.where(v > 0, v, 1.0)), np.nan)

    @property
    def slope(self):
        pv = self.pvar
        ok = (pv > 0) & (self.var[:, None] == self.var[:, None])
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ok, self.cov / np.where(pv > 0, pv, 1.0), np.nan)

    def src(self):
        """Standardised regression coefficients of all predictors jointly -> [R, K]: R_pp beta =
        corr per row, with R_pp the weighted correlation matrix of the predictors, computed here in
        numpy from the integer weights q and the predictor arrays over the members with q > 0 and
        all predictors finite.  A row whose n_part differs from the number of those members (some
        of them were NaN in that row) gets NaN: its participants are not those of R_pp."""
        k = len(self.names)
        out = np.full((self.shift.size, k), np.nan)
        if k == 0:
            return out
        if self._q is None or self._pred is None:
            raise HectorAmdError("Moments.src: needs the weights q and the predictor arrays")
        on = (self._q > 0) & np.isfinite(self._pred).all(axis=0)
        if not on.any():
            return out
        w = self._q[on].astype(np.float64)
        p = self._pred[:, on]
        z = p - (p * w).sum(axis=1, keepdims=True) / w.sum()
        cpp = (z * w) @ z.T / w.sum()
        sd = np.sqrt(np.diag(cpp))
        if not (sd > 0).all():
            return out
        rpp = cpp / np.outer(sd, sd)
        rows = (self.n_part == int(on.sum())) & ~np.isnan(self.corr).any(axis=1)
        if rows.any():
            try:
                out[rows] = np.linalg.solve(rpp, self.corr[rows].T).T
            except np.linalg.LinAlgError:
                pass
        return out

    def __repr__(self):
        return "Moments(rows=%d, against=%r)" % (self.shift.size, self.names)


GROUP_MAX = 16   # HX_GROUP_MAX


class GroupedMoments:
    """What hx_group_moments returns (include/hector_amd.h): the raw fields of Moments with a leading
    group axis -- shift[G, R], sums[G, R, 2 + 3 K], wsum[G, R] (uint64), n_part[G, R], pshift[G, K] --
    and the partition of the rows' variance over the groups.  gm[g] is the Moments of group g; it
    carries the group's pshift, integer weights (0 outside the group) and the predictors, so that
    gm[g].src() works.  Over the groups that take part in a row (W_g > 0), all in float64:
      weight_share[G, R] = W_g / sum_g W_g
      pooled_mean[R] = sum_g share_g mean_g
      between[R] = sum_g share_g (mean_g - pooled_mean)**2      (the variance of the group means)
      within[R]  = sum_g share_g var_g                          (the mean of the group variances)
      pooled_var[R] = between + within        (the law of total variance: the variance of the union)
      eta2[R] = between / (between + within)  (the correlation ratio: with labels = bins of a
                parameter, the given-data estimate of its first-order sensitivity index)
    A row nobody takes part in is NaN throughout; eta2 is NaN where the total variance is 0."""

    def __init__(self, shift, sums, wsum, n_part, names=(), pshift=None, q=None, predictors=None, labels=None):
        self.shift = np.asarray(shift, dtype=np.float64)
        if self.shift.ndim != 2:
            raise HectorAmdError("GroupedMoments: shift must be [groups, rows]")
        g, r = self.shift.shape
        self.names = list(names)
        k = len(self.names)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(g, r, -1)
        if self.sums.shape[2] != 2 + 3 * k:
            raise HectorAmdError("GroupedMoments: sums must have 2 + 3 * len(names) columns")
        self.wsum = np.asarray(wsum, dtype=np.uint64).reshape(g, r)
        self.n_part = np.asarray(n_part, dtype=np.int64).reshape(g, r)
        self.pshift = np.zeros((g, k)) if pshift is None else np.asarray(pshift, dtype=np.float64).reshape(g, k)
        self._q = None if q is None else np.asarray(q, dtype=np.uint64)
        self._pred = None if predictors is None else np.asarray(predictors, dtype=np.float64).reshape(k, -1)
        self._labels = None if labels is None else np.asarray(labels)

    @property
    def n_groups(self):
        return self.shift.shape[0]

    def __len__(self):
        return self.n_groups

    def __getitem__(self, g):
        g = int(g)
        if not 0 <= g < self.n_groups:
            raise IndexError("GroupedMoments: group %d of %d" % (g, self.n_groups))
        q = None
        if self._q is not None and self._labels is not None:
            q = np.where(self._labels == g, self._q, np.uint64(0)).astype(np.uint64)
        return Moments(self.shift[g], self.sums[g], self.wsum[g], self.n_part[g], self.names, self.pshift[g], q,
                       self._pred)

    def _group_stats(self):
        """-> share[G, R] (0 where a group takes no part, NaN where nobody does), c[R] = the smallest
        shift of the row, the group means LESS c and the group variances [G, R] with 0 in place of
        NaN.  Means relative to c: a row whose participants are all equal has every one exactly 0, so
        that its between-group variance is exactly 0 whatever the rounding of the shares."""
        w = self.wsum.astype(np.float64)
        on = w > 0
        tot = w.sum(axis=0)
        tot = np.where(tot > 0, tot, np.nan)
        wg = np.where(on, w, 1.0)
        a = self.sums[:, :, 0] / wg
        c = np.where(on, self.shift, np.inf).min(axis=0)
        c = np.where(np.isfinite(c), c, np.nan)
        with np.errstate(invalid="ignore"):
            dmean = np.where(on, (self.shift - c[None, :]) + a, 0.0)
        var = np.where(on, self.sums[:, :, 1] / wg - a * a, 0.0)
        return w / tot[None, :], c, dmean, var

    @property
    def weight_share(self):
        return self._group_stats()[0]

    @property
    def pooled_mean(self):
        share, c, dmean, _ = self._group_stats()
        return c + (share * dmean).sum(axis=0)

    @property
    def between(self):
        share, _, dmean, _ = self._group_stats()
        pm = (share * dmean).sum(axis=0)
        return (share * (dmean - pm[None, :]) ** 2).sum(axis=0)

    @property
    def within(self):
        share, _, _, var = self._group_stats()
        return (share * var).sum(axis=0)

    @property
    def pooled_var(self):
        return self.between + self.within

    @property
    def eta2(self):
        b, t = self.between, self.pooled_var
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(t > 0, b / np.where(t > 0, t, 1.0), np.nan)

    def __repr__(self):
        return "GroupedMoments(groups=%d, rows=%d, against=%r)" % (self.shift.shape + (self.names,))


SOBOL_MAX_FACTORS = 16   # HX_SOBOL_MAX_FACTORS


class Sobol:
    """What hx_ensemble_sobol / hx_metric_sobol return, and the statistics they define
    (include/hector_amd.h), all in float64.  R rows (years or metrics), K factors of a Saltelli
    design (hector_amd.ensemble.saltelli).
    Raw: names[K]; shift[R] = c_y, the smallest participating x_A or x_B of the row; sums[R, 4 + 4 K]
    = SA1, SA2, SB1, SB2, then T_i, TT_i, F_i, FF_i per factor; n_part[R] = participating groups n.
    Derived:  m = (SA1 + SB1) / (2 n), mean = shift + m;  var = V = (SA2 + SB2) / (2 n) - m m, the
    population variance of the 2 n pooled A and B values;  total = T / (2 n V) and first = 1 -
    F / (2 n V), [R, K] (Jansen's estimators);  total_se = sqrt((TT / n - (T / n)**2) / n) / (2 V) and
    first_se the same from F, FF: the standard errors of the numerators with V taken as known.
    Where V is 0 or nobody takes part, the indices and their standard errors are NaN."""

    def __init__(self, names, shift, sums, n_part):
        self.names = list(names)
        self.shift = np.asarray(shift, dtype=np.float64)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(self.shift.size, -1)
        self.n_part = np.asarray(n_part, dtype=np.int64)
        if self.sums.shape[1] != 4 + 4 * len(self.names):
            raise HectorAmdError("Sobol: sums must have 4 + 4 * len(names) columns")

    def _n(self):
        n = self.n_part.astype(np.float64)
        return np.where(n > 0, n, np.nan)

    def _m(self):
        return (self.sums[:, 0] + self.sums[:, 2]) / (2.0 * self._n())

    @property
    def mean(self):
        return self.shift + self._m()

    @property
    def var(self):
        m = self._m()
        return (self.sums[:, 1] + self.sums[:, 3]) / (2.0 * self._n()) - m * m

    def _v(self):
        v = self.var
        return np.where(v != 0, v, np.nan)[:, None]   # (V == 0: undefined)

    @property
    def total(self):
        return self.sums[:, 4::4] / (2.0 * self._n()[:, None] * self._v())

    @property
    def first(self):
        return 1.0 - self.sums[:, 6::4] / (2.0 * self._n()[:, None] * self._v())

    def _se(self, s1, s2):
        n = self._n()[:, None]
        with np.errstate(invalid="ignore"):
            return np.sqrt((s2 / n - (s1 / n) ** 2) / n) / (2.0 * self._v())

    @property
    def total_se(self):
        return self._se(self.sums[:, 4::4], self.sums[:, 5::4])

    @property
    def first_se(self):
        return self._se(self.sums[:, 6::4], self.sums[:, 7::4])

    def __repr__(self):
        return "Sobol(rows=%d, factors=%r)" % (self.shift.size, self.names)


class CoMoments:
    """What hx_ensemble_comoments returns, and the statistics it defines (include/hector_amd.h), all
    in float64.  Window A has na rows (years_a), window B nb rows (years_b); participation is by
    complete cases, so there is ONE wsum (W) and ONE n_part.
    Raw: shift_a[na], shift_b[nb] = the rows' smallest participating values; sums_a[na, 2],
    sums_b[nb, 2] = (sum q d, sum q d d); cross[na, nb] = sum (q d_a) d_b; symmetric: B is A.
    Derived: mean_a = shift_a + S_a/W, var_a = T_a/W - (S_a/W)**2 (population), mean_b / var_b
    likewise; cov = cross/W - (S_a/W)(S_b/W); corr = cov / sqrt(var_a var_b); slope = cov / var_b
    (the regression of A's year on B's year).  corr is NaN where var_a or var_b is 0, slope where
    var_b is 0; everything is NaN when nobody takes part."""

    def __init__(self, shift_a, sums_a, shift_b, sums_b, cross, wsum, n_part, years_a=None, years_b=None,
                 symmetric=False):
        self.shift_a = np.asarray(shift_a, dtype=np.float64).reshape(-1)
        self.shift_b = np.asarray(shift_b, dtype=np.float64).reshape(-1)
        na, nb = self.shift_a.size, self.shift_b.size
        self.sums_a = np.asarray(sums_a, dtype=np.float64).reshape(-1, 2)
        self.sums_b = np.asarray(sums_b, dtype=np.float64).reshape(-1, 2)
        self.cross = np.asarray(cross, dtype=np.float64)
        if self.sums_a.shape[0] != na or self.sums_b.shape[0] != nb or self.cross.shape != (na, nb):
            raise HectorAmdError("CoMoments: sums_a [na, 2], sums_b [nb, 2] and cross [na, nb] must match the shifts")
        self.wsum = int(wsum)
        self.n_part = int(n_part)
        self.years_a = np.arange(na) if years_a is None else np.asarray(years_a)
        self.years_b = np.arange(nb) if years_b is None else np.asarray(years_b)
        self.symmetric = bool(symmetric)

    def _over_w(self, x):
        return x / np.float64(self.wsum) if self.wsum > 0 else np.full(np.shape(x), np.nan)

    @property
    def mean_a(self):
        return self.shift_a + self._over_w(self.sums_a[:, 0])

    @property
    def mean_b(self):
        return self.shift_b + self._over_w(self.sums_b[:, 0])

    @property
    def var_a(self):
        s = self._over_w(self.sums_a[:, 0])
        return self._over_w(self.sums_a[:, 1]) - s * s

    @property
    def var_b(self):
        s = self._over_w(self.sums_b[:, 0])
        return self._over_w(self.sums_b[:, 1]) - s * s

    @property
    def cov(self):
        return self._over_w(self.cross) - np.outer(self._over_w(self.sums_a[:, 0]), self._over_w(self.sums_b[:, 0]))

    @property
    def corr(self):
        v = np.outer(self.var_a, self.var_b)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(v > 0, self.cov / np.sqrt(np.where(v > 0, v, 1.0)), np.nan)

    @property
    def slope(self):
        vb = np.broadcast_to(self.var_b[None, :], self.cross.shape)
        ok = (vb > 0) & (self.var_a[:, None] == self.var_a[:, None])
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ok, self.cov / np.where(vb > 0, vb, 1.0), np.nan)

    def pca(self, k):
        """The k leading principal components of a symmetric result (numpy.linalg.eigh of cov, on
        the host) -> (eigenvalues [k] descending, their share of the trace [k], patterns [k, na]).
        The sign of a pattern is fixed so that its largest-magnitude component is positive."""
        if not self.symmetric:
            raise HectorAmdError("CoMoments.pca: needs a symmetric result (comoments(var, dates) without var_b)")
        na = self.shift_a.size
        k = int(k)
        if k < 1 or k > na:
            raise HectorAmdError("CoMoments.pca: k must lie in 1..%d" % na)
        cov = self.cov
        if not np.isfinite(cov).all():
            raise HectorAmdError("CoMoments.pca: the covariance is not finite (nobody takes part)")
        val, vec = np.linalg.eigh(cov)
        order = np.argsort(val)[::-1][:k]
        val, pat = val[order], vec[:, order].T.copy()
        for p in pat:
            if p[np.argmax(np.abs(p))] < 0:
                p *= -1.0
        tr = np.trace(cov)
        return val, (val / tr if tr > 0 else np.full(k, np.nan)), pat

    def scores(self, core, var, k):
        """The k leading principal-component scores of every member, on the device: pattern .
        (trajectory - mean) -> ndarray [k, n_members]; core.project(var, years_a, pca(k)[2],
        center=mean_a).  var is the variable this result was taken of; a result that is not
        symmetric is refused as pca refuses it."""
        return core.project(var, self.years_a, self.pca(k)[2], center=self.mean_a)

    def __repr__(self):
        return "CoMoments(na=%d, nb=%d, symmetric=%r, n_part=%d)" % (self.shift_a.size, self.shift_b.size,
                                                                     self.symmetric, self.n_part)


# The hx_* function of include/hector_amd.h that serves (verb, kind of rows, grouped).  A grouped call
# has one function per verb, for a window of years and for metrics; pair rows have no grouped form.
_SUMMARY_FN = {
    ("quantiles", "window", False): "hx_ensemble_quantiles",
    ("quantiles", "metric", False): "hx_metric_quantiles",
    ("quantiles", "pair", False): "hx_pair_metric_quantiles",
    ("quantiles", "window", True): "hx_group_quantiles",
    ("quantiles", "metric", True): "hx_group_quantiles",
    ("probabilities", "window", False): "hx_ensemble_probabilities",
    ("probabilities", "metric", False): "hx_metric_probabilities",
    ("probabilities", "pair", False): "hx_pair_metric_probabilities",
    ("probabilities", "window", True): "hx_group_probabilities",
    ("probabilities", "metric", True): "hx_group_probabilities",
    ("moments", "window", False): "hx_ensemble_moments",
    ("moments", "metric", False): "hx_metric_moments",
    ("moments", "pair", False): "hx_pair_metric_moments",
    ("moments", "window", True): "hx_group_moments",
    ("moments", "metric", True): "hx_group_moments",
    ("sobol", "window", False): "hx_ensemble_sobol",
    ("sobol", "metric", False): "hx_metric_sobol",
    ("members", "metric", False): "hx_member_metrics",
    ("members", "pair", False): "hx_member_pair_metrics",
    ("ranks", "metric", False): "hx_metric_ranks",
}

_PTR_OF = {np.dtype(t).num: ctypes.POINTER(c) for t, c in (   # the C pointer an array goes as, by dtype.num
    (np.float64, ctypes.c_double), (np.int64, ctypes.c_longlong), (np.uint64, ctypes.c_ulonglong),
    (np.int32, ctypes.c_int), (np.uint8, ctypes.c_ubyte))}


class _Rows:
    """The rows a summary verb runs over -- the RowSource of csrc/ensemble_core.hpp on this side: a
    window of years, metrics or pair metrics.  what: the public verb, the prefix of every message;
    nrows; lead / group_lead: the arguments of the ungrouped / grouped ABI function between the
    handle and the labels or the verb's own arguments; keep: what they point into (alive as long as
    the rows are, and the verb holds the rows until its call has returned)."""
    __slots__ = ("core", "what", "kind", "nrows", "lead", "group_lead", "keep")

    def __init__(self, core, what, kind, nrows, lead, group_lead=None, keep=None):
        self.core, self.what, self.kind, self.nrows = core, what, kind, nrows
        self.lead, self.group_lead, self.keep = lead, group_lead, keep

    @classmethod
    def window(cls, core, what, var, dates):
        y0, y1, ny = core._window(dates)
        cap = var.encode()
        return cls(core, what, "window", ny, (cap, y0, y1), (cap, y0, y1, None, 0))

    @staticmethod
    def _specs(specs, of, ctype, what):
        if isinstance(specs, of):
            specs = [specs]
        specs = list(specs)
        if not all(isinstance(m, of) for m in specs):
            raise HectorAmdError("%s: specs must be hector_amd.%s objects" % (what, of.__name__))
        return (ctype * max(len(specs), 1))(*[m._c() for m in specs]), len(specs)

    @classmethod
    def metrics(cls, core, what, var, specs):
        arr, ns = cls._specs(specs, Metric, _HxMetric, what)
        sp = ctypes.byref(arr)
        return cls(core, what, "metric", ns, (var.encode(), sp, ns), (var.encode(), 0, 0, sp, ns), arr)

    @classmethod
    def pair_metrics(cls, core, what, var_a, b, specs):
        """b: a variable name, or (years, values) -- a per-year vector, the same for every member."""
        arr, ns = cls._specs(specs, PairMetric, _HxPairMetric, what)
        if isinstance(b, str):
            side, v = (b.encode(), None, 0, 0), None
        else:
            try:
                years, values = b
            except (TypeError, ValueError):
                raise HectorAmdError("%s: b is a variable name or a (years, values) pair" % what)
            yr = np.atleast_1d(np.asarray(years)).astype(np.int64)
            v = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=np.float64)))
            if yr.ndim != 1 or yr.size < 1 or v.shape != yr.shape:
                raise HectorAmdError("%s: the vector b needs one value per year" % what)
            if yr.size > 1 and not (np.diff(yr) == 1).all():
                raise HectorAmdError("%s: the years of the vector b must be consecutive and ascending" % what)
            side = (None, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(yr[0]), int(yr[-1]))
        return cls(core, what, "pair", ns, (var_a.encode(),) + side + (ctypes.byref(arr), ns), keep=(arr, v))

    def shape(self, grp, *tail):
        """The shape of an output with `tail` entries per row: a grouped call has a leading group axis."""
        return (() if grp is None else (grp[1],)) + (self.nrows,) + tail

    def call(self, verb, grp, *args):
        """The one call of a verb: the function of _SUMMARY_FN over these rows, grp = None or what
        Core._groups returned, then the verb's own arguments (an array goes as a pointer to its
        elements, None as NULL)."""
        core = self.core
        lead = self.lead
        if grp is not None:
            lead = self.group_lead + (grp[0].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), grp[1])
        args = [a.ctypes.data_as(_PTR_OF[a.dtype.num]) if isinstance(a, np.ndarray) else a for a in args]
        core._ck(getattr(core._lib, _SUMMARY_FN[verb, self.kind, grp is not None])(core._h, *lead, *args))


class Core:
    """An N-member ensemble core bound to one GPU (device=) or sharded over a list of GPUs
    (devices=[...]: contiguous member blocks, hx_newcore_devices)."""

    def __init__(self, scenario=None, n_members=1, device=0, lib_path=None,
                 allow_emulation=False, name=None, devices=None):
        self._lib = _lib.load(lib_path, allow_emulation)
        self._h = ctypes.c_void_p()
        if devices is None:
            self._ck(self._lib.hx_newcore((scenario or DEFAULT_SCENARIO).encode(), int(n_members),
                                          int(device), ctypes.byref(self._h)))
        else:
            devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            self._ck(self._lib.hx_newcore_devices((scenario or DEFAULT_SCENARIO).encode(),
                                                  int(n_members), devs, len(devices),
                                                  ctypes.byref(self._h)))
        self.n_members = int(n_members)
        if name is None:   # newcore(..., name =): default here the INI's run_name
            rn = ctypes.c_char_p()
            self._ck(self._lib.hx_run_name(self._h, ctypes.byref(rn)))
            name = rn.value.decode() if rn.value else "Unnamed Hector core"
        self.name = name
        s, e, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._ck(self._lib.hx_dates(self._h, ctypes.byref(s), ctypes.byref(e), ctypes.byref(c)))
        self.strtdate, self.enddate = s.value, e.value

    def _ck(self, rc):
        if rc != 0:
            raise HectorAmdError(self._lib.hx_last_error().decode())

    @property
    def backend(self):
        return self._lib.hx_backend().decode()

    @property
    def current_date(self):
        c = ctypes.c_int()
        self._ck(self._lib.hx_dates(self._h, None, None, ctypes.byref(c)))
        return c.value

    def setvar(self, var, values, unit=None):
        v = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=np.float64)))
        self._ck(self._lib.hx_setvar(self._h, var.encode(),
                                     v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), v.size,
                                     unit.encode() if unit else None))
        return self

    def getvar(self, var):
        out = np.empty(self.n_members)
        self._ck(self._lib.hx_getvar(self._h, var.encode(),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def create_biome(self, biome):
        self._ck(self._lib.hx_create_biome(self._h, biome.encode()))
        return self

    def delete_biome(self, biome):
        self._ck(self._lib.hx_delete_biome(self._h, biome.encode()))
        return self

    def rename_biome(self, oldname, newname):
        self._ck(self._lib.hx_rename_biome(self._h, oldname.encode(), newname.encode()))
        return self

    def split_biome(self, names, fveg_c=None, fdetritus_c=None, fsoil_c=None,
                    fpermafrost_c=None, fnpp_flux0=None, old_biome=None):
        n = len(names)
        arr = (ctypes.c_char_p * n)(*[s.encode() for s in names])

        def f(x):
            if x is None:
                return None
            a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
            assert a.size == n
            keep.append(a)
            return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        keep = []
        if old_biome is None:
            self._ck(self._lib.hx_split_biome(self._h, n, arr, f(fveg_c), f(fdetritus_c),
                                              f(fsoil_c), f(fpermafrost_c), f(fnpp_flux0)))
        else:
            self._ck(self._lib.hx_split_biome_of(self._h, old_biome.encode(), n, arr, f(fveg_c),
                                                 f(fdetritus_c), f(fsoil_c), f(fpermafrost_c),
                                                 f(fnpp_flux0)))
        return self

    def set_outputs(self, variables):
        n = len(variables)
        arr = (ctypes.c_char_p * n)(*[s.encode() for s in variables])
        self._ck(self._lib.hx_set_outputs(self._h, n, arr))
        return self

    def tracking_pools(self):
        names = ctypes.POINTER(ctypes.c_char_p)()
        n = ctypes.c_int()
        self._ck(self._lib.hx_tracking_pools(self._h, ctypes.byref(names), ctypes.byref(n)))
        return [names[i].decode() for i in range(n.value)]

    def tracking_data(self, member, dates, masks=False):
        """-> (values[ny, TP], fractions[ny, TP, TP]) for dates = (year0, year1); with masks=True
        also in_map[ny, TP, TP] (bool: the source is in the pool's map)."""
        y0, y1 = int(min(dates)), int(max(dates))
        tp = len(self.tracking_pools())
        v = np.zeros((y1 - y0 + 1, tp)); f = np.zeros((y1 - y0 + 1, tp, tp))
        dp = ctypes.POINTER(ctypes.c_double)
        w = (tp + 63) // 64   # mask words per pool (2 from 12 biomes on)
        mk = np.zeros((y1 - y0 + 1, tp, w), dtype=np.uint64)
        self._ck(self._lib.hx_tracking_data(self._h, int(member), y0, y1, v.ctypes.data_as(dp),
                                            f.ctypes.data_as(dp),
                                            mk.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))))
        if masks:
            src = np.arange(tp)
            bits = (mk[:, :, src // 64] >> (src % 64).astype(np.uint64)[None, None, :]) & np.uint64(1)
            return v, f, bits.astype(bool)
        return v, f

    def getunits(self, var):
        """getunits(var)  R/units.R"""
        u = ctypes.c_char_p()
        self._ck(self._lib.hx_var_info(self._h, var.encode(), None, ctypes.byref(u)))
        return u.value.decode()

    def component_of(self, var):
        comp = ctypes.c_char_p()
        self._ck(self._lib.hx_var_info(self._h, var.encode(), ctypes.byref(comp), None))
        return comp.value.decode()

    def biomes(self):
        """get_biome_list(core)  R/biome.R:8-16"""
        names = ctypes.POINTER(ctypes.c_char_p)()
        n = ctypes.c_int()
        self._ck(self._lib.hx_biomes(self._h, ctypes.byref(names), ctypes.byref(n)))
        return [names[i].decode() for i in range(n.value)]

    def halocarbons(self):
        names = ctypes.POINTER(ctypes.c_char_p)()
        n = ctypes.c_int()
        self._ck(self._lib.hx_halocarbons(self._h, ctypes.byref(names), ctypes.byref(n)))
        return [names[i].decode() for i in range(n.value)]

    def enable_spinup_record(self, on=True):
        """Keep what the reference's output stream sees after every spinup step (its spinup = 1
        rows, csv_outputstream_visitor.cpp:86-95): the carbon-cycle variables."""
        self._ck(self._lib.hx_enable_spinup_record(self._h, 1 if on else 0))
        return self

    def spinup_record(self, member=0):
        """-> dict capability -> values[steps] (steps 1 .. spinup_steps(member))"""
        names = ctypes.POINTER(ctypes.c_char_p)()
        nv = ctypes.c_int()
        self._ck(self._lib.hx_spinup_record(self._h, int(member), ctypes.byref(names), ctypes.byref(nv),
                                            None, 0, None))
        mx = self.spinup_steps(member)
        vals = np.zeros((max(mx, 1), nv.value))
        steps = ctypes.c_int()
        self._ck(self._lib.hx_spinup_record(self._h, int(member), None, None,
                                            vals.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), max(mx, 1),
                                            ctypes.byref(steps)))
        return {names[i].decode(): vals[:steps.value, i].copy() for i in range(nv.value)}

    def enable_history(self, on=True):
        self._ck(self._lib.hx_enable_history(self._h, 1 if on else 0))
        return self

    def enable_slcf_mixes(self, on=True):
        """Let setvar_dated_mix, clear_mix, mix_capabilities and setvar_scenarios take the aerosol and
        ozone / OH precursor emissions too (hx_enable_slcf_mixes): SO2, BC, OC, NH3, NOX, CO and
        NMVOC -- what the shipped SSPs differ in besides the names that are always mixable.  Off by
        default; costs nothing until such a mix is set (then 8 B per member-year and row: one row
        for the aerosols, six for the precursors); switching it off under such a mix is refused."""
        self._ck(self._lib.hx_enable_slcf_mixes(self._h, 1 if on else 0))
        return self

    def enable_member_forcing(self, on=True):
        """Let setvar take one value per member for the forcing efficacies delta_co2, delta_ch4,
        delta_n2o, rho_bc, rho_oc, rho_so2 and rho_nh3 (hx_enable_member_forcing).  Off by default;
        a per-member rho_* costs 8 B per member-year (one aerosol row, however many of the four
        differ), the three delta_* 24 B per member.  Switching it off while one of the seven differs
        between members is refused."""
        self._ck(self._lib.hx_enable_member_forcing(self._h, 1 if on else 0))
        return self

    def setvar_dated(self, var, years, values, unit=None):
        y = np.ascontiguousarray(np.atleast_1d(np.asarray(years, dtype=np.int32)))
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64), y.shape))
        self._ck(self._lib.hx_setvar_dated(self._h, var.encode(),
                                           y.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                           v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), y.size,
                                           unit.encode() if unit else None))
        return self

    def setvar_dated_members(self, var, years, values, unit=None):
        """values[year, member]: a different input series for every member."""
        y = np.ascontiguousarray(np.atleast_1d(np.asarray(years, dtype=np.int32)))
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        if v.shape != (y.size, self.n_members):
            raise HectorAmdError("setvar_dated_members: values must be [n_years, n_members]")
        self._ck(self._lib.hx_setvar_dated_members(
            self._h, var.encode(), y.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), y.size,
            unit.encode() if unit else None))
        return self

    def setvar_dated_mix(self, var, years, basis, coeff, unit=None):
        """A different input series for every member as a mix of K shared year-vectors
        (hx_setvar_dated_mix): basis[K, n_years], coeff[K, n_members], or both 1-D for K = 1.  In
        `years` member m holds coeff[0, m] * basis[0, i] + coeff[1, m] * basis[1, i] + ... (each
        product rounded, added in ascending k); the table is built on the device, and a new coeff
        for the same years and basis costs K * n_members doubles of upload."""
        y = np.ascontiguousarray(np.atleast_1d(np.asarray(years, dtype=np.int32)))
        b = np.ascontiguousarray(np.atleast_2d(np.asarray(basis, dtype=np.float64)))
        w = np.ascontiguousarray(np.atleast_2d(np.asarray(coeff, dtype=np.float64)))
        if y.ndim != 1 or b.ndim != 2 or b.shape[1] != y.size:
            raise HectorAmdError("setvar_dated_mix: basis must be [K, n_years]")
        if w.ndim != 2 or w.shape != (b.shape[0], self.n_members):
            raise HectorAmdError("setvar_dated_mix: coeff must be [K, n_members] with the K of basis")
        if b.shape[0] < 1:
            raise HectorAmdError("setvar_dated_mix: K = 0 (clear_mix removes a mix)")
        self._ck(self._lib.hx_setvar_dated_mix(
            self._h, var.encode(), y.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), y.size,
            b.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), b.shape[0],
            w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), unit.encode() if unit else None))
        return self

    def clear_mix(self, var):
        """Remove the mix of `var`: the per-member table beneath it, or the shared series, again."""
        self._ck(self._lib.hx_setvar_dated_mix(self._h, var.encode(), None, 0, None, 0, None, None))
        return self

    def mix_capabilities(self):
        """The names setvar_dated_mix accepts for this core (hx_mix_capabilities): the carbon-cycle
        and CH4 emissions, N2O_emissions, RF_albedo and the scenario's <gas>_emissions."""
        names = ctypes.POINTER(ctypes.c_char_p)()
        n = ctypes.c_int()
        self._ck(self._lib.hx_mix_capabilities(self._h, ctypes.byref(names), ctypes.byref(n)))
        return [names[i].decode() for i in range(n.value)]

    def setvar_scenarios(self, paths, coeff):
        """Whole scenarios in one core (hx_setvar_scenario_mix): every dated input series in which
        one of the scenario files `paths` differs from this core's becomes a mix over
        startDate..endDate with the scenarios' series as basis.  coeff[n_scenarios, n_members], or
        one integer label 0 .. n_scenarios-1 per member (one-hot coefficients: the member's inputs
        are then its scenario's own bits).  Returns the number of series mixed; a refused call
        (different dates, halocarbons, scalars, an unmixable series) changes nothing."""
        paths = [os.fspath(p) for p in paths]
        w = np.asarray(coeff)
        if w.ndim == 1 and w.shape == (self.n_members,) and np.issubdtype(w.dtype, np.integer):
            if w.size and (w.min() < 0 or w.max() >= len(paths)):
                raise HectorAmdError("setvar_scenarios: a label outside 0..n_scenarios-1")
            w = (w[None, :] == np.arange(len(paths))[:, None]).astype(np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (len(paths), self.n_members):
            raise HectorAmdError("setvar_scenarios: coeff must be [n_scenarios, n_members] or one "
                                 "integer label per member")
        arr = (ctypes.c_char_p * len(paths))(*[p.encode() for p in paths])
        n = ctypes.c_int()
        self._ck(self._lib.hx_setvar_scenario_mix(self._h, arr, len(paths),
                                                  w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  ctypes.byref(n)))
        return n.value

    def set_member_sorting(self, on=True):
        self._ck(self._lib.hx_set_member_sorting(self._h, 1 if on else 0))
        return self

    def set_lane_calibration(self, on=True):
        """Lane order by measured cost after the first complete run (hx_set_lane_calibration)."""
        self._ck(self._lib.hx_set_lane_calibration(self._h, 1 if on else 0))
        return self

    def lane_order_source(self):
        """What the lanes are ordered by: "parameter key", "measured cost" (a complete run of this
        core) or "cost model" (fitted to an earlier core's measurements: hx_lane_order_source)."""
        v = ctypes.c_int(0)
        self._ck(self._lib.hx_lane_order_source(self._h, ctypes.byref(v)))
        return ("parameter key", "measured cost", "cost model")[v.value]

    def set_cost_model(self, on=True):
        self._ck(self._lib.hx_set_cost_model(self._h, 1 if on else 0))
        return self

    def lanes_calibrated(self):
        v = ctypes.c_int()
        self._ck(self._lib.hx_lanes_calibrated(self._h, ctypes.byref(v)))
        return bool(v.value)

    def lane_of_member(self):
        out = np.zeros(self.n_members, dtype=np.int32)
        self._ck(self._lib.hx_lane_of_member(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def reset(self, date=0):
        self._ck(self._lib.hx_reset(self._h, float(date)))
        return self

    def run(self, runtodate=-1, wait=True):
        self._ck(self._lib.hx_run(self._h, float(runtodate)))
        # the Rcpp wrapper's check (src/rcpp_hector.cpp:168-175), after the pending auto-reset
        # like there; Core::run itself -- hx_run -- does nothing for such a date (core.cpp:454-458)
        if runtodate > 0 and runtodate < self.current_date:
            raise HectorAmdError("Requested run date %g is prior to the current date of %d. "
                                 "Run reset() to reset to an earlier date."
                                 % (runtodate, self.current_date))
        if wait:
            self._ck(self._lib.hx_sync(self._h))
        return self

    def sync(self):
        self._ck(self._lib.hx_sync(self._h))

    def stream(self):
        """The core's hipStream_t as an integer (for torch.cuda.ExternalStream): every launch of
        this core -- run, statistics, gathers -- is queued on it, not on torch's current stream."""
        p = ctypes.c_void_p()
        self._ck(self._lib.hx_stream(self._h, ctypes.byref(p)))
        return p.value or 0

    def fetchvars(self, var, dates=None, out=None):
        """-> ndarray [n_years, n_members] for dates = (year0, year1) inclusive.  `out`: a
        C-contiguous float64 array of that shape to reuse (a buffer the host has already touched
        takes the device-to-host copy ~3x faster than a fresh allocation)."""
        y0, y1, _ = self._window(dates)
        shape = (y1 - y0 + 1, self.n_members)
        if out is None:
            out = np.empty(shape)
        elif out.shape != shape or out.dtype != np.float64 or not out.flags["C_CONTIGUOUS"]:
            raise HectorAmdError("fetchvars: out must be a C-contiguous float64 array of shape %r" % (shape,))
        self._ck(self._lib.hx_fetchvars(self._h, var.encode(), y0, y1,
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def device_var(self, var):
        p, npad = ctypes.c_void_p(), ctypes.c_int()
        self._ck(self._lib.hx_device_var(self._h, var.encode(), ctypes.byref(p), ctypes.byref(npad)))
        return p.value, npad.value

    def shards(self):
        """-> (devices[n_shards], offsets[n_shards + 1]): shard s holds members
        offsets[s] .. offsets[s + 1] - 1 on GPU devices[s]."""
        n = ctypes.c_int()
        self._ck(self._lib.hx_shards(self._h, ctypes.byref(n), None, None))
        dev = (ctypes.c_int * n.value)()
        off = (ctypes.c_int * (n.value + 1))()
        self._ck(self._lib.hx_shards(self._h, None, dev, off))
        return list(dev), list(off)

    def device_var_shard(self, shard, var):
        p, npad = ctypes.c_void_p(), ctypes.c_int()
        self._ck(self._lib.hx_device_var_shard(self._h, int(shard), var.encode(), ctypes.byref(p),
                                               ctypes.byref(npad)))
        return p.value, npad.value

    def comm_init_rank(self, n_procs, proc_rank, unique_id):
        """Join an RCCL communicator of n_procs x n_shards ranks (hx_comm_init_rank);
        unique_id: the 128 bytes of comm_unique_id() of ONE process."""
        if len(unique_id) != 128:
            raise HectorAmdError("comm_init_rank: the unique id is 128 bytes")
        self._ck(self._lib.hx_comm_init_rank(self._h, int(n_procs), int(proc_rank), bytes(unique_id)))
        return self

    def comm_info(self):
        """-> (world, first_rank, backend); world 0 = no communicator."""
        w, r, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_char_p()
        self._ck(self._lib.hx_comm_info(self._h, ctypes.byref(w), ctypes.byref(r), ctypes.byref(b)))
        return w.value, r.value, (b.value or b"").decode()

    def ensemble_stats(self, variables, dates=None, d_out=None, host=True):
        """Per-year {count, sum, sumsq, min, max} of `variables` over every member on every GPU
        and every process of the communicator (hx_ensemble_stats: local reductions + ONE RCCL
        all-gather): -> ndarray [n_vars, n_years, 5] (host=True) and / or into the device buffer
        d_out (an integer address on the first shard's GPU)."""
        if isinstance(variables, str):
            variables = [variables]
        y0, y1, _ = self._window(dates)
        arr = (ctypes.c_char_p * len(variables))(*[v.encode() for v in variables])
        out = np.empty((len(variables), y1 - y0 + 1, 5)) if host else None
        self._ck(self._lib.hx_ensemble_stats(
            self._h, len(variables), arr, y0, y1,
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if host else None,
            ctypes.c_void_p(d_out) if d_out else None))
        return out

    def stats_device(self, var, year0, year1, d_ptr):
        self._ck(self._lib.hx_stats_device(self._h, var.encode(), int(year0), int(year1),
                                           ctypes.c_void_p(d_ptr)))

    def score(self, var, years, obs, sigma=None, baseline=None, return_used=False, *, cov=None, ar1=None,
              whiten=None):
        """chi2 of every member against an observed record, on the device (hx_member_score):
        sum over i of (((x(years[i]) - base) - obs[i]) / sigma[i])**2 -> ndarray [n_members].
        obs NaN: that year is skipped; sigma None: no division; baseline = (year0, year1): base is
        the member's own mean of x over those years, None: nothing is subtracted.  The evaluation
        order is fixed (include/hector_amd.h): numpy reproduces the result bit for bit.

        Correlated observation errors (hx_member_score_whitened: chi2 = r^T C^-1 r = |W r|^2, at
        most 256 years), by ONE of
          cov=C        the n x n error covariance (not with sigma);
          ar1=rho      with sigma (scalar or per year): C_ij = sigma_i sigma_j rho^|years_i - years_j|,
                       0 <= rho < 1;
          whiten=W     a ready lower-triangular W = L^-1 of C = L L^T (hector_amd.whiten(C)[0]): what
                       a calibration loop factorises once.
        With cov and ar1 the years whose obs is NaN are dropped BEFORE the factorisation (their rows
        and columns of C deleted: the Gaussian's marginal) and n_used is what remains; with whiten a
        NaN observation is an error."""
        if cov is not None or ar1 is not None or whiten is not None:
            return self._score_whitened(var, years, obs, sigma, baseline, return_used, cov, ar1, whiten)
        dp = ctypes.POINTER(ctypes.c_double)
        yr = np.ascontiguousarray(np.atleast_1d(np.asarray(years)).astype(np.int32))
        ob = np.ascontiguousarray(np.atleast_1d(np.asarray(obs, dtype=np.float64)))
        if ob.shape != yr.shape or yr.ndim != 1:
            raise HectorAmdError("score: years and obs must be one-dimensional and of equal length")
        sg = None
        if sigma is not None:
            sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), yr.shape))
        b0, b1 = (1, 0) if baseline is None else (int(baseline[0]), int(baseline[1]))
        out = np.empty(self.n_members)
        used = ctypes.c_int()
        self._ck(self._lib.hx_member_score(
            self._h, var.encode(), yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ob.ctypes.data_as(dp),
            sg.ctypes.data_as(dp) if sg is not None else None, int(yr.size), b0, b1,
            out.ctypes.data_as(dp), ctypes.byref(used)))
        return (out, used.value) if return_used else out

    def _score_whitened(self, var, years, obs, sigma, baseline, return_used, cov, ar1, whiten):
        """score() with cov=, ar1= or whiten=: builds W and calls hx_member_score_whitened."""
        dp = ctypes.POINTER(ctypes.c_double)
        if sum(a is not None for a in (cov, ar1, whiten)) != 1:
            raise HectorAmdError("score: cov, ar1 and whiten are mutually exclusive")
        yr = np.ascontiguousarray(np.atleast_1d(np.asarray(years)).astype(np.int32))
        ob = np.ascontiguousarray(np.atleast_1d(np.asarray(obs, dtype=np.float64)))
        if ob.shape != yr.shape or yr.ndim != 1:
            raise HectorAmdError("score: years and obs must be one-dimensional and of equal length")
        n = int(yr.size)
        if ar1 is None and sigma is not None:
            raise HectorAmdError("score: sigma goes with ar1 only; cov and whiten carry the variances themselves")
        if whiten is not None:
            W = np.asarray(whiten, dtype=np.float64)
            if W.shape != (n, n):
                raise HectorAmdError("score: whiten must be n x n for n years")
            if np.isnan(ob).any():
                raise HectorAmdError("score: a NaN observation cannot be skipped under whiten (drop the year "
                                     "and factorise the remaining covariance: cov= and ar1= do that)")
        else:
            if ar1 is not None:
                if sigma is None:
                    raise HectorAmdError("score: ar1 needs sigma")
                rho = float(ar1)
                if not 0.0 <= rho < 1.0:
                    raise HectorAmdError("score: ar1 must lie in [0, 1)")
                sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), yr.shape)
                lag = np.abs(yr[:, None].astype(np.int64) - yr[None, :].astype(np.int64))
                C = sg[:, None] * sg[None, :] * rho ** lag
            else:
                C = np.asarray(cov, dtype=np.float64)
                if C.shape != (n, n):
                    raise HectorAmdError("score: cov must be n x n for n years")
            keep = ~np.isnan(ob)
            if not keep.all():
                yr, ob, C = np.ascontiguousarray(yr[keep]), np.ascontiguousarray(ob[keep]), C[np.ix_(keep, keep)]
                n = int(yr.size)
            if n < 1:
                raise HectorAmdError("score: no observation is left")
            if n <= _SCORE_WHITENED_MAX:   # (more: refused below, before a factorisation of that size)
                W = _whiten(C, "score")[0]
        if n > _SCORE_WHITENED_MAX:
            raise HectorAmdError("score: more than %d years (hx_member_score_whitened takes 1..%d)"
                                 % (_SCORE_WHITENED_MAX, _SCORE_WHITENED_MAX))
        W = np.ascontiguousarray(W)
        b0, b1 = (1, 0) if baseline is None else (int(baseline[0]), int(baseline[1]))
        out = np.empty(self.n_members)
        self._ck(self._lib.hx_member_score_whitened(
            self._h, var.encode(), yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ob.ctypes.data_as(dp),
            W.ctypes.data_as(dp), n, b0, b1, out.ctypes.data_as(dp)))
        return (out, n) if return_used else out

    def project(self, var, years, basis, center=None, baseline=None):
        """A matrix applied to every member's series, on the device (hx_member_project):
          r_k = (x(years[k], member) - base(member)) - center[k]
          out[j, member] = sum over k of basis[j, k] * r_k
        -> ndarray [m, n_members] for basis [m, n]; a one-dimensional basis of n entries -> [n_members].
        years in any order, repeats allowed (basis refers to the order given), 1 <= n <= 1024 and
        1 <= m <= 64; center None: zeros; baseline = (year0, year1): base is the member's own mean
        of x over those years, None: nothing is subtracted.  basis and center must be finite; a
        member with a NaN in a year read or in the reference period is NaN in all m outputs.
        The order of the sum is not part of the definition (fp64 matrix pipe): with s_j = sum_k
        |basis[j, k] r_k| every output lies within (n + 2) 2^-53 s_j of the exact sum.  An output is
        bit-identical from call to call and independent of lane order, shards, the other members
        and the other rows of basis."""
        dp = ctypes.POINTER(ctypes.c_double)
        yr = np.ascontiguousarray(np.atleast_1d(np.asarray(years)).astype(np.int32))
        if yr.ndim != 1 or yr.size < 1:
            raise HectorAmdError("project: years must be one-dimensional and not empty")
        n = int(yr.size)
        B = np.asarray(basis, dtype=np.float64)
        one = B.ndim == 1
        if one:
            B = B[None, :]
        if B.ndim != 2 or B.shape[1] != n or B.shape[0] < 1:
            raise HectorAmdError("project: basis must be [m, n] (or [n]) for n years")
        m = int(B.shape[0])
        if n > _PROJECT_MAX_YEARS:
            raise HectorAmdError("project: more than %d years (hx_member_project takes 1..%d)"
                                 % (_PROJECT_MAX_YEARS, _PROJECT_MAX_YEARS))
        if m > _PROJECT_MAX_OUT:
            raise HectorAmdError("project: more than %d basis rows (hx_member_project takes 1..%d)"
                                 % (_PROJECT_MAX_OUT, _PROJECT_MAX_OUT))
        if not np.isfinite(B).all():
            raise HectorAmdError("project: basis has a NaN or infinite entry")
        B = np.ascontiguousarray(B)
        cp = None
        if center is not None:
            ce = np.ascontiguousarray(np.atleast_1d(np.asarray(center, dtype=np.float64)))
            if ce.shape != yr.shape:
                raise HectorAmdError("project: center must have one entry per year")
            if not np.isfinite(ce).all():
                raise HectorAmdError("project: center has a NaN or infinite entry")
            cp = ce.ctypes.data_as(dp)
        b0, b1 = (1, 0) if baseline is None else (int(baseline[0]), int(baseline[1]))
        out = np.empty((m, self.n_members))
        self._ck(self._lib.hx_member_project(
            self._h, var.encode(), yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), cp, B.ctypes.data_as(dp),
            n, m, b0, b1, out.ctypes.data_as(dp)))
        return out[0] if one else out

    def _groups(self, groups, what):
        """groups= of the summary verbs: labels[n_members] (integers, -1 = in no group), or
        (labels, G); G defaults to max(label) + 1 -> (labels as contiguous int32, G)."""
        g = None
        if isinstance(groups, tuple) and len(groups) == 2 and np.ndim(groups[1]) == 0 and np.ndim(groups[0]) > 0:
            groups, g = groups
            if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer)):
                raise HectorAmdError("%s: the number of groups must be an integer" % what)
            g = int(g)
        lab = np.asarray(groups)
        if lab.shape != (self.n_members,):
            raise HectorAmdError("%s: groups must have n_members labels" % what)
        if lab.dtype == np.bool_ or not np.issubdtype(lab.dtype, np.integer):
            raise HectorAmdError("%s: the labels of groups must be integers (dtype %s)" % (what, lab.dtype))
        if g is None:
            g = int(lab.max()) + 1
        if not 1 <= g <= GROUP_MAX:
            raise HectorAmdError("%s: the number of groups must lie in 1..%d (it is %d)" % (what, GROUP_MAX, g))
        if int(lab.min()) < -1 or int(lab.max()) >= g:
            bad = int(lab.min()) if int(lab.min()) < -1 else int(lab.max())
            raise HectorAmdError("%s: label %d lies outside -1..%d" % (what, bad, g - 1))
        return np.ascontiguousarray(lab.astype(np.int32)), g

    def _window(self, dates):
        """dates= of the verbs over years (None: every year run so far) -> (year0, year1, n_years)."""
        y0, y1 = (self.strtdate, self.current_date) if dates is None else \
            (int(min(dates)), int(max(dates)))
        return y0, y1, max(y1 - y0 + 1, 0)

    def _weights(self, weights, what):
        if weights is None:
            return None
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
        if w.shape != (self.n_members,):
            raise HectorAmdError("%s: weights must have n_members entries" % what)
        return w

    # The summary verbs, once each: rows is a _Rows, groups what the caller gave (None: ungrouped).

    def _quantiles(self, rows, groups, probs, weights, counts):
        grp = None if groups is None else self._groups(groups, rows.what)
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if pr.ndim != 1:
            raise HectorAmdError("%s: probs must be one-dimensional" % rows.what)
        w = self._weights(weights, rows.what)
        out = np.empty(rows.shape(grp, pr.size))
        npart = np.zeros(rows.shape(grp), dtype=np.int64)
        rows.call("quantiles", grp, w, pr, int(pr.size), out, npart)
        return (out, npart) if counts else out

    def _probabilities(self, rows, groups, edges, weights, counts, sums):
        grp = None if groups is None else self._groups(groups, rows.what)
        ed = np.ascontiguousarray(np.atleast_1d(np.asarray(edges, dtype=np.float64)))
        if ed.ndim != 1:
            raise HectorAmdError("%s: edges must be one-dimensional" % rows.what)
        w = self._weights(weights, rows.what)
        prob = np.empty(rows.shape(grp, ed.size + 1))
        qs = np.zeros(rows.shape(grp, ed.size + 1), dtype=np.uint64)
        npart = np.zeros(rows.shape(grp), dtype=np.int64)
        rows.call("probabilities", grp, w, ed, int(ed.size), prob, qs, npart)
        res = (prob,) + ((npart,) if counts else ()) + ((qs,) if sums else ())
        return res if len(res) > 1 else prob

    def _moments(self, rows, groups, weights, against):
        grp = None if groups is None else self._groups(groups, rows.what)
        names, pred, w, q, pshift = self._against(against, weights, rows.what)
        k = len(names)
        shift = np.empty(rows.shape(grp))
        sums = np.zeros(rows.shape(grp, 2 + 3 * k))
        wsum = np.zeros(rows.shape(grp), dtype=np.uint64)
        npart = np.zeros(rows.shape(grp), dtype=np.int64)
        if grp is None:
            rows.call("moments", None, w, pred, k, shift, sums, wsum, npart)
            return Moments(shift, sums, wsum, npart, names, pshift, q, pred)
        pshift = np.full((grp[1], k), np.nan)   # (a grouped call returns every group's shifts itself)
        rows.call("moments", grp, w, pred, k, shift, pshift, sums, wsum, npart)
        return GroupedMoments(shift, sums, wsum, npart, names, pshift, q, pred, grp[0])

    def _sobol(self, rows, factors, n_base, use):
        names = ["factor[%d]" % i for i in range(int(factors))] if isinstance(factors, (int, np.integer)) \
            else [str(f) for f in factors]
        k = len(names)
        if k > SOBOL_MAX_FACTORS:
            raise HectorAmdError("%s: at most %d factors" % (rows.what, SOBOL_MAX_FACTORS))
        nb = self.n_members // (k + 2) if n_base is None else int(n_base)
        u = None
        if use is not None:
            u = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8)
            if u.shape != (nb,):
                raise HectorAmdError("%s: use must have n_base entries" % rows.what)
        shift = np.empty(rows.nrows)
        sums = np.zeros((rows.nrows, 4 + 4 * k))
        npart = np.zeros(rows.nrows, dtype=np.int64)
        rows.call("sobol", None, k, nb, u, shift, sums, npart)
        return Sobol(names, shift, sums, npart)

    def quantiles(self, var, probs, dates=None, weights=None, counts=False, groups=None):
        """Per-year weighted quantiles over every member, on the device (hx_ensemble_quantiles:
        exact inverted-CDF quantiles, numpy's method="inverted_cdf") -> ndarray [n_years, n_probs];
        counts=True: also the members that took part in every year [n_years].
        groups: labels[n_members] in 0..G-1 (-1: in no group), or (labels, G) with G <= 16: the
        quantiles of every group from ONE call (hx_group_quantiles; the weights are quantised over
        the whole ensemble) -> [G, n_years, n_probs], counts [G, n_years].  Measured
        (profiles/post_summaries.md, 65 536 members, 556 years, 5 probabilities): 0.46 of the time of
        the G masked calls at G = 8 and 0.40 at G = 16, but 1.57 times the two masked calls at G = 2,
        where the grouped select's fixed cost is not yet repaid."""
        return self._quantiles(_Rows.window(self, "quantiles", var, dates), groups, probs, weights, counts)

    def metrics(self, var, specs):
        """One number per member and specification, on the device (hx_member_metrics): windowed
        mean / min / max / year of min or max / first year at or above a threshold / years at or
        above it / least-squares trend of a recorded output, optionally relative to the member's
        own reference-period mean -> ndarray [n_specs, n_members].  The evaluation order is fixed
        (include/hector_amd.h): numpy reproduces the result bit for bit."""
        rows = _Rows.metrics(self, "metrics", var, specs)
        out = np.empty((rows.nrows, self.n_members))
        rows.call("members", None, out)
        return out

    def metric_quantiles(self, var, specs, probs, weights=None, counts=False, groups=None):
        """Weighted quantiles of every metric over the ensemble (hx_metric_quantiles: the metrics
        are computed and selected on the device, definition as quantiles()) -> ndarray
        [n_specs, n_probs]; counts=True: also the members that took part [n_specs].  groups: as in
        quantiles() -> [G, n_specs, n_probs], counts [G, n_specs]."""
        return self._quantiles(_Rows.metrics(self, "metric_quantiles", var, specs), groups, probs, weights, counts)

    def probabilities(self, var, edges, dates=None, weights=None, counts=False, sums=False, groups=None):
        """Per-year weighted probabilities of the classes x < edges[0], edges[0] <= x < edges[1],
        ..., x >= edges[-1] over every member, on the device (hx_ensemble_probabilities: one pass
        over the rows, exact integer sums) -> ndarray [n_years, n_edges + 1]; counts=True: also
        the members that took part [n_years]; sums=True: also the integer sums (uint64).
        groups: as in quantiles() -- the classes of every group from ONE pass
        (hx_group_probabilities) -> [G, n_years, n_edges + 1], counts [G, n_years], sums likewise:
        for one year, the contingency table of (group x class)."""
        return self._probabilities(_Rows.window(self, "probabilities", var, dates), groups, edges, weights, counts,
                                   sums)

    def metric_probabilities(self, var, specs, edges, weights=None, counts=False, sums=False, groups=None):
        """The same classes over metrics (hx_metric_probabilities) -> ndarray
        [n_specs, n_edges + 1] (+ counts [n_specs], + sums).  groups: as in probabilities() ->
        [G, n_specs, n_edges + 1]."""
        return self._probabilities(_Rows.metrics(self, "metric_probabilities", var, specs), groups, edges, weights,
                                   counts, sums)

    def pair_metrics(self, var_a, b, specs):
        """One number per member and specification from TWO series of that member, on the device
        (hx_member_pair_metrics): the regression of var_a on b (slope, intercept, r2), var_a where b
        first reaches a threshold / peaks / bottoms out, its mean while b is at or above a threshold,
        or the ratio of the two end-to-end changes -> ndarray [n_specs, n_members].
        b: a variable name, or (years, values) -- a per-year vector that is the same for every member
        (cumulative emissions, the year itself).  The evaluation order is fixed
        (include/hector_amd.h): numpy reproduces the result bit for bit."""
        rows = _Rows.pair_metrics(self, "pair_metrics", var_a, b, specs)
        out = np.empty((rows.nrows, self.n_members))
        rows.call("members", None, out)
        return out

    def pair_metric_quantiles(self, var_a, b, specs, probs, weights=None, counts=False):
        """Weighted quantiles of every pair metric over the ensemble (hx_pair_metric_quantiles;
        definition as metric_quantiles()) -> ndarray [n_specs, n_probs] (+ counts [n_specs])."""
        return self._quantiles(_Rows.pair_metrics(self, "pair_metric_quantiles", var_a, b, specs), None, probs,
                               weights, counts)

    def pair_metric_probabilities(self, var_a, b, specs, edges, weights=None, counts=False, sums=False):
        """The classes of probabilities() over pair metrics (hx_pair_metric_probabilities) -> ndarray
        [n_specs, n_edges + 1] (+ counts [n_specs], + sums)."""
        return self._probabilities(_Rows.pair_metrics(self, "pair_metric_probabilities", var_a, b, specs), None,
                                   edges, weights, counts, sums)

    def pair_metric_moments(self, var_a, b, specs, weights=None, against=None):
        """moments() over pair metrics (hx_pair_metric_moments): one row per specification -> Moments."""
        return self._moments(_Rows.pair_metrics(self, "pair_metric_moments", var_a, b, specs), None, weights,
                             against)

    def _against(self, against, weights, what):
        """-> (names, predictors [K, n_members] or None, weights or None, q [n_members] uint64,
        pshift [K]).  q and pshift restate the library's definition (include/hector_amd.h: q =
        rint(w / wmax * 2^32), c_k the smallest predictor over the members with q > 0 and all
        predictors finite) for Moments.pmean and Moments.src(); tests/test_gpu_moments.py holds wsum
        and pshift against the same definition."""
        w = self._weights(weights, what)
        single = isinstance(against, str) or (isinstance(against, tuple) and len(against) == 2 and
                                               isinstance(against[1], Metric)) or \
            (isinstance(against, tuple) and len(against) == 3 and isinstance(against[2], PairMetric)) or \
            (isinstance(against, np.ndarray) and against.ndim == 1)   # one array is one entry
        entries = [] if against is None else ([against] if single else list(against))
        if len(entries) > MOMENTS_MAX_AGAINST:
            raise HectorAmdError("%s: at most %d entries in against" % (what, MOMENTS_MAX_AGAINST))
        names, cols = [], []
        for i, a in enumerate(entries):
            if isinstance(a, str):
                names.append(a)
                cols.append(self.getvar(a))
            elif isinstance(a, tuple) and len(a) == 2 and isinstance(a[1], Metric):
                names.append("%s %r" % (a[0], a[1]))
                cols.append(self.metrics(a[0], [a[1]])[0])
            elif isinstance(a, tuple) and len(a) == 3 and isinstance(a[2], PairMetric):
                names.append("%s | %s %r" % (a[0], a[1] if isinstance(a[1], str) else "vector", a[2]))
                cols.append(self.pair_metrics(a[0], a[1], [a[2]])[0])
            else:
                v = np.asarray(a, dtype=np.float64)
                if v.shape != (self.n_members,):
                    raise HectorAmdError("%s: entry %d of against must have n_members values" % (what, i))
                names.append("against[%d]" % i)
                cols.append(v)
        pred = np.ascontiguousarray(np.stack(cols)) if cols else None
        # the integer weights and predictor shifts as include/hector_amd.h defines them (for pmean, src)
        if w is None:
            q = np.ones(self.n_members, dtype=np.uint64)
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                q = np.rint(w / w.max() * 2.0 ** 32)
            q = np.where(np.isfinite(q) & (q > 0), q, 0).astype(np.uint64)   # (a bad weight: the call refuses it)
        pshift = np.full(len(names), np.nan)
        if pred is not None:
            on = (q > 0) & np.isfinite(pred).all(axis=0)
            if on.any():
                pshift = pred[:, on].min(axis=1)
        return names, pred, w, q, pshift

    def moments(self, var, dates=None, weights=None, against=None, groups=None):
        """Per-year weighted mean and variance of `var` over the ensemble and its covariance,
        correlation and regression slope against per-member quantities, on the device
        (hx_ensemble_moments) -> Moments.  against: a list of parameter names (getvar), arrays
        [n_members], (var, Metric) pairs (metrics) or (var_a, b, PairMetric) triples (pair_metrics),
        at most 8.  A member takes part in a year if
        its weight is not 0, its value is not NaN and all its `against` values are finite.
        groups: as in quantiles() -- the moments of every group from one call (hx_group_moments) ->
        GroupedMoments: gm[g] is the Moments of group g, and gm.between / gm.within / gm.eta2
        partition every year's variance into the spread of the group means and the spread inside
        the groups."""
        return self._moments(_Rows.window(self, "moments", var, dates), groups, weights, against)

    def metric_moments(self, var, specs, weights=None, against=None, groups=None):
        """The same over metrics (hx_metric_moments): one row per specification -> Moments
        (groups: -> GroupedMoments, as in moments())."""
        return self._moments(_Rows.metrics(self, "metric_moments", var, specs), groups, weights, against)

    def sobol(self, var, factors, dates=None, n_base=None, use=None):
        """Per-year first-order and total Sobol indices of `var` with respect to the factors of a
        Saltelli design, on the device (hx_ensemble_sobol) -> Sobol.  The members must be laid out as
        hector_amd.ensemble.saltelli gives them: n_base groups of k + 2 consecutive members (A_j, B_j,
        then A_j with factor i from B_j).  factors: the number of factors k or a list of k names
        (labels only), at most 16; n_base defaults to n_members // (k + 2), members past
        n_base * (k + 2) are ignored; use[n_base]: groups with a zero entry take no part.  A group
        takes part in a year if none of its k + 2 values is NaN."""
        return self._sobol(_Rows.window(self, "sobol", var, dates), factors, n_base, use)

    def metric_sobol(self, var, specs, factors, n_base=None, use=None):
        """The same over metrics (hx_metric_sobol): one row per specification -> Sobol."""
        return self._sobol(_Rows.metrics(self, "metric_sobol", var, specs), factors, n_base, use)

    def comoments(self, var_a, dates_a=None, var_b=None, dates_b=None, weights=None):
        """Year-by-year weighted co-moments of two windows over the ensemble, on the device
        (hx_ensemble_comoments) -> CoMoments: the covariance / correlation matrix of the years
        dates_a of var_a against the years dates_b of var_b.  var_b=None and dates_b=None is the
        symmetric call (B is A; only the blocks on or above the diagonal are computed and mirrored:
        an exactly symmetric matrix; CoMoments.pca);
        dates_b alone means var_b = var_a.  A member takes part if its weight is not 0 and none of
        its values in either window is NaN (complete cases: one W, one n_part)."""
        dp = ctypes.POINTER(ctypes.c_double)
        w = self._weights(weights, "comoments")
        whole = (self.strtdate, self.current_date)
        a0, a1 = whole if dates_a is None else (int(min(dates_a)), int(max(dates_a)))
        sym = var_b is None and dates_b is None
        if sym:
            b0, b1, vb = a0, a1, None
        else:
            b0, b1 = whole if dates_b is None else (int(min(dates_b)), int(max(dates_b)))
            vb = (var_a if var_b is None else var_b).encode()
        for y0, y1 in ((a0, a1), (b0, b1)):   # (nothing is sized from a window outside the scenario)
            if y0 < self.strtdate or y1 > self.enddate or y1 < y0:
                raise HectorAmdError("hx_ensemble_comoments: dates must lie between startDate and the "
                                     "current date")
        na, nb = a1 - a0 + 1, b1 - b0 + 1
        shift_a, sums_a = np.empty(na), np.zeros((na, 2))
        shift_b, sums_b = np.empty(nb), np.zeros((nb, 2))
        cross = np.zeros((na, nb))
        wsum, npart = ctypes.c_ulonglong(0), ctypes.c_longlong(0)
        self._ck(self._lib.hx_ensemble_comoments(
            self._h, var_a.encode(), a0, a1, vb, b0, b1, w.ctypes.data_as(dp) if w is not None else None,
            shift_a.ctypes.data_as(dp), sums_a.ctypes.data_as(dp), shift_b.ctypes.data_as(dp),
            sums_b.ctypes.data_as(dp), cross.ctypes.data_as(dp), ctypes.byref(wsum), ctypes.byref(npart)))
        return CoMoments(shift_a, sums_a, shift_b, sums_b, cross, wsum.value, npart.value,
                         np.arange(a0, a1 + 1), np.arange(b0, b1 + 1), symmetric=sym)

    def hold(self, name, var):
        """Keep the trajectory of every member of `var` -- a recorded output, a derived diagnostic
        or a series -- as the series `name` (hx_series_define, COPY): a snapshot on the device that
        later reset / run / setvar do not touch, and that every summary verb and fetchvars take
        like a variable."""
        return self.derive(name, "copy", var)

    def derive(self, name, op, a, b=None, *, years=None, width=None, align="trailing", lag=None,
               first_year=None):
        """Define the series `name` from the per-member variable `a` on the device, one operation
        per call (hx_series_define in include/hector_amd.h fixes every order: numpy reproduces the
        result bit for bit).  op: "copy"; "add" / "sub" / "mul" / "div" with b = a variable name, a
        number, or a per-year vector that starts at first_year (NaN outside its span); "anomaly"
        with years = (year0, year1), the member's own reference period; "cumsum" with years = the
        first year; "runmean" with width and align = "trailing" or "centred"; "delta" with lag.
        Defining an existing series replaces it; the operands may name it."""
        if op not in SERIES_OPS:
            raise HectorAmdError("hx_series_define: unknown op %r (one of %s)" % (op, ", ".join(SERIES_OPS)))
        o = _HxSeriesOp()
        o.op = SERIES_OPS[op]
        keep = None
        if years is not None:
            y = np.atleast_1d(np.asarray(years)).astype(np.int64)
            o.year0, o.year1 = int(y.min()), int(y.max())
        if width is not None:
            o.width = int(width)
        if align not in ("trailing", "centred", "centered"):
            raise HectorAmdError("hx_series_define: align must be 'trailing' or 'centred'")
        o.align = 0 if align == "trailing" else 1
        if lag is not None:
            o.lag = int(lag)
        if isinstance(b, str):
            o.b_kind, o.b = 1, b.encode()
        elif b is not None and np.ndim(b) == 0:
            o.b_kind, o.b_scalar = 2, float(b)
        elif b is not None:
            if first_year is None:
                raise HectorAmdError("hx_series_define: a per-year vector b needs first_year")
            keep = np.ascontiguousarray(np.asarray(b, dtype=np.float64).ravel())
            o.b_kind, o.b_first_year, o.b_n = 3, int(first_year), int(keep.size)
            o.b_values = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self._ck(self._lib.hx_series_define(self._h, name.encode(), a.encode(), ctypes.byref(o)))
        return self

    def derive_expr(self, name, expr, bind=None):
        """Define the series `name` from a whole expression over per-member variables, evaluated on
        the device in one launch (hx_series_eval in include/hector_amd.h: every distinct operand row
        is read once, the result written once, nothing reaches the host).  expr: text -- the grammar
        is hector_amd.expr's: + - * /, comparisons, & | ~ on indicators, ** 2..4, abs sqrt log exp
        minimum maximum where ifnan lag(x, k), var("name"), param("S"), year -- or a compiled
        hector_amd.expr.Program; bind: names of the text -> a variable name (an alias), an n_members
        array, expr.param("S") (the members' parameter, through getvar as `against=` does),
        (first_year, values) or a number.  Everything but log and exp is what Program.numpy gives,
        bit for bit.  Defining an existing series replaces it; the expression may name it."""
        from . import expr as _expr
        if isinstance(expr, _expr.Program):
            if bind is not None:
                raise HectorAmdError("hx_series_eval: bind goes with text; a Program is compiled already")
            prog = expr
        else:
            prog = _expr.compile(expr, bind)
        ex, keep = prog._c(self.n_members, self.getvar)
        self._ck(self._lib.hx_series_eval(self._h, name.encode(), ctypes.byref(ex)))
        del keep
        return self

    def drop_series(self, name):
        self._ck(self._lib.hx_series_drop(self._h, name.encode()))
        return self

    def series(self):
        """-> {name: the last year that holds values} of the core's series, in definition order."""
        names = ctypes.POINTER(ctypes.c_char_p)()
        years = ctypes.POINTER(ctypes.c_int)()
        n = ctypes.c_int()
        self._ck(self._lib.hx_series_list(self._h, ctypes.byref(names), ctypes.byref(years), ctypes.byref(n)))
        return {names[i].decode(): int(years[i]) for i in range(n.value)}

    def rank_series(self, name, var, dates=None, weights=None, kind="pit"):
        """Define the series `name` as every member's weighted mid-rank of `var` within its year, by
        a sort of every row on the device (hx_series_rank; hector_amd.ensemble.midpit is the same
        definition in numpy, bit for bit).  kind "pit": (2 L + E) / (2 W) in (0, 1], the share of the
        ensemble's weight below the member, ties counted half; "numerator": the exact integer
        2 L + E.  The rows of `dates` (default: all years run) hold the ranks, every other row NaN.
        As a series the ranks feed the other verbs: moments(name, against=ranked predictors) is a
        Spearman correlation (spearman() does that), probabilities(name, edges) a rank histogram,
        derive and metrics a trajectory's depth."""
        if kind not in RANK_KINDS:
            raise HectorAmdError("rank_series: kind must be 'pit' or 'numerator'")
        w = self._weights(weights, "rank_series")
        y0, y1, _ = self._window(dates)
        self._ck(self._lib.hx_series_rank(
            self._h, name.encode(), var.encode(), y0, y1,
            w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if w is not None else None, RANK_KINDS[kind]))
        return self

    def metric_ranks(self, var, specs, weights=None, kind="pit"):
        """Every member's weighted mid-rank among the members, metric by metric (hx_metric_ranks: the
        metrics of hx_member_metrics are computed and sorted on the device) -> ndarray
        [n_specs, n_members]; NaN where a member's metric is NaN.  kind as in rank_series()."""
        if kind not in RANK_KINDS:
            raise HectorAmdError("metric_ranks: kind must be 'pit' or 'numerator'")
        rows = _Rows.metrics(self, "metric_ranks", var, specs)
        w = self._weights(weights, "metric_ranks")
        out = np.empty((rows.nrows, self.n_members))
        rows.call("ranks", None, w, RANK_KINDS[kind], out)
        return out

    def crps(self, var, years, obs, weights=None, return_pit=False, counts=False):
        """The continuous ranked probability score of the weighted ensemble against the observation
        obs[i] of the year years[i], on the device (hx_ensemble_crps; hector_amd.ensemble.crps is the
        definition in numpy) -> ndarray [n_years].  The years need not be ascending or contiguous; a
        NaN observation, or a year in which no member takes part, gives NaN.  return_pit=True: also
        the mid-PIT of every observation within its year's ensemble (their histogram is the rank
        histogram); counts=True: also the members that took part."""
        yr = np.ascontiguousarray(np.atleast_1d(np.asarray(years)).astype(np.int32))
        ob = np.ascontiguousarray(np.atleast_1d(np.asarray(obs, dtype=np.float64)))
        if yr.ndim != 1 or ob.shape != yr.shape:
            raise HectorAmdError("crps: years and obs must be one-dimensional and of one length")
        w = self._weights(weights, "crps")
        dp = ctypes.POINTER(ctypes.c_double)
        out, pit = np.empty(yr.size), np.empty(yr.size)
        npart = np.zeros(yr.size, dtype=np.int64)
        self._ck(self._lib.hx_ensemble_crps(
            self._h, var.encode(), yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ob.ctypes.data_as(dp),
            int(yr.size), w.ctypes.data_as(dp) if w is not None else None, out.ctypes.data_as(dp),
            pit.ctypes.data_as(dp), npart.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        res = (out,) + ((pit,) if return_pit else ()) + ((npart,) if counts else ())
        return res if len(res) > 1 else out

    def spearman(self, var, against, dates=None, weights=None):
        """Per-year weighted Spearman rank correlation of `var` with per-member quantities ->
        ndarray [n_years, K]: the Pearson correlation (moments().corr) of the members' mid-ranks
        within the year (a temporary rank series, dropped again) with the mid-ranks of every
        predictor (hector_amd.ensemble.midpit, same weights).  against: as in moments() -- parameter
        names, arrays [n_members], (var, Metric) pairs.  The core must have room for one more
        series (16 at most)."""
        from . import ensemble
        names, pred, w, _, _ = self._against(against, weights, "spearman")
        if pred is None:
            raise HectorAmdError("spearman: against is empty")
        ranked = [ensemble.midpit(p, w) for p in pred]
        have = self.series()
        temp = next(t for t in ("_spearman_%d" % i for i in range(len(have) + 1)) if t not in have)
        self.rank_series(temp, var, dates, weights)
        try:
            return self.moments(temp, dates, weights, against=ranked).corr
        finally:
            self.drop_series(temp)

    def status(self):
        out = np.zeros(self.n_members, dtype=np.uint32)
        self._ck(self._lib.hx_status(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))))
        return out

    def state_row(self, row):
        out = np.empty(self.n_members)
        self._ck(self._lib.hx_state_row(self._h, int(row),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def spinup_steps(self, member=0):
        s = ctypes.c_int()
        self._ck(self._lib.hx_spinup_steps(self._h, int(member), ctypes.byref(s)))
        return s.value

    def last_run_ms(self):
        v = ctypes.c_double()
        self._ck(self._lib.hx_last_run_ms(self._h, ctypes.byref(v)))
        return v.value

    def set_pair_kernel_limit(self, max_members):
        """Ensembles of up to max_members (one biome, no constraints, outputs within
        CO2/tas/forcing/pools/NBP/pH) run on the
        two-wavefront kernel (include/hector_amd.h); 0 switches it off."""
        self._ck(self._lib.hx_set_pair_kernel_limit(self._h, int(max_members)))
        return self

    def wave_clock(self, shard=0):
        """-> int64 array [wavefronts][2]: start and end of every wavefront of the last run's
        year-loop launch, in ticks of the device's constant 100 MHz clock relative to the earliest
        start (hx_wave_clock): the launch's tail, wavefront by wavefront."""
        cap = 2 * ((self.n_members + 63) // 64)
        buf = np.zeros((cap, 2), dtype=np.int64)
        n = ctypes.c_int(0)
        self._ck(self._lib.hx_wave_clock(self._h, int(shard), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                         cap, ctypes.byref(n)))
        return buf[:n.value]

    def wave_epilogue_clock(self, shard=0):
        """-> int64 array [wavefronts]: ticks of the same clock every wavefront of the last launch
        spent behind its year loop on its partial statistics (hx_wave_epilogue_clock); empty when
        the launch wrote none."""
        cap = 2 * ((self.n_members + 63) // 64)
        buf = np.zeros(cap, dtype=np.int64)
        n = ctypes.c_int(0)
        self._ck(self._lib.hx_wave_epilogue_clock(self._h, int(shard),
                                                  buf.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                                  cap, ctypes.byref(n)))
        return buf[:n.value]

    def set_two_wave_from(self, min_members):
        """Ensembles of at least min_members members (one biome, no carbon
        tracking) run on the flavour of the kernel built for two resident
        wavefronts per SIMD (include/hector_amd.h); < 0: the default (more wavefronts than the
        GPU has SIMDs), 0: never."""
        self._ck(self._lib.hx_set_two_wave_from(self._h, int(min_members)))
        return self

    def set_prewarm(self, ms):
        """Keep the chip's clocks up while run()'s preparation uploads and spins up after an idle
        gap (hx_set_prewarm): at most `ms` milliseconds of a small busy loop, 0 = off."""
        self._ck(self._lib.hx_set_prewarm(self._h, int(ms)))
        return self

    def last_run_prewarmed(self):
        v = ctypes.c_int(0)
        self._ck(self._lib.hx_last_run_prewarmed(self._h, ctypes.byref(v)))
        return bool(v.value)

    def last_run_kernel(self):
        """'run', 'run2' or 'pair': the kernel the last run() launched."""
        s = ctypes.c_char_p()
        self._ck(self._lib.hx_last_run_kernel(self._h, ctypes.byref(s)))
        return s.value.decode()

    def last_run_variant(self):
        """The run-kernel family of the last run(): 0 plain, -2 plain + diagnostics, -1 extended,
        1 extended with the NBP machinery, 2 carbon tracking (hx_last_run_variant)."""
        v = ctypes.c_int()
        self._ck(self._lib.hx_last_run_variant(self._h, ctypes.byref(v)))
        return v.value

    def last_run_retries(self):
        """1: the last run() took the solver's retries inside the step loop, discarded steps executed
        and counted (solver_steps recorded, or HECTOR_AMD_FAITHFUL_RETRIES=1); 0: at the head of the
        segment (hx_last_run_retries)."""
        v = ctypes.c_int()
        self._ck(self._lib.hx_last_run_retries(self._h, ctypes.byref(v)))
        return v.value

    def last_spinup_ms(self):
        v = ctypes.c_double()
        self._ck(self._lib.hx_last_spinup_ms(self._h, ctypes.byref(v)))
        return v.value

    def shutdown(self):
        if self._h:
            self._lib.hx_shutdown(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.shutdown()
        except Exception:
            pass


def comm_unique_id(lib_path=None, allow_emulation=False):
    """128 bytes that identify a new RCCL communicator (hx_comm_unique_id): made by ONE process,
    handed to the others by the host's own means (MPI, a torch.distributed store, a file)."""
    lib = _lib.load(lib_path, allow_emulation)
    buf = ctypes.create_string_buffer(128)
    if lib.hx_comm_unique_id(buf) != 0:
        raise HectorAmdError(lib.hx_last_error().decode())
    return buf.raw


def cost_models_export(path, lib_path=None, allow_emulation=False):
    """Write every lane-cost model this process holds to `path` (hx_cost_models_export) -> count."""
    lib = _lib.load(lib_path, allow_emulation)
    n = ctypes.c_int(0)
    if lib.hx_cost_models_export(os.fsencode(path), ctypes.byref(n)) != 0:
        raise HectorAmdError(lib.hx_last_error().decode())
    return n.value


def cost_models_load(path, lib_path=None, allow_emulation=False):
    """Add the lane-cost models of a file to the process's registry (hx_cost_models_load) -> count."""
    lib = _lib.load(lib_path, allow_emulation)
    n = ctypes.c_int(0)
    if lib.hx_cost_models_load(os.fsencode(path), ctypes.byref(n)) != 0:
        raise HectorAmdError(lib.hx_last_error().decode())
    return n.value


# R-style free functions
def newcore(inifile=None, n_members=1, device=0, **kw):
    return Core(inifile, n_members, device, **kw)


def run(core, runtodate=-1):
    return core.run(runtodate)


def reset(core, date=0):
    return core.reset(date)


def shutdown(core):
    core.shutdown()


def isactive(core):
    """isactive(core)  R/hector.R:122-125: false after shutdown()."""
    return bool(core._h)


def startdate(core):
    return core.strtdate


def enddate(core):
    return core.enddate


def getdate(core):
    return core.current_date


def getname(core):
    return core.name


def get_biome_list(core):
    return core.biomes()


def getunits(vars, core):
    """getunits(vars)  R/units.R:10-21: unit strings; None (R: NA + a warning) for unknown names.
    The table lives in the library (hx_var_info), hence the core argument."""
    out = []
    for v in ([vars] if isinstance(vars, str) else vars):
        try:
            out.append(core.getunits(v))
        except HectorAmdError:
            out.append(None)
    return out[0] if isinstance(vars, str) else out


def getfxn(strings):
    """getfxn(str)  R/fxns.R:11-21: the accessor ('BETA()') that returns a capability string;
    None for unknown strings."""
    from . import capabilities
    rev = {}
    for fn, (cap, _per_biome) in capabilities._TABLE.items():
        rev.setdefault(cap, fn + "()")
    out = [rev.get(x) for x in ([strings] if isinstance(strings, str) else strings)]
    return out[0] if isinstance(strings, str) else out


def runscenario(infile, n_members=1, **kw):
    """runscenario(infile)  R/hector.R:57-63: run to the end, return the default variables."""
    core = newcore(infile, n_members, **kw)
    try:
        core.set_outputs(list(DEFAULT_FETCHVARS))
        core.run()
        return fetchvars(core, (core.strtdate, core.enddate))
    finally:
        core.shutdown()


def setvar(core, dates, var, values, unit=None):
    if not _is_na(dates):
        return core.setvar_dated(var, dates, values, unit)
    return core.setvar(var, values, unit)


def _is_na(dates):
    return dates is None or (isinstance(dates, float) and np.isnan(dates))


DEFAULT_FETCHVARS = ("CO2_concentration", "RF_tot", "RF_CO2", "global_tas")   # R/messages.R:4 default_fetchvars


def fetchvars(core, dates, variables=None):
    """fetchvars(core, dates, vars)  R/messages.R:46-88.  dates = a tuple (year0, year1) for the
    whole range or a list of years: -> dict variable -> ndarray [n_dates, n_members]; dates =
    None / NaN (R's NA), for parameters: -> dict variable -> ndarray [n_members]."""
    if variables is None:   # getOption("hector.default.fetchvars"), R/messages.R:47-56
        if _is_na(dates):
            raise HectorAmdError("The default vars (%s) all require dates" % ", ".join(DEFAULT_FETCHVARS))
        variables = list(DEFAULT_FETCHVARS)
    if isinstance(variables, str):
        variables = [variables]
    if _is_na(dates):
        return {v: core.getvar(v) for v in variables}
    # dates outside startDate..current date are dropped, none left is an error (:62-72)
    strt, cur = core.strtdate, core.current_date
    want = [int(d) for d in np.atleast_1d(dates)]
    if len(want) == 2 and isinstance(dates, tuple):      # (year0, year1): the whole range
        want = list(range(min(want), max(want) + 1))
    valid = [d for d in want if strt <= d <= cur]
    if not valid:
        raise HectorAmdError("None of these dates are valid for this core (start=%d, current=%d)"
                             % (strt, cur))
    lo, hi = min(valid), max(valid)
    idx = np.array(valid) - lo
    return {v: core.fetchvars(v, (lo, hi))[idx] for v in variables}


GETDATA, SETDATA = "getData", "setData"      # component_data.hpp:409-410


def sendmessage(core, msgtype, capability, date=None, value=None, unit=None):
    """sendmessage(core, msgtype, capability, date, value, unit)  src/rcpp_hector.cpp:262-350,
    the low-level message bus under setvar/fetchvars.  getData -> list of rows
    (year or None, variable, values[n_members], units); setData -> the core."""
    if msgtype == GETDATA:
        units = core.getunits(capability)
        if _is_na(date):
            return [(None, capability, core.getvar(capability), units)]
        years = [int(y) for y in np.atleast_1d(date)]
        data = core.fetchvars(capability, (min(years), max(years)))
        return [(y, capability, data[y - min(years)], units) for y in years]
    if msgtype == SETDATA:
        return setvar(core, date, capability, value, unit)
    raise HectorAmdError("sendmessage: unknown message type %r" % (msgtype,))


def get_tracking_data(core, member=0):
    """get_tracking_data(core)  R/hector.R: rows (year, component, pool_name, pool_value,
    pool_units, source_name, source_fraction) for one member, trackingDate .. current date."""
    start = int(core.getvar("trackingDate")[0])
    if start == 9999 or core.current_date < start:
        return []
    names = core.tracking_pools()
    v, f, held = core.tracking_data(member, (start, core.current_date), masks=True)
    rows = []
    for iy in range(v.shape[0]):
        for p, pn in enumerate(names):
            comp = "ocean" if pn in ("HL", "LL", "intermediate", "deep") else "simpleNbox"
            for s, sn in enumerate(names):
                if held[iy, p, s]:
                    rows.append((start + iy, comp, pn, v[iy, p], "Pg C", sn, f[iy, p, s]))
    return rows


_BIOME_PARAMS = ("warmingfactor", "beta", "q10_rh", "f_nppv", "f_nppd", "f_litterd")


def split_biome(core, old_biome, new_biomes, fveg_c=None, fdetritus_c=None, fsoil_c=None,
                fpermafrost_c=None, fnpp_flux0=None, **params):
    """split_biome(core, old_biome, new_biomes, ...)  R/biome.R:61-130.  `params`: warmingfactor,
    beta, q10_rh, f_nppv, f_nppd, f_litterd for the new biomes (a scalar, or one value per new
    biome); default: the old biome's."""
    new_biomes = list(new_biomes)
    bad = set(params) - set(_BIOME_PARAMS)
    if bad:
        raise HectorAmdError("split_biome: unknown biome parameter(s) %s" % sorted(bad))
    for name, f in (("fveg_c", fveg_c), ("fdetritus_c", fdetritus_c), ("fsoil_c", fsoil_c),
                    ("fpermafrost_c", fpermafrost_c), ("fnpp_flux0", fnpp_flux0)):
        if f is None:
            continue
        f = np.asarray(f, dtype=float)  # the stopifnot block of the R function
        lo_ok = (f >= 0).all() if name == "fpermafrost_c" else (f > 0).all()
        if f.size != len(new_biomes) or abs(f.sum() - 1.0) > 1e-12 or not lo_ok:
            raise HectorAmdError("split_biome: %s must be %d positive fractions summing to 1"
                                 % (name, len(new_biomes)))
    core.split_biome(new_biomes, fveg_c, fdetritus_c, fsoil_c, fpermafrost_c, fnpp_flux0,
                     old_biome=old_biome)
    for key, val in params.items():
        vals = np.broadcast_to(np.asarray(val, dtype=float), (len(new_biomes),))
        for b, v in zip(new_biomes, vals):
            core.setvar("%s.%s" % (b, key), [v])
    return core


def create_biome(core, biome, veg_c0, detritus_c0, soil_c0, permafrost_c0, npp_flux0,
                 warmingfactor, beta, q10_rh, f_nppv, f_nppd, f_litterd):
    """create_biome(core, biome, ...)  R/biome.R:20-40 (values: a scalar or one per member)."""
    core.create_biome(biome)
    for key, val in (("veg_c", veg_c0), ("detritus_c", detritus_c0), ("soil_c", soil_c0),
                     ("permafrost_c", permafrost_c0), ("npp_flux0", npp_flux0),
                     ("warmingfactor", warmingfactor), ("beta", beta), ("q10_rh", q10_rh),
                     ("f_nppv", f_nppv), ("f_nppd", f_nppd), ("f_litterd", f_litterd)):
        core.setvar("%s.%s" % (biome, key), np.atleast_1d(np.asarray(val, dtype=float)))
    return core


def rename_biome(core, oldname, newname):
    return core.rename_biome(oldname, newname)


def get_biome_inits(core, biome):
    """get_biome_inits(core, biome)  R/biome.R:140-170: initial pools and parameters of a biome
    (per member)."""
    pre = "" if (biome == "global" and core.biomes() == ["global"]) else biome + "."
    out = {k: core.getvar(pre + k) for k in ("veg_c", "detritus_c", "soil_c", "permafrost_c",
                                             "npp_flux0", "f_litterd", "f_nppd", "f_nppv", "beta",
                                             "q10_rh", "warmingfactor")}
    out["thawedp_c"] = np.zeros(core.n_members)  # always empty at t = 0 (simpleNbox.cpp:146)
    return out
