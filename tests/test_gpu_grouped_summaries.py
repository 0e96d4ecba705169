"""hx_group_quantiles / hx_group_probabilities / hx_group_moments (groups= of the summary verbs) on
the GPU.

The authority for group g is the project's own checker -- `checker` of tests/test_gpu_quantiles.py,
`bin_reference` of tests/test_gpu_metrics_probabilities.py, `checker` / `check_raw` of
tests/test_gpu_moments.py -- applied with q quantised from the FULL weight vector and then zeroed
outside the group.  Integer results (quantiles, bin sums, W, n_part, shifts) are compared with `==`,
the floating sums within the header's bound (n_part + 8) 2^-53 through check_raw, whose condition (no
term underflows or overflows) is asserted on the checker's own terms as tests/test_gpu_post_edges.py
does.

Rows are synthetic (tests/post_edge_cases.py) on cores run to 1790 without member sorting, at
n = 257 (one partial chunk), 8193 (a chunk plus one member) and 12289 (a chunk plus a batch edge).
Label patterns: m % 3; contiguous groups with a boundary exactly at member 8192, a group of one member
(member 8192), an empty group and every seventh member of the rest -1; sixteen groups of seeded random
labels with -1 among them (with sixteen probabilities: 256 select slots); one group of all members.
A real run with member sorting ON (lane order is not member order) holds the member / lane mapping
of the labels.

eta2 of the real run: against numpy in longdouble with the relative tolerance
4 kappa (n_part + 8) 2^-53 of tests/test_gpu_moments.py, where kappa is the largest cancellation that
enters it -- (B_g / W_g) / var_g of a group's variance and sum_g share_g dmean_g^2 / between of the
group means about the pooled mean (means taken relative to the smallest shift) -- and kappa <= 3e4 is
asserted.
"""
import ctypes

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, Moments, ensemble
from conftest import SCENARIO

import post_edge_cases as pe
from test_gpu_quantiles import _hip_runtime, _write_row, checker as q_checker
from test_gpu_metrics_probabilities import bin_reference
from test_gpu_moments import KAPPA_MAX, check_raw, checker as moments_checker, same_bits, within_bound

pytestmark = pytest.mark.gpu

E = hector_amd.HectorAmdError
VAR = "global_tas"
LD = np.longdouble
U = 2.0 ** -53
SIZES = (257, 8193, 12289)
_cores = {}


def _new_core(n, hip_lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def _row_core(n, hip_lib):
    c = _new_core(n, hip_lib)
    c.set_member_sorting(False)
    c.run(pe.RUN_TO)
    assert np.array_equal(c.lane_of_member(), np.arange(n))
    r = pe.rows(n)
    for k, name in enumerate(pe.ALL_ROWS):
        _write_row(c, VAR, pe.year_of(name), r[name], pad_value=pe.pad_value(k))
    x = c.fetchvars(VAR, (pe.FIRST_ROW_YEAR, pe.FIRST_ROW_YEAR + len(pe.ALL_ROWS) - 1))
    assert np.array_equal(x.view(np.uint64), pe.matrix(r, pe.ALL_ROWS).view(np.uint64))
    return c, r


@pytest.fixture(scope="module")
def row_core(hip_lib):
    def get(n):
        if n not in _cores:
            _cores[n] = _row_core(n, hip_lib)
        return _cores[n]
    yield get
    for c, _ in _cores.values():
        c.shutdown()
    _cores.clear()


def labels(n, pattern):
    """-> (labels[n] int32, G)."""
    i = np.arange(n)
    if pattern == "mod3":
        return (i % 3).astype(np.int32), 3
    if pattern == "contiguous":
        assert n > pe.CHUNK
        lab = np.where(i < pe.CHUNK, 0, 3)
        lab[i % 7 == 6] = -1
        lab[pe.CHUNK] = 1                      # a group of ONE member, first of the second chunk; group 2 is empty
        assert lab[pe.CHUNK - 1] == 0 and (lab == 1).sum() == 1 and not (lab == 2).any()
        return lab.astype(np.int32), 4
    if pattern == "random16":
        lab = np.random.default_rng(4000 + n).integers(-1, 16, n)
        assert (lab == -1).any() and len(set(lab)) == 17
        return lab.astype(np.int32), 16
    assert pattern == "one"
    return np.zeros(n, dtype=np.int32), 1


def patterns(n):
    return ("mod3", "random16", "one") + (("contiguous",) if n > pe.CHUNK else ())


CASES = [(n, p) for n in SIZES for p in patterns(n)]


def _years(names):
    ys = [pe.year_of(k) for k in names]
    assert ys == list(range(ys[0], ys[0] + len(ys)))
    return ys[0], ys[-1]


def check_group_quantiles(x, got, npart, q, lab, G, probs, what):
    assert got.shape == (G, x.shape[0], len(probs)) and npart.shape == (G, x.shape[0]), what
    for g in range(G):
        qg = np.where(lab == g, q, 0).astype(np.uint64)
        for y in range(x.shape[0]):
            ref, cnt = q_checker(x[y], qg, probs)
            assert npart[g, y] == cnt, (what, g, y, npart[g, y], cnt)
            if cnt == 0:
                assert np.isnan(got[g, y]).all(), (what, g, y, got[g, y])
            else:
                assert (got[g, y] == ref).all(), (what, g, y, got[g, y], ref)


def check_group_bins(x, res, q, lab, G, edges, what):
    prob, npart, sums = res
    assert prob.shape == sums.shape == (G, x.shape[0], len(edges) + 1) and sums.dtype == np.uint64, what
    for g in range(G):
        qg = np.where(lab == g, q, 0).astype(np.uint64)
        for y in range(x.shape[0]):
            ref, cnt = bin_reference(x[y], qg, edges)
            assert npart[g, y] == cnt, (what, g, y, npart[g, y], cnt)
            assert (sums[g, y] == ref).all(), (what, g, y, sums[g, y], ref)
            if cnt == 0:
                assert np.isnan(prob[g, y]).all(), (what, g, y)
            else:
                assert (prob[g, y] == ref.astype(np.float64) / float(int(ref.sum(dtype=np.uint64)))).all(), (what, g, y)


def check_group_moments(gm, x, q, lab, G, pred, what):
    """check_raw per group, on the group's slice as a Moments -> the groups' records."""
    assert gm.shift.shape == (G, x.shape[0]) and gm.pshift.shape == (G, pred.shape[0]), what
    refs = []
    for g in range(G):
        qg = np.where(lab == g, q, 0).astype(np.uint64)
        ref = moments_checker(x, qg, pred)
        assert pe.terms_zero_or_normal(x, qg, pred, ref) > 0 or ref["n_part"].sum() == 0, (what, g)
        m = gm[g]
        assert isinstance(m, Moments)
        check_raw(m, x, qg, pred, what + ("group", g))
        refs.append(ref)
    return refs


def _only_one_group_takes_part(npart, lab, n):
    """The weight setting "one": the last member alone has a weight, every other group has W = 0."""
    g1 = lab[n - 1]
    for g in range(npart.shape[0]):
        if g != g1:
            assert (npart[g] == 0).all(), g


@pytest.mark.parametrize("n,pattern", CASES)
def test_grouped_quantiles_on_the_edge_rows(row_core, n, pattern):
    core, r = row_core(n)
    lab, G = labels(n, pattern)
    names = pe.PART1_ROWS + pe.INTEGER_ONLY_ROWS
    rows = [pe.ALL_ROWS.index(k) for k in names]
    y0, y1 = _years(pe.ALL_ROWS)
    x = pe.matrix(r, pe.ALL_ROWS)
    for wname, w in pe.weight_settings(n).items():
        q = pe.q_of(n, w)
        for k in (1, 5, 16):
            probs = pe.probs_for(k)
            got, npart = core.quantiles(VAR, probs, (y0, y1), weights=w, counts=True, groups=(lab, G))
            check_group_quantiles(x[rows], got[:, rows], npart[:, rows], q, lab, G, probs, (n, pattern, wname, k))
            if wname == "one":
                _only_one_group_takes_part(npart, lab, n)
                assert np.isnan(got[[g for g in range(G) if g != lab[n - 1]]]).all()


@pytest.mark.parametrize("n,pattern", CASES)
def test_grouped_probabilities_on_the_edge_rows(row_core, n, pattern):
    core, r = row_core(n)
    lab, G = labels(n, pattern)
    y0, y1 = _years(pe.ALL_ROWS)
    x = pe.matrix(r, pe.ALL_ROWS)
    for edges in pe.EDGE_SETS:
        for wname, w in pe.weight_settings(n).items():
            res = core.probabilities(VAR, edges, (y0, y1), weights=w, counts=True, sums=True, groups=(lab, G))
            check_group_bins(x, res, pe.q_of(n, w), lab, G, edges, (n, pattern, wname, len(edges)))
            if wname == "one":
                _only_one_group_takes_part(res[1], lab, n)


@pytest.mark.parametrize("n,pattern", CASES)
def test_grouped_moments_on_the_edge_rows(row_core, n, pattern):
    core, r = row_core(n)
    lab, G = labels(n, pattern)
    y0, y1 = _years(pe.MOMENT_ROWS)
    x = pe.matrix(r, pe.MOMENT_ROWS)
    allp = pe.predictors(n)
    for k in (0, 3, 8):
        pred = allp[:k]
        against = [p for p in pred] if k else None
        for wname, w in pe.weight_settings(n).items():
            what = (n, pattern, "npred", k, wname)
            gm = core.moments(VAR, (y0, y1), weights=w, against=against, groups=(lab, G))
            check_group_moments(gm, x, pe.q_of(n, w), lab, G, pred, what)
            again = core.moments(VAR, (y0, y1), weights=w, against=against, groups=(lab, G))
            assert same_bits(gm, again) and np.array_equal(gm.pshift, again.pshift, equal_nan=True), what
            if wname == "one":
                _only_one_group_takes_part(gm.n_part, lab, n)


@pytest.mark.parametrize("n", SIZES)
def test_one_group_of_all_members_is_the_ungrouped_verb(row_core, n):
    core, r = row_core(n)
    lab, G = labels(n, "one")
    y0, y1 = _years(pe.ALL_ROWS)
    m0, m1 = _years(pe.MOMENT_ROWS)
    pred = [p for p in pe.predictors(n)[:3]]
    for wname, w in pe.weight_settings(n).items():
        a, na = core.quantiles(VAR, pe.probs_for(5), (y0, y1), weights=w, counts=True)
        b, nb = core.quantiles(VAR, pe.probs_for(5), (y0, y1), weights=w, counts=True, groups=lab)
        assert b.shape == (1,) + a.shape and np.array_equal(a, b[0], equal_nan=True) and np.array_equal(na, nb[0])
        ra = core.probabilities(VAR, pe.EDGE_SETS[1], (y0, y1), weights=w, counts=True, sums=True)
        rb = core.probabilities(VAR, pe.EDGE_SETS[1], (y0, y1), weights=w, counts=True, sums=True, groups=lab)
        assert all(np.array_equal(p, s[0], equal_nan=True) for p, s in zip(ra, rb)), (n, wname)
        ma = core.moments(VAR, (m0, m1), weights=w, against=pred)
        mb = core.moments(VAR, (m0, m1), weights=w, against=pred, groups=lab)
        within_bound(ma, mb[0], (n, wname))     # n_part, wsum and shift equal, the sums within the bound
        assert np.array_equal(ma.pshift, mb.pshift[0], equal_nan=True)


@pytest.mark.parametrize("n", (257, 8193))
def test_weights_whose_maximum_lies_in_every_group_equal_masked_calls(row_core, n):
    """With the largest weight inside every group a masked call quantises as the grouped call does."""
    core, r = row_core(n)
    lab, G = labels(n, "mod3")
    w = np.random.default_rng(5000 + n).choice([0.25, 0.5, 1.0], n)
    w[:3] = 1.0
    assert all((w[lab == g] == 1.0).any() for g in range(G))
    y0, y1 = _years(pe.ALL_ROWS)
    m0, m1 = _years(pe.MOMENT_ROWS)
    probs = pe.probs_for(5)
    pred = [p for p in pe.predictors(n)[1:3]]
    gq, gn = core.quantiles(VAR, probs, (y0, y1), weights=w, counts=True, groups=lab)
    gp = core.probabilities(VAR, pe.EDGE_SETS[2], (y0, y1), weights=w, counts=True, sums=True, groups=lab)
    gm = core.moments(VAR, (m0, m1), weights=w, against=pred, groups=lab)
    for g in range(G):
        wm = np.where(lab == g, w, 0.0)
        a, na = core.quantiles(VAR, probs, (y0, y1), weights=wm, counts=True)
        assert np.array_equal(a, gq[g], equal_nan=True) and np.array_equal(na, gn[g]), (n, g)
        ra = core.probabilities(VAR, pe.EDGE_SETS[2], (y0, y1), weights=wm, counts=True, sums=True)
        assert all(np.array_equal(p, s[g], equal_nan=True) for p, s in zip(ra, gp)), (n, g)
        ma = core.moments(VAR, (m0, m1), weights=wm, against=pred)
        within_bound(ma, gm[g], (n, g))
        assert np.array_equal(ma.pshift, gm.pshift[g])


def test_metric_rows_behind_a_full_chunk(row_core):
    """The metric block is a second source of the grouped kernels, with its own row stride."""
    n = 8193
    core, r = row_core(n)
    lab, G = labels(n, "contiguous")
    specs = [Metric("mean", pe.year_of(k)) for k in pe.MOMENT_ROWS] + [Metric("max", _years(pe.PART1_ROWS[:3]))]
    m = core.metrics(VAR, specs)
    w = pe.weight_settings(n)["wide"]
    q = pe.q_of(n, w)
    probs = pe.probs_for(5)
    got, npart = core.metric_quantiles(VAR, specs, probs, weights=w, counts=True, groups=(lab, G))
    check_group_quantiles(m, got, npart, q, lab, G, probs, ("metric", n))
    res = core.metric_probabilities(VAR, specs, pe.EDGE_SETS[1], weights=w, counts=True, sums=True, groups=(lab, G))
    check_group_bins(m, res, q, lab, G, pe.EDGE_SETS[1], ("metric", n))
    pred = pe.predictors(n)[:3]
    gm = core.metric_moments(VAR, specs, weights=w, against=[p for p in pred], groups=(lab, G))
    check_group_moments(gm, m, q, lab, G, pred, ("metric", n))


# ---- a real run: member sorting on, labels from a parameter ------------------------------------------

def test_a_sorted_run_with_terciles_of_the_sensitivity(hip_lib):
    n = 2048
    core = hector_amd.Core(SCENARIO, n, lib_path=hip_lib)
    S, q10 = ensemble.ecs_q10(n)
    beta = 0.2 + 0.6 * np.fmod(np.arange(n) * 0.7548776662466927, 1.0)
    core.setvar("S", S, "degC").setvar("q10_rh", q10).setvar("beta", beta)
    core.set_member_sorting(True)
    core.run(2100)
    assert not np.array_equal(core.lane_of_member(), np.arange(n))   # a member / lane mix-up cannot pass
    lab = np.searchsorted(np.quantile(S, [1 / 3, 2 / 3]), S, side="right").astype(np.int32)
    G = 3
    assert set(lab) == {0, 1, 2}
    rng = np.random.default_rng(8)
    w = rng.random(n) ** 6
    x = core.fetchvars(VAR, (1850, 2100))
    probs = (0.05, 0.5, 0.95)
    for weights in (None, w):
        q = pe.q_of(n, weights)
        got, npart = core.quantiles(VAR, probs, (1850, 2100), weights=weights, counts=True, groups=lab)
        check_group_quantiles(x, got, npart, q, lab, G, probs, ("run", weights is not None))
        edges = np.array([0.5, 1.5, 2.0])
        res = core.probabilities(VAR, edges, (1850, 2100), weights=weights, counts=True, sums=True, groups=lab)
        check_group_bins(x, res, q, lab, G, edges, ("run", weights is not None))
    # metrics: the peak, and the year a level is first reached (members that never reach it: NaN)
    peak = core.metrics(VAR, [Metric("max", (1850, 2100))])[0]
    specs = [Metric("max", (1850, 2100)), Metric("first_ge", (1850, 2100), threshold=float(np.median(peak)))]
    m = core.metrics(VAR, specs)
    assert np.isnan(m[1]).any() and not np.isnan(m[1]).all()
    q = pe.q_of(n, w)
    got, npart = core.metric_quantiles(VAR, specs, probs, weights=w, counts=True, groups=lab)
    check_group_quantiles(m, got, npart, q, lab, G, probs, "run metrics")
    medges = np.array([1.5, 2.0, 2050.0])
    res = core.metric_probabilities(VAR, specs, medges, weights=w, counts=True, sums=True, groups=lab)
    check_group_bins(m, res, q, lab, G, medges, "run metrics")
    pred = np.stack([q10, beta])
    gm = core.metric_moments(VAR, specs, weights=w, against=["q10_rh", "beta"], groups=lab)
    assert np.array_equal(pred, np.stack([core.getvar("q10_rh"), core.getvar("beta")]))
    check_group_moments(gm, m, q, lab, G, pred, ("run metrics",))
    # eta2 of the 2100 warming by tercile of S, against numpy in longdouble
    gm = core.moments(VAR, (2100, 2100), weights=w, groups=lab)
    refs = check_group_moments(gm, x[-1:], q, lab, G, np.zeros((0, n)), ("run 2100",))
    on = q > 0
    wl, xl = q[on].astype(LD), x[-1, on].astype(LD)
    W = wl.sum()
    mean = (wl * xl).sum() / W
    var = (wl * (xl - mean) ** 2).sum() / W
    between, kappa = LD(0), 0.0
    c = min(ref["shift"][0] for ref in refs)
    second = LD(0)
    for g in range(G):
        og = on & (lab == g)
        wg, xg = q[og].astype(LD), x[-1, og].astype(LD)
        mg = (wg * xg).sum() / wg.sum()
        vg = (wg * (xg - mg) ** 2).sum() / wg.sum()
        between += wg.sum() / W * (mg - mean) ** 2
        second += wg.sum() / W * (mg - LD(c)) ** 2
        kappa = max(kappa, float((refs[g]["sums"][0, 1] / wg.sum()) / vg))
    kappa = max(kappa, float(second / between))
    eta2 = between / var
    tol = 4.0 * kappa * (int(gm.n_part.sum()) + 8) * U
    print("eta2 %.6f (reference %.6f), kappa %.4g, tolerance %.3g" % (gm.eta2[0], float(eta2), kappa, tol))
    assert kappa <= KAPPA_MAX
    assert abs(LD(gm.eta2[0]) - eta2) <= tol * eta2
    assert 0.5 < gm.eta2[0] < 1.0     # the sensitivity dominates the 2100 warming
    assert abs(LD(gm.pooled_var[0]) - var) <= tol * var
    core.shutdown()


# ---- shards ------------------------------------------------------------------------------------------

def _write_row_sharded(core, var, year, values, pad_value):
    """_write_row for a core of several shards: every shard's block has its own lanes and padding."""
    lane = core.lane_of_member()
    offsets = core.shards()[1]
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    for s, (a, b) in enumerate(zip(offsets, offsets[1:])):
        ptr, npad = core.device_var_shard(s, var)
        row = np.full(npad, pad_value)
        row[lane[a:b]] = values[a:b]
        dst = ptr + (year - core.strtdate) * npad * 8
        assert hip.hipMemcpy(ctypes.c_void_p(dst), row.ctypes.data_as(ctypes.c_void_p), npad * 8, 1) == 0


@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_row_core_against_one_core(row_core, hip_lib, monkeypatch, shards):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    n = 12289
    one, r = row_core(n)
    many = _new_core(n, hip_lib, devices=[0] * shards)
    many.set_member_sorting(False)
    many.run(pe.RUN_TO)
    assert len(many.shards()[1]) == shards + 1
    for k, name in enumerate(pe.ALL_ROWS):
        _write_row_sharded(many, VAR, pe.year_of(name), r[name], pad_value=pe.pad_value(k))
    y0, y1 = _years(pe.ALL_ROWS)
    m0, m1 = _years(pe.MOMENT_ROWS)
    x = pe.matrix(r, pe.ALL_ROWS)
    assert np.array_equal(many.fetchvars(VAR, (y0, y1)).view(np.uint64), x.view(np.uint64))
    xm = pe.matrix(r, pe.MOMENT_ROWS)
    pred = pe.predictors(n)[:3]
    w = pe.weight_settings(n)["wide"]
    q = pe.q_of(n, w)
    spec = [Metric("mean", pe.year_of(k)) for k in pe.PART1_ROWS]
    for pattern in ("contiguous", "random16"):
        lab, G = labels(n, pattern)
        what = (shards, pattern)
        a, na = one.quantiles(VAR, pe.probs_for(5), (y0, y1), weights=w, counts=True, groups=(lab, G))
        b, nb = many.quantiles(VAR, pe.probs_for(5), (y0, y1), weights=w, counts=True, groups=(lab, G))
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(na, nb), what
        check_group_quantiles(x, b, nb, q, lab, G, pe.probs_for(5), what)
        a, na = one.metric_quantiles(VAR, spec, pe.probs_for(16), counts=True, groups=(lab, G))
        b, nb = many.metric_quantiles(VAR, spec, pe.probs_for(16), counts=True, groups=(lab, G))
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(na, nb), what
        ra = one.probabilities(VAR, pe.EDGE_SETS[1], (y0, y1), weights=w, counts=True, sums=True, groups=(lab, G))
        rb = many.probabilities(VAR, pe.EDGE_SETS[1], (y0, y1), weights=w, counts=True, sums=True, groups=(lab, G))
        assert all(np.array_equal(p, s, equal_nan=True) for p, s in zip(ra, rb)), what
        check_group_bins(x, rb, q, lab, G, pe.EDGE_SETS[1], what)
        ma = one.moments(VAR, (m0, m1), weights=w, against=[p for p in pred], groups=(lab, G))
        mb = many.moments(VAR, (m0, m1), weights=w, against=[p for p in pred], groups=(lab, G))
        assert np.array_equal(ma.pshift, mb.pshift, equal_nan=True), what
        for g in range(G):
            within_bound(ma[g], mb[g], what + (g,))     # n_part, wsum and shift equal, the sums within the bound
        check_group_moments(mb, xm, q, lab, G, pred, what)
        again = many.moments(VAR, (m0, m1), weights=w, against=[p for p in pred], groups=(lab, G))
        assert same_bits(mb, again), what
    many.shutdown()


# ---- errors raised by the library --------------------------------------------------------------------

def test_the_librarys_errors_by_text_and_nothing_changes(row_core):
    n = 257
    core, r = row_core(n)
    before = core.fetchvars(VAR, (1745, pe.RUN_TO))
    lab, G = labels(n, "mod3")
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    lib, h = core._lib, core._h
    probs = np.array([0.5])
    out = np.full((16 * 46,), 7.0)

    def raw_q(labels_, ngroups):
        lp = None if labels_ is None else np.ascontiguousarray(labels_, dtype=np.int32).ctypes.data_as(ip)
        rc = lib.hx_group_quantiles(h, VAR.encode(), 1745, pe.RUN_TO, None, 0, lp, ngroups, None,
                                    probs.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), None)
        return rc, lib.hx_last_error().decode()

    # (the binding raises these itself: the library's own texts through the C ABI)
    for labels_, ngroups, text in ((None, 3, "hx_group_quantiles: labels is NULL"),
                                   (lab, 17, "hx_group_quantiles: ngroups must lie in 1..16"),
                                   (lab, 0, "hx_group_quantiles: ngroups must lie in 1..16"),
                                   (lab, 2, "hx_group_quantiles: label 2 of member 2 lies outside -1..1"),
                                   (np.where(np.arange(n) == 5, -2, lab), 3,
                                    "hx_group_quantiles: label -2 of member 5 lies outside -1..2"),
                                   (np.full(n, -1), 3, "hx_group_quantiles: no member has a label >= 0")):
        rc, msg = raw_q(labels_, ngroups)
        assert rc != 0 and msg == text, (msg, text)
    assert (out == 7.0).all()     # a refused call changes nothing
    # the ungrouped verbs' errors, passed through under the grouped name
    for call, text in (
            (lambda: core.quantiles(VAR, [1.5], groups=lab), "hx_group_quantiles: a probability outside [0, 1]"),
            (lambda: core.quantiles(VAR, np.linspace(0, 1, 17), groups=lab), "hx_group_quantiles: nprobs must lie in 1..16"),
            (lambda: core.quantiles(VAR, [0.5], (1745, 1791), groups=lab),
             "hx_group_quantiles: dates must lie between startDate and the current date"),
            (lambda: core.quantiles(VAR, [0.5], weights=np.zeros(n), groups=lab), "hx_group_quantiles: the weights are all zero"),
            (lambda: core.quantiles("RF_tot", [0.5], groups=lab),
             "hx_group_quantiles: variable RF_tot was not enabled with set_outputs()"),
            (lambda: core.probabilities(VAR, [1.0, 0.5], groups=lab), "hx_group_probabilities: the edges are not strictly ascending"),
            (lambda: core.probabilities(VAR, np.arange(32.0), groups=lab), "hx_group_probabilities: nedges must lie in 1..31"),
            (lambda: core.probabilities(VAR, [0.5], weights=np.where(np.arange(n) == 3, -1.0, 1.0), groups=lab),
             "hx_group_probabilities: a weight is negative, NaN or infinite"),
            (lambda: core.metric_probabilities(VAR, [Metric("mean", (1700, 1750))], [0.5], groups=lab),
             "hx_group_probabilities: the window must lie between startDate and the current date (specification 0)"),
            (lambda: core.moments(VAR, (1745, 1795), groups=lab),
             "hx_group_moments: dates must lie between startDate and the current date"),
            (lambda: core.metric_moments(VAR, [Metric("first_ge", (1750, 1760), threshold=float("nan"))], groups=lab),
             "hx_group_moments: the threshold is NaN (specification 0)")):
        with pytest.raises(E) as err:
            call()
        assert str(err.value) == text, (str(err.value), text)
    assert np.array_equal(before, core.fetchvars(VAR, (1745, pe.RUN_TO)), equal_nan=True)
    assert (core.status() == 0).all()
    got = core.quantiles(VAR, [0.5], groups=lab)      # ... and the core goes on
    assert got.shape == (3, pe.RUN_TO - 1745 + 1, 1)
