"""The summary kernels of hector_amd/csrc/hx_dev_post.h at their chunk, batch and template edges.

The shapes of the other GPU suites come from the workload: exact multiples of the workgroup chunk
(65 536, 131 072) or one partial chunk.  Here they come from the kernel constants
(tests/post_edge_cases.py): 8191 / 8192 / 8193, ragged last chunks behind full ones, the chunk
remainders at which a register batch of the moments kernel ends, all nine predictor counts, both
arms of HECTOR_AMD_POST_AB, ragged multi-chunk shards, and the series / score / metric kernels on
+-inf, NaN, +-0.0, denormals and 1e+-300.

Rows are synthetic: a core runs to 1790 (46 recorded rows) and the rows are written through the
device pointer of Core.device_var (`_write_row` of tests/test_gpu_quantiles.py); the padding lanes
n..npad-1 get poison, alternately NaN and -1e300.  The cores run without member sorting, so that
member order is lane order and 'the last chunk' of a generated row is the last workgroup's.

The authorities are the project's own checkers, imported: `checker` / `check_rows` of
tests/test_gpu_quantiles.py, `bin_reference` / `check_bin_rows` of
tests/test_gpu_metrics_probabilities.py, `checker` / `check_raw` / `within_bound` of
tests/test_gpu_moments.py, `numpy_series` / `numpy_score` of tests/test_device_series.py and
`numpy_metric` of tests/test_member_metrics.py; tests/test_post_edge_checkers.py holds them to brute
force on the same rows.

Moments: the header's bound |S - S_ref| <= (n_part + 8) 2^-53 S_ref assumes that no term underflows
or overflows.  That is a condition on the input, not a tolerance: the rows of the moments parts are
chosen so that every reference term q d, q d d, q e, q e e, q d e is exactly 0 or a normal double, and
`terms_zero_or_normal` asserts it on the checker's own terms before anything is compared.  Rows with
+-inf, denormal spreads or 1e+-300 (INTEGER_ONLY_ROWS) are therefore left out of the moments and stay
in the quantile and bin parts, whose arithmetic is integer.
"""
import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import SCENARIO

import post_edge_cases as pe
from test_gpu_quantiles import _write_row, check_rows
from test_gpu_metrics_probabilities import check_bin_rows
from test_gpu_moments import check_raw, checker as moments_checker, same_bits as same_moment_bits, within_bound
from test_device_series import numpy_score, numpy_series
from test_member_metrics import OPS, numpy_metric

pytestmark = pytest.mark.gpu

VAR = "global_tas"
LD = np.longdouble
U = 2.0 ** -53
_cores = {}
_worst = {"ratio": 0.0, "what": None}


def _new_core(n, hip_lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def _row_core(n, hip_lib):
    """A fresh core of n members with pe.rows(n) written from 1750 on -> (core, rows)."""
    c = _new_core(n, hip_lib)
    c.set_member_sorting(False)
    c.run(pe.RUN_TO)
    assert np.array_equal(c.lane_of_member(), np.arange(n))
    assert c.device_var(VAR)[1] == pe.npad_of(n)
    r = pe.rows(n)
    assert tuple(r) == pe.ALL_ROWS
    for k, name in enumerate(pe.ALL_ROWS):
        _write_row(c, VAR, pe.year_of(name), r[name], pad_value=pe.pad_value(k))
    x = c.fetchvars(VAR, (pe.FIRST_ROW_YEAR, pe.FIRST_ROW_YEAR + len(pe.ALL_ROWS) - 1))
    assert np.array_equal(x.view(np.uint64), pe.matrix(r, pe.ALL_ROWS).view(np.uint64))   # bit for bit
    return c, r


@pytest.fixture(scope="module")
def row_core(hip_lib):
    """n -> (core, rows), one core a size for the whole module."""
    def get(n):
        if n not in _cores:
            _cores[n] = _row_core(n, hip_lib)
        return _cores[n]
    yield get
    for c, _ in _cores.values():
        c.shutdown()
    _cores.clear()
    print("worst sum error / bound over the edge shapes: %.3g at %r" % (_worst["ratio"], _worst["what"]))


def _years(names):
    """The rows `names` are adjacent in pe.ALL_ROWS -> (year0, year1)."""
    ys = [pe.year_of(k) for k in names]
    assert ys == list(range(ys[0], ys[0] + len(ys)))
    return ys[0], ys[-1]


def test_the_size_set_has_cores_with_and_without_padding_lanes():
    pads = [pe.npad_of(n) - n for n in pe.SIZES]
    assert any(p > 0 for p in pads) and any(p == 0 for p in pads)
    assert {pe.nprobs_of(n) for n in pe.SIZES} == set(range(1, 17))
    for k in range(1, 17):
        assert len(pe.probs_for(k)) == k and (k == 1 or (0.0 in pe.probs_for(k) and 1.0 in pe.probs_for(k)))
    covered = {k for n in pe.SIZES for k in pe.npred_for(n)}
    assert covered == set(range(9))
    for n in pe.SIZES:
        ks = pe.npred_for(n)
        assert 0 in ks and any(1 <= k <= 3 for k in ks) and any(4 <= k <= 8 for k in ks)   # batches of 32, 16, 8
    for n in pe.ALL_PREDICTOR_SIZES:
        assert pe.npred_for(n) == tuple(range(9))
    assert [len(e) for e in pe.EDGE_SETS] == [1, 7, 31]


# ---- 1. member counts chosen from the kernel constants ---------------------------------------------

@pytest.mark.parametrize("n", pe.SIZES)
def test_quantiles_at_the_chunk_edges(row_core, n):
    core, r = row_core(n)
    probs = pe.probs_for(pe.nprobs_of(n))
    y0, y1 = _years(pe.ALL_ROWS)
    x = pe.matrix(r, pe.ALL_ROWS)
    for wname, w in pe.weight_settings(n).items():
        if wname == "wide" and n > 1:
            assert (pe.quantise(w) == 0).any()
        got, npart = core.quantiles(VAR, probs, (y0, y1), weights=w, counts=True)
        assert got.shape == (len(pe.ALL_ROWS), len(probs))
        check_rows(x, got, npart, w, probs, (n, wname))
    # the written rows next to the untouched model rows around them, in one call
    xa = core.fetchvars(VAR, (1745, pe.RUN_TO))
    got, npart = core.quantiles(VAR, probs, weights=pe.weight_settings(n)["wide"], counts=True)
    check_rows(xa, got, npart, pe.weight_settings(n)["wide"], probs, (n, "all rows"))


@pytest.mark.parametrize("n", pe.SIZES)
def test_probabilities_at_the_chunk_edges(row_core, n):
    core, r = row_core(n)
    y0, y1 = _years(pe.ALL_ROWS)
    x = pe.matrix(r, pe.ALL_ROWS)
    on_edge = 0
    for edges in pe.EDGE_SETS:
        on_edge += int(np.isin(x, edges).sum())
        for wname, w in pe.weight_settings(n).items():
            res = core.probabilities(VAR, edges, (y0, y1), weights=w, counts=True, sums=True)
            check_bin_rows(x, res, w, edges, (n, wname, len(edges)))
    assert on_edge > 0    # members exactly on edges: they lie in the upper bin


def _moment_ratio(m, ref):
    s = ref["sums"]
    bound = (ref["n_part"].astype(LD)[:, None] + 8) * LD(U) * s
    err = np.abs(m.sums.astype(LD) - s)
    return float(np.max(np.where(s > 0, err / np.where(s > 0, bound, 1), 0)))


def _check_moments(call, x, n, w, pred, what):
    """The normal-range condition on the checker's own terms, then check_raw, then the same bits
    from a second identical call -> the checker's record."""
    q = pe.q_of(n, w)
    ref = moments_checker(x, q, pred)
    assert pe.terms_zero_or_normal(x, q, pred, ref) > 0 or ref["n_part"].sum() == 0
    m = call()
    check_raw(m, x, q, pred, what)
    ratio = _moment_ratio(m, ref)
    if ratio > _worst["ratio"]:
        _worst["ratio"], _worst["what"] = ratio, what
    assert same_moment_bits(m, call()), what
    return ref


@pytest.mark.parametrize("n", pe.SIZES)
def test_moments_at_the_chunk_and_batch_edges(row_core, n):
    core, r = row_core(n)
    y0, y1 = _years(pe.PART1_ROWS)
    x = pe.matrix(r, pe.PART1_ROWS)
    allp = pe.predictors(n)
    nobody = 0
    for k in pe.npred_for(n):
        pred = allp[:k]
        against = [p for p in pred] if k else None
        for wname, w in pe.weight_settings(n).items():
            ref = _check_moments(lambda: core.moments(VAR, (y0, y1), weights=w, against=against), x, n, w, pred,
                                 (n, "npred", k, wname))
            nobody += int((ref["n_part"] == 0).sum())
    if n > 1:
        assert nobody > 0   # rows nobody takes part in (check_raw: shift NaN, sums 0, W 0)


@pytest.mark.parametrize("n", pe.METRIC_SIZES)
def test_metric_verbs_behind_full_chunks(row_core, n):
    """The metric block is a second source of the cooperative kernels, with its own row stride."""
    core, r = row_core(n)
    specs = [Metric("mean", pe.year_of(k)) for k in pe.ALL_ROWS] + \
            [Metric("min", _years(pe.PART1_ROWS[:3])), Metric("slope", _years(pe.PART1_ROWS[:3])),
             Metric("year_of_max", _years(pe.PART1_ROWS[:3])), Metric("count_ge", _years(pe.PART1_ROWS[:3]), threshold=1.0),
             Metric("mean", (1745, 1749))]
    xa = core.fetchvars(VAR, (1745, pe.RUN_TO))
    m = core.metrics(VAR, specs)
    for k, s in enumerate(specs):
        with np.errstate(all="ignore"):
            ref = numpy_metric(xa, 1745, s)
        assert np.array_equal(m[k], ref, equal_nan=True), (n, s)
    probs = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
    mom_rows = [i for i, k in enumerate(pe.ALL_ROWS) if k in pe.MOMENT_ROWS] + list(range(len(pe.ALL_ROWS), len(specs)))
    mom_specs = [specs[i] for i in mom_rows]
    pred = pe.predictors(n)[:5]
    for wname, w in pe.weight_settings(n).items():
        got, npart = core.metric_quantiles(VAR, specs, probs, weights=w, counts=True)
        check_rows(m, got, npart, w, probs, (n, "metric", wname))
        for edges in pe.EDGE_SETS:
            res = core.metric_probabilities(VAR, specs, edges, weights=w, counts=True, sums=True)
            check_bin_rows(m, res, w, edges, (n, "metric", wname, len(edges)))
        for k in (0, 2, 5):
            against = [p for p in pred[:k]] if k else None
            _check_moments(lambda: core.metric_moments(VAR, mom_specs, weights=w, against=against), m[mom_rows], n, w,
                           pred[:k], (n, "metric_moments", k, wname))


# ---- 2. the moments on hostile rows ----------------------------------------------------------------

@pytest.mark.parametrize("n", pe.HOSTILE_SIZES)
def test_moments_on_hostile_rows(row_core, n):
    core, r = row_core(n)
    y0, y1 = _years(pe.HOSTILE_MOMENT_ROWS)
    x = pe.matrix(r, pe.HOSTILE_MOMENT_ROWS)
    allp = pe.predictors(n)
    for k in (0, 3, 8):
        pred = allp[:k]
        against = [p for p in pred] if k else None
        for wname, w in pe.weight_settings(n).items():
            ref = _check_moments(lambda: core.moments(VAR, (y0, y1), weights=w, against=against), x, n, w, pred,
                                 (n, "hostile", k, wname))
            all_nan = pe.HOSTILE_MOMENT_ROWS.index("all NaN")
            assert ref["n_part"][all_nan] == 0
    # every moment row of the core in one call, the model's own rows before them included
    xa = core.fetchvars(VAR, (1745, _years(pe.MOMENT_ROWS)[1]))
    w = pe.weight_settings(n)["wide"]
    _check_moments(lambda: core.moments(VAR, (1745, _years(pe.MOMENT_ROWS)[1]), weights=w, against=[allp[1], allp[6]]),
                   xa, n, w, allp[[1, 6]], (n, "all moment rows"))


# ---- 3. the arms of HECTOR_AMD_POST_AB ------------------------------------------------------------

@pytest.mark.parametrize("n", pe.AB_SIZES)
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_select_arms_give_the_same_exact_answers(hip_lib, monkeypatch, flags, n):
    """1: every select starts at bit 63; 2: the wave-aggregated LDS add of hxq_add (ballot, shuffle,
    leader atomics; weighted through __shfl_xor, unweighted through a popcount); 3: both.  The
    library reads the variable on each call; a core of its own, so that no other test inherits it."""
    core, r = _row_core(n, hip_lib)
    x = pe.matrix(r, pe.ALL_ROWS)
    y0, y1 = _years(pe.ALL_ROWS)
    probs = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
    specs = [Metric("mean", pe.year_of(k)) for k in pe.ALL_ROWS]
    plain = {}
    for wname in ("none", "wide"):
        w = pe.weight_settings(n)[wname]
        plain[wname] = core.quantiles(VAR, probs, (y0, y1), weights=w)
    monkeypatch.setenv("HECTOR_AMD_POST_AB", str(flags))
    m = core.metrics(VAR, specs)
    for wname in ("none", "wide"):
        w = pe.weight_settings(n)[wname]
        got, npart = core.quantiles(VAR, probs, (y0, y1), weights=w, counts=True)
        check_rows(x, got, npart, w, probs, (n, flags, wname))
        assert np.array_equal(got, plain[wname], equal_nan=True)
        got, npart = core.metric_quantiles(VAR, specs, probs, weights=w, counts=True)
        check_rows(m, got, npart, w, probs, (n, flags, "metric", wname))
    core.shutdown()


# ---- 4. sharded cores whose shards are ragged multi-chunk -------------------------------------------

def test_ragged_multi_chunk_shards_equal_one_core(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    n = 2 * 8449 + 5
    one, many = _new_core(n, hip_lib), _new_core(n, hip_lib, devices=[0] * 2)
    for c in (one, many):
        c.set_pair_kernel_limit(0)
        c.run(pe.RUN_TO, wait=False)
    offsets = many.shards()[1]
    assert len(offsets) == 3 and all(b - a > pe.CHUNK and (b - a) % pe.CHUNK for a, b in zip(offsets, offsets[1:]))
    rng = np.random.default_rng(2)
    w = rng.random(n) ** 12
    w[:offsets[1]] = 0.0               # the whole first shard takes no part
    w[n - 1] = 5.0                     # the largest weight lives on the last shard
    probs = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
    pred = pe.predictors(n)[:3]
    for var in ("global_tas", "CO2_concentration"):
        x = one.fetchvars(var, (1745, pe.RUN_TO))
        assert np.array_equal(x, many.fetchvars(var, (1745, pe.RUN_TO)))
        edges = tuple(sorted(set(np.quantile(x[-1], [0.2, 0.5, 0.9])) | {float(x[-1][n - 1])}))
        for weights in (None, w):
            what = (var, weights is not None)
            a, na = one.quantiles(var, probs, weights=weights, counts=True)
            b, nb = many.quantiles(var, probs, weights=weights, counts=True)
            assert np.array_equal(a, b) and np.array_equal(na, nb), what
            check_rows(x, b, nb, weights, probs, what)
            ra = one.probabilities(var, edges, weights=weights, counts=True, sums=True)
            rb = many.probabilities(var, edges, weights=weights, counts=True, sums=True)
            assert all(np.array_equal(p, s, equal_nan=True) for p, s in zip(ra, rb)), what
            check_bin_rows(x, rb, weights, edges, what)
            for k in (0, 3):
                against = [p for p in pred[:k]] if k else None
                ma = one.moments(var, weights=weights, against=against)
                mb = many.moments(var, weights=weights, against=against)
                within_bound(ma, mb, what)     # n_part, wsum and shift equal, the sums within the bound
                q = pe.q_of(n, weights)
                ref = moments_checker(x, q, pred[:k])
                pe.terms_zero_or_normal(x, q, pred[:k], ref)
                check_raw(ma, x, q, pred[:k], ("one",) + what)
                check_raw(mb, x, q, pred[:k], ("many",) + what)
                assert same_moment_bits(mb, many.moments(var, weights=weights, against=against)), what
    one.shutdown(); many.shutdown()


# ---- 5. series, score and metric kernels on hostile content -----------------------------------------

@pytest.mark.parametrize("n", pe.SERIES_SIZES)
def test_series_score_and_metrics_on_hostile_content(hip_lib, n):
    core = _new_core(n, hip_lib)
    core.run(pe.RUN_TO)
    y0, ny = core.strtdate, pe.RUN_TO - core.strtdate + 1
    assert y0 == 1745
    blocks = {VAR: pe.hostile_block(n, 11), "CO2_concentration": pe.hostile_block(n, 12)}
    for var, blk in blocks.items():
        for k in range(ny):
            _write_row(core, var, y0 + k, blk[k], pad_value=pe.pad_value(k))
    x = {v: core.fetchvars(v, (y0, pe.RUN_TO)) for v in blocks}
    for v in blocks:
        pe.same_bits(x[v], blocks[v], ("written", v))
    a, b = x[VAR], x["CO2_concentration"]
    for special in (np.inf, -np.inf, 0.0, pe.TINY, 1e300):
        assert (a == special).any() and (b == special).any()
    assert (np.signbit(b) & (b == 0)).any() and np.isnan(a).any()
    assert (np.isinf(a) & np.isinf(b) & (a == b)).any()      # sub of inf from inf
    assert ((b == 0) & (a == 0)).any() and ((b == 0) & (a != 0) & ~np.isnan(a)).any()   # 0 / 0 and x / +-0

    def run(what, op, operand=None, ref_b=None, **kw):
        core.derive("z", op, VAR, operand, **kw)
        got = core.fetchvars("z", (y0, pe.RUN_TO))
        with np.errstate(all="ignore"):
            ref = numpy_series(op, a, operand if ref_b is None else ref_b, y0=y0, **kw)
        pe.same_bits(got, ref, (n, what, op, kw))

    core.hold("held", VAR)
    pe.same_bits(core.fetchvars("held", (y0, pe.RUN_TO)), a, (n, "hold"))
    whole, inside = pe.hostile_vector(ny, 21), pe.hostile_vector(20, 22)
    for op in ("add", "sub", "mul", "div"):
        for c in (1.5, 0.0, -0.0, np.inf, pe.TINY, 1.0 / 3.0, -1e300):
            run("scalar %r" % c, op, c)
        run("vector", op, whole, first_year=y0)
        run("vector inside", op, inside, first_year=y0 + 7)
        run("variable", op, "CO2_concentration", ref_b=b)
    for period in ((1760, 1770), (y0, y0), (y0, pe.RUN_TO)):
        run("anomaly", "anomaly", years=period)
    for first in (y0 + 5, y0 + 17, pe.RUN_TO):       # not multiples of 16 from startDate
        core.derive("z", "cumsum", VAR, years=first)
        with np.errstate(all="ignore"):
            ref = numpy_series("cumsum", a, y0=y0, years=first)
        pe.same_bits(core.fetchvars("z", (y0, pe.RUN_TO)), ref, (n, "cumsum", first))
    for w in (1, 16, 17, 33):
        for align in ("trailing", "centred"):
            run("runmean", "runmean", width=w, align=align)
    for lag in (1, 7, ny - 1):
        run("delta", "delta", lag=lag)
    # score, with and without sigma and baseline
    rng = np.random.default_rng(7)
    years = np.arange(1750, 1786)
    rng.shuffle(years)
    obs = rng.normal(0, 1, years.size)
    obs[::9] = np.nan
    sig = 0.05 + 0.1 * rng.random(years.size)
    for var in (VAR, "held"):
        for sigma in (None, sig):
            for baseline in (None, (1760, 1775)):
                with np.errstate(all="ignore"):
                    ref = numpy_score(a, y0, years, obs, sigma, baseline)
                assert np.array_equal(core.score(var, years, obs, sigma=sigma, baseline=baseline), ref,
                                      equal_nan=True), (n, var, sigma is not None, baseline)
    # metrics: every operation, windows of one batch + 1 and of the whole record
    specs = [Metric(op, win, baseline=base, threshold=0.25) for op in OPS
             for win, base in (((1750, 1766), None), ((y0, pe.RUN_TO), (1760, 1762)), ((1771, 1771), None))]
    for lo in range(0, len(specs), 32):
        got = core.metrics(VAR, specs[lo:lo + 32])
        for k, s in enumerate(specs[lo:lo + 32]):
            with np.errstate(all="ignore"):
                ref = numpy_metric(a, y0, s)
            assert np.array_equal(got[k], ref, equal_nan=True), (n, s)
    core.shutdown()
