"""Core.pair_metrics and its ensemble-wide siblings (pair_metric_quantiles, pair_metric_probabilities,
pair_metric_moments) on the GPU.

Authorities, all numpy on the host:
  * `numpy_pair_metric` (tests/test_member_pair_metrics.py): the header's sequence, compared bit for bit;
  * `checker` / `bin_reference` (tests/test_gpu_metrics_probabilities.py) and the moments checker
    (tests/test_gpu_moments.py), applied to the rows Core.pair_metrics() returns: integer results with
    `==`, the floating sums within the header's (n_part + 8) 2^-53 bound.
"""
import importlib.util
import os

import numpy as np
import pytest

import hector_amd
from hector_amd import PairMetric
from conftest import ROOT
from test_member_pair_metrics import OPS, BATCH, VAR_A, VAR_B, _params, numpy_pair_metric
from test_gpu_metrics_probabilities import check_bin_rows, check_quantile_rows, quantise, _write_row
from test_gpu_moments import check_raw, same_bits

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
Y0, END = 1745, 1900
BASE = (1850, 1870)
FLAVOURS = {"pair": (32768, 0), "run": (0, 0), "run2": (0, 1)}   # set_pair_kernel_limit, set_two_wave_from


def _core(n, hip_lib, flavour="pair", **kw):
    c = hector_amd.Core(n_members=n, lib_path=hip_lib, **kw)
    S, q10, beta = _params(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10).setvar("beta", beta)
    limit, two_wave = FLAVOURS[flavour]
    c.set_pair_kernel_limit(limit)
    c.set_two_wave_from(two_wave)
    return c


def _specs(xb, y1=END):
    """Every op over the record with both reference periods, a threshold from numpy that some members
    reach and some do not, and windows around the kernel's batch."""
    b = xb[1871 - Y0:y1 - Y0 + 1] - xb[BASE[0] - Y0:BASE[1] - Y0 + 1].mean(axis=0)
    thr = float(np.median(b.max(axis=0)))
    specs = [PairMetric(op, (1871, y1), baseline=BASE, baseline_b=BASE, threshold=thr) for op in OPS]
    specs += [PairMetric(OPS[k % 8], (1800 + k, 1800 + k + length - 1), baseline=None if k % 2 else (Y0, Y0 + k),
                         baseline_b=None if k % 3 else (y1 - k, y1), threshold=float(np.median(xb[1820 - Y0])))
              for k, length in enumerate((1, 2, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1, 3 * BATCH, 40))]
    return specs


def _vector():
    years = np.arange(Y0 - 3, END + 1)
    return years, np.cumsum(0.05 + 0.01 * (years - years[0]).astype(float))


def _check_rows(got, xa, xb, specs, what):
    assert got.shape == (len(specs), xa.shape[1])
    for k, m in enumerate(specs):
        ref = numpy_pair_metric(xa, xb, Y0, m)
        assert np.array_equal(got[k], ref, equal_nan=True), (what, m)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_member_counts_on_every_year_loop_flavour(hip_lib, flavour):
    """1, 63, 64, 65, 257 and 1 024 members: the wavefront and workgroup edges, where an unwritten or
    overwritten lane would show.  The operands are also read from held series whose padding lanes hold
    1e300 or NaN in every row."""
    vy, vv = _vector()
    for n in (1, 63, 64, 65, 257, 1024):
        core = _core(n, hip_lib, flavour)
        core.run(END)
        assert core.last_run_kernel() == flavour
        xa, xb = core.fetchvars(VAR_A, (Y0, END)), core.fetchvars(VAR_B, (Y0, END))
        specs = _specs(xb)
        assert len(specs) == 16
        _check_rows(core.pair_metrics(VAR_A, VAR_B, specs), xa, xb, specs, (flavour, n))
        vb = np.repeat(vv[3:, None], n, axis=1)
        _check_rows(core.pair_metrics(VAR_A, (vy, vv), specs), xa, vb, specs, (flavour, n, "vector"))
        core.derive("pm_a", "copy", VAR_A).derive("pm_b", "copy", VAR_B)
        for y in range(Y0, END + 1):
            _write_row(core, "pm_a", y, xa[y - Y0], pad_value=1e300)
            _write_row(core, "pm_b", y, xb[y - Y0], pad_value=np.nan if y % 2 else -1e300)
        _check_rows(core.pair_metrics("pm_a", "pm_b", specs), xa, xb, specs, (flavour, n, "hostile padding"))
        # the ensemble-wide verbs see no padding lane either
        w = np.where(np.arange(n) % 3 == 1, 0.0, 1.0 + np.arange(n) % 5) if n > 1 else None
        m = core.pair_metrics("pm_a", "pm_b", specs)
        got, npart = core.pair_metric_quantiles("pm_a", "pm_b", specs, PROBS, weights=w, counts=True)
        check_quantile_rows(m, got, npart, w, PROBS, (flavour, n))
        edges = (float(np.nanmedian(m[0])), float(np.nanmedian(m[0])) + 1.0)
        check_bin_rows(m, core.pair_metric_probabilities("pm_a", "pm_b", specs, edges, weights=w, counts=True, sums=True),
                       w, edges, (flavour, n))
        core.shutdown()


def test_quantiles_probabilities_and_moments_of_pair_metrics(hip_lib):
    n = 1000
    core = _core(n, hip_lib)
    core.run(2100)
    xa, xb = core.fetchvars(VAR_A, (Y0, 2100)), core.fetchvars(VAR_B, (Y0, 2100))
    specs = _specs(xb, 2100)
    vy = np.arange(1850, 2101)
    vec = (vy, np.cumsum(np.linspace(0.5, 12.0, vy.size)))
    vspecs = [PairMetric("slope", (1850, 2100), baseline=(1850, 1900)), PairMetric("r2", (1850, 2100)),
              PairMetric("at_first_ge", (1850, 2100), threshold=800.0), PairMetric("end_ratio", (1850, 2100))]
    rng = np.random.default_rng(7)
    w = rng.random(n) ** 10
    w[rng.integers(0, n, 50)] = 0.0
    assert (quantise(w) == 0).any() and (quantise(w) > 0).sum() > 10
    S, q10, beta = _params(n)
    pred = np.stack([S, q10])
    for a, b, sp in ((VAR_A, VAR_B, specs), (VAR_B, vec, vspecs)):
        m = core.pair_metrics(a, b, sp)
        nan_rows = [k for k in range(len(sp)) if np.isnan(m[k]).any() and not np.isnan(m[k]).all()]
        if isinstance(b, str):
            assert nan_rows    # members whose pair metric is NaN exist: they must not take part
        for weights in (None, w):
            tag = (a, weights is not None)
            got, npart = core.pair_metric_quantiles(a, b, sp, PROBS, weights=weights, counts=True)
            assert got.shape == (len(sp), len(PROBS))
            check_quantile_rows(m, got, npart, weights, PROBS, tag)
            assert np.array_equal(got, core.pair_metric_quantiles(a, b, sp, PROBS, weights=weights), equal_nan=True)
            held = m[0][~np.isnan(m[0])]
            edges = tuple(np.unique(held[[1, held.size // 2, held.size - 2]]))   # values some members sit on
            check_bin_rows(m, core.pair_metric_probabilities(a, b, sp, edges, weights=weights, counts=True, sums=True),
                           weights, edges, tag)
            q = np.ones(n, dtype=np.uint64) if weights is None else quantise(weights)
            mom = core.pair_metric_moments(a, b, sp, weights=weights, against=[S, q10])
            check_raw(mom, m, q, pred, tag)
            assert same_bits(mom, core.pair_metric_moments(a, b, sp, weights=weights, against=["S", "q10_rh"]))
    # a pair metric as a predictor: the triple equals the array passed directly
    tcre = PairMetric("slope", (1850, 2100), baseline=(1850, 1900))
    cross = PairMetric("at_first_ge", (1850, 2100), baseline_b=(1850, 1900), threshold=2.0)
    col_v, col_c = core.pair_metrics(VAR_B, vec, [tcre])[0], core.pair_metrics(VAR_A, VAR_B, [cross])[0]
    assert np.isnan(col_c).any() and np.isfinite(col_c).any()
    for verb, args in ((core.moments, (VAR_B, (2050, 2100))),
                       (core.metric_moments, (VAR_B, [hector_amd.Metric("mean", (2081, 2100))])),
                       (core.pair_metric_moments, (VAR_A, VAR_B, specs[:3]))):
        direct = verb(*args, weights=w, against=[col_v, col_c])
        triples = verb(*args, weights=w, against=[(VAR_B, vec, tcre), (VAR_A, VAR_B, cross)])
        assert same_bits(direct, triples) and np.array_equal(direct.pshift, triples.pshift)
        assert (direct.n_part <= int(np.isfinite(col_c).sum())).all()
    one = core.moments(VAR_B, (2100, 2100), against=(VAR_B, vec, tcre))     # one triple is one entry
    assert same_bits(one, core.moments(VAR_B, (2100, 2100), against=[col_v])) and len(one.names) == 1
    core.shutdown()


@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_core_equals_one_core(hip_lib, monkeypatch, shards):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    n = shards * 512 + 5
    one = _core(n, hip_lib, "run")
    many = _core(n, hip_lib, "run", devices=[0] * shards)
    for c in (one, many):
        c.run(END, wait=False)
    xa, xb = one.fetchvars(VAR_A, (Y0, END)), one.fetchvars(VAR_B, (Y0, END))
    assert np.array_equal(xa, many.fetchvars(VAR_A, (Y0, END))) and np.array_equal(xb, many.fetchvars(VAR_B, (Y0, END)))
    rng = np.random.default_rng(shards)
    w = rng.random(n) ** 12
    w[:700] = 0.0                    # (the whole first shard of eight, and more, left out)
    w[n - 1] = 5.0                   # the largest weight lives on the last shard
    specs = _specs(xb)
    for b, block in ((VAR_B, xb), (_vector(), np.repeat(_vector()[1][3:, None], n, axis=1))):
        m = one.pair_metrics(VAR_A, b, specs)
        _check_rows(m, xa, block, specs, shards)
        assert np.array_equal(m, many.pair_metrics(VAR_A, b, specs), equal_nan=True)
        held = m[0][~np.isnan(m[0])]
        edges = tuple(np.unique(np.quantile(held, [0.2, 0.5, 0.9]))) + (float(m[0][n - 1]),)
        edges = tuple(sorted(set(e for e in edges if np.isfinite(e))))
        for weights in (None, w):
            p, na = one.pair_metric_quantiles(VAR_A, b, specs, PROBS, weights=weights, counts=True)
            q, nb = many.pair_metric_quantiles(VAR_A, b, specs, PROBS, weights=weights, counts=True)
            assert np.array_equal(p, q, equal_nan=True) and np.array_equal(na, nb)
            check_quantile_rows(m, q, nb, weights, PROBS, (shards, weights is not None))
            ra = one.pair_metric_probabilities(VAR_A, b, specs, edges, weights=weights, counts=True, sums=True)
            rb = many.pair_metric_probabilities(VAR_A, b, specs, edges, weights=weights, counts=True, sums=True)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ra, rb))
            check_bin_rows(m, rb, weights, edges, (shards, weights is not None))
            qq = np.ones(n, dtype=np.uint64) if weights is None else quantise(weights)
            check_raw(many.pair_metric_moments(VAR_A, b, specs, weights=weights), m, qq, np.zeros((0, n)),
                      (shards, weights is not None))
    one.shutdown(); many.shutdown()


def test_errors_name_their_function_and_leave_the_core_usable(hip_lib):
    n = 300
    core = _core(n, hip_lib)
    fresh = _core(n, hip_lib)
    E = hector_amd.HectorAmdError
    first = [PairMetric("at_max", Y0)]
    verbs = (("hx_member_pair_metrics", lambda c, a, b, s, **kw: c.pair_metrics(a, b, s)),
             ("hx_pair_metric_quantiles", lambda c, a, b, s, **kw: c.pair_metric_quantiles(a, b, s, [0.5], **kw)),
             ("hx_pair_metric_probabilities", lambda c, a, b, s, **kw: c.pair_metric_probabilities(a, b, s, [1.0], **kw)),
             ("hx_pair_metric_moments", lambda c, a, b, s, **kw: c.pair_metric_moments(a, b, s, **kw)))
    for fn, call in verbs:
        with pytest.raises(E, match=fn + ".*run the core first"):
            call(fresh, VAR_A, VAR_B, first)
    core.run(1850)
    before = core.fetchvars(VAR_A, (Y0, 1850))
    status, ms = core.status(), core.last_run_ms()
    ok = [PairMetric("slope", (1800, 1850))]
    vec = (np.arange(1800, 1851), np.arange(51.0))
    bad = [("not enabled", "RF_tot", VAR_B, ok), ("not enabled", VAR_A, "RF_tot", ok), ("nspecs", VAR_A, VAR_B, []),
           ("nspecs", VAR_A, VAR_B, ok * 33), ("window", VAR_A, VAR_B, [PairMetric("slope", (1800, 1851))]),
           ("window", VAR_A, vec, [PairMetric("slope", (1799, 1850))]),
           ("reference period of a", VAR_A, VAR_B, [PairMetric("slope", (1800, 1850), baseline=(1744, 1800))]),
           ("reference period of b", VAR_A, vec, [PairMetric("slope", (1800, 1850), baseline_b=(1790, 1810))]),
           ("threshold", VAR_A, VAR_B, [PairMetric("at_first_ge", (1800, 1850))]),
           ("threshold", VAR_A, VAR_B, [PairMetric("mean_where_ge", (1800, 1850))]),
           ("not finite in 1803", VAR_A, (vec[0], np.where(vec[0] == 1803, np.nan, 1.0)), ok)]
    for msg, a, b, s in bad:
        for fn, call in verbs:
            with pytest.raises(E, match=fn + ".*" + msg):
                call(core, a, b, s)
    for fn, call in verbs[1:]:
        for msg, wt in (("negative", np.where(np.arange(n) == 3, -1.0, 1.0)), ("all zero", np.zeros(n))):
            with pytest.raises(E, match=fn + ".*" + msg):
                call(core, VAR_A, VAR_B, ok, weights=wt)
    with pytest.raises(E, match="hx_pair_metric_quantiles.*nprobs"):
        core.pair_metric_quantiles(VAR_A, VAR_B, ok, [])
    with pytest.raises(E, match="hx_pair_metric_probabilities.*nedges"):
        core.pair_metric_probabilities(VAR_A, VAR_B, ok, [])
    with pytest.raises(E, match="hx_pair_metric_moments.*npred"):
        _npred_nine(core)
    # the verbs themselves, and the refused calls, changed nothing
    for fn, call in verbs:
        call(core, VAR_A, VAR_B, ok)
        call(core, VAR_A, vec, ok)
    assert np.array_equal(before, core.fetchvars(VAR_A, (Y0, 1850)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    # ... and the core goes on as a fresh one does
    core.run(1900)
    fresh.run(1850)
    fresh.run(1900)
    assert np.array_equal(core.fetchvars(VAR_B, (Y0, 1900)), fresh.fetchvars(VAR_B, (Y0, 1900)))
    core.shutdown(); fresh.shutdown()


def _npred_nine(core):
    """npred = 9 through the C function (the binding refuses nine entries itself)."""
    import ctypes
    from hector_amd.core import _HxPairMetric
    dp = ctypes.POINTER(ctypes.c_double)
    n = core.n_members
    arr = (_HxPairMetric * 1)(PairMetric("slope", (1800, 1850))._c())
    pred, shift, sums = np.ones((9, n)), np.zeros(1), np.zeros(2 + 27)
    core._ck(core._lib.hx_pair_metric_moments(core._h, VAR_A.encode(), VAR_B.encode(), None, 0, 0, ctypes.byref(arr), 1,
                                              None, pred.ctypes.data_as(dp), 9, shift.ctypes.data_as(dp),
                                              sums.ctypes.data_as(dp), None, None))


def test_the_carbon_budget_example_runs(hip_lib, capsys):
    spec = importlib.util.spec_from_file_location("example_carbon_budget", os.path.join(ROOT, "examples", "carbon_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 640
    tcre, crossing, bands = mod.main(n, lib_path=hip_lib)
    out = capsys.readouterr().out
    assert "TCRE" in out and "1.5 K" in out and "2.0 K" in out and out.count("constrained") >= 3
    assert tcre.shape == (n,) and np.isfinite(tcre).mean() > 0.9 and (tcre[np.isfinite(tcre)] > 0).all()
    assert crossing.shape == (2, n) and np.isnan(crossing[1]).any() and np.isfinite(crossing[0]).any()
    assert np.isfinite(bands["prior"]).all() and np.isfinite(bands["constrained"]).all()
