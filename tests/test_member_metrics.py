"""hx_member_metrics (Core.metrics): one number per member from a window of a recorded output.

include/hector_amd.h fixes the order of every operation, in IEEE double without fused multiply-add,
so `numpy_metric` below -- a Python loop over the years, vectorised over the members, on fetchvars
output, following those definitions literally -- reproduces the device result bit for bit: no
tolerance anywhere.  The kernel exchanges nothing between lanes, so the host-emulation build runs it
faithfully (CPU part); the same body runs on the GPU against the product library.
"""
import glob
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric
from conftest import ROOT

RUN_TO = 2100
VARS = ("CO2_concentration", "global_tas")
OPS = ("mean", "min", "max", "year_of_min", "year_of_max", "first_ge", "count_ge", "slope")


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


def numpy_metric(x, y0, m):
    """The exact sequence of include/hector_amd.h on x[year - y0, member] for one Metric."""
    n = x.shape[1]
    bad = np.zeros(n, dtype=bool)
    base = None
    if m.baseline is not None:
        s = np.zeros(n)
        for y in range(m.baseline[0], m.baseline[1] + 1):
            s = s + x[y - y0]
            bad |= np.isnan(x[y - y0])
        base = s / float(m.baseline[1] - m.baseline[0] + 1)
    year0, year1 = m.years
    count = year1 - year0 + 1
    thr = m.threshold
    acc = np.zeros(n)
    den = np.zeros(n)
    best = None
    when = np.full(n, np.nan)
    for y in range(year0, year1 + 1):
        bad |= np.isnan(x[y - y0])
        a = x[y - y0] - base if base is not None else x[y - y0]
        if m.op == "mean":
            acc = acc + a
        elif m.op in ("min", "year_of_min", "max", "year_of_max"):
            if y == year0:
                best, when = a.copy(), np.full(n, float(y))
            else:
                with np.errstate(invalid="ignore"):
                    take = a < best if "min" in m.op else a > best
                best = np.where(take, a, best)
                when = np.where(take, float(y), when)
        elif m.op == "first_ge":
            with np.errstate(invalid="ignore"):
                when = np.where(np.isnan(when) & (a >= thr), float(y), when)
        elif m.op == "count_ge":
            with np.errstate(invalid="ignore"):
                acc = acc + np.where(a >= thr, 1.0, 0.0)
        elif m.op == "slope":
            t = float(y) - 0.5 * float(year0 + year1)
            p = t * a
            acc = acc + p
            tt = t * t
            den = den + tt
    if m.op == "mean":
        out = acc / float(count)
    elif m.op in ("min", "max"):
        out = best
    elif m.op in ("year_of_min", "year_of_max", "first_ge"):
        out = when
    elif m.op == "count_ge":
        out = acc
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            out = acc / den
    return np.where(bad, np.nan, out)


def _check(core, var, specs, x=None, y0=None):
    y0 = core.strtdate if y0 is None else y0
    if x is None:
        x = core.fetchvars(var, (y0, core.current_date))
    got = core.metrics(var, specs)
    assert got.shape == (len(specs), core.n_members)
    for k, m in enumerate(specs):
        ref = numpy_metric(x, y0, m)
        assert np.array_equal(got[k], ref, equal_nan=True), (var, m, np.nanmax(np.abs(got[k] - ref)))
    return got


def _thresholds(x, y0, years, baseline):
    """-> (threshold, a matrix): the ensemble median of the window maximum, from numpy alone."""
    a = x[years[0] - y0:years[1] - y0 + 1]
    if baseline is not None:
        a = a - numpy_metric(x, y0, Metric("mean", baseline))
    return float(np.median(a.max(axis=0))), a


def _check_all_ops(core):
    y0 = core.strtdate
    for var in VARS:
        x = core.fetchvars(var, (y0, RUN_TO))
        for baseline in (None, (1850, 1900)):
            thr, a = _thresholds(x, y0, (1950, RUN_TO), baseline)
            specs = [Metric(op, (1950, RUN_TO), baseline=baseline, threshold=thr) for op in OPS]
            got = _check(core, var, specs, x, y0)
            assert np.isfinite(got[:5]).all() and np.isfinite(got[6:]).all()
            # both outcomes of first_ge, established from numpy alone
            crosses = (a >= thr).any(axis=0)
            assert crosses.mean() >= 0.1 and (~crosses).mean() >= 0.1, (var, baseline, crosses.mean())
            first = got[OPS.index("first_ge")]
            assert np.array_equal(np.isnan(first), ~crosses)
            assert (got[OPS.index("count_ge")][~crosses] == 0).all()


def _check_window_shapes(core):
    y0 = core.strtdate
    x = core.fetchvars("global_tas", (y0, RUN_TO))
    thr = float(np.median(x[-1]))
    # a one-year window: every op (slope: 0 / 0 = NaN), at the first and at the last recorded year
    for y in (y0, 1900, RUN_TO):
        got = _check(core, "global_tas", [Metric(op, y, threshold=thr) for op in OPS], x, y0)
        assert np.array_equal(got[0], x[y - y0]) and np.isnan(got[OPS.index("slope")]).all()
    # windows that start at startDate, end at the current date, overlap, share or differ in baseline
    specs = [Metric("mean", (y0, y0 + 40)),
             Metric("slope", (y0, RUN_TO)),
             Metric("max", (2050, RUN_TO), baseline=(y0, y0 + 9)),
             Metric("year_of_max", (2040, 2060), baseline=(RUN_TO - 20, RUN_TO)),
             Metric("mean", (2081, RUN_TO), baseline=(1850, 1900)),
             Metric("count_ge", (1990, 2080), baseline=(1850, 1900), threshold=1.0),
             Metric("first_ge", (2000, RUN_TO), baseline=(1986, 2005), threshold=0.8),
             Metric("min", (1800, 1830)),
             Metric("slope", (2015, 2050), baseline=(2015, 2050))]
    _check(core, "global_tas", specs, x, y0)
    # 32 specifications in one call (eight groups), windows of every length incl. one batch + 1
    many = [Metric(OPS[k % 8], (1760 + 7 * k, 1760 + 7 * k + (k * 5) % 50 + (17 if k % 3 else 0)),
                   baseline=None if k % 4 == 0 else (1850 + k, 1880 + 2 * k), threshold=0.3 + 0.02 * k)
            for k in range(32)]
    _check(core, "global_tas", many, x, y0)
    _check(core, "CO2_concentration", many[:31])
    # one specification as a bare Metric
    assert core.metrics("global_tas", Metric("mean", 2000)).shape == (1, core.n_members)


def _check_errors(core):
    E = hector_amd.HectorAmdError
    ok = Metric("mean", (1900, 1950))
    bad = [("not enabled", "RF_tot", [ok]),
           ("nspecs", "global_tas", []),
           ("nspecs", "global_tas", [ok] * 33),
           ("window", "global_tas", [ok, Metric("max", (1900, RUN_TO + 1))]),
           ("window", "global_tas", [Metric("max", (core.strtdate - 1, 1900))]),
           ("reference period", "global_tas", [Metric("mean", (1900, 1950), baseline=(1850, RUN_TO + 1))]),
           ("reference period", "global_tas", [Metric("mean", (1900, 1950), baseline=(1700, 1900))]),
           ("threshold", "global_tas", [Metric("first_ge", (1900, 1950))]),
           ("threshold", "global_tas", [Metric("count_ge", (1900, 1950))])]
    for msg, var, specs in bad:
        with pytest.raises(E, match="hx_member_metrics.*" + msg):
            core.metrics(var, specs)
    # what the Metric class cannot express: through the C structure
    from hector_amd.core import _HxMetric
    for msg, raw in (("unknown op", _HxMetric(8, 1900, 1950, 1, 0, 0, 0.0)),
                     ("unknown op", _HxMetric(-1, 1900, 1950, 1, 0, 0, 0.0)),
                     ("year1 < year0", _HxMetric(0, 1950, 1900, 1, 0, 0, 0.0))):
        class Raw(Metric):
            def _c(self, raw=raw):
                return raw
        with pytest.raises(E, match="hx_member_metrics.*" + msg):
            core.metrics("global_tas", [Raw("mean", 1900)])
    with pytest.raises(E, match="unknown op"):
        Metric("median", 1900)
    with pytest.raises(E, match="Metric objects"):
        core.metrics("global_tas", ["mean"])
    assert core.current_date == RUN_TO


def _body(n, lib):
    core = _core(n, lib)
    fresh = _core(3, lib)
    with pytest.raises(hector_amd.HectorAmdError, match="hx_member_metrics.*run the core first"):
        fresh.metrics("global_tas", [Metric("mean", fresh.strtdate)])
    fresh.shutdown()
    core.run(RUN_TO)
    before = {v: core.fetchvars(v, (core.strtdate, RUN_TO)) for v in VARS}
    status, ms = core.status(), core.last_run_ms()
    _check_all_ops(core)
    _check_window_shapes(core)
    _check_errors(core)
    # metrics read results: they change none of them, and neither do the refused calls
    for v in VARS:
        assert np.array_equal(before[v], core.fetchvars(v, (core.strtdate, RUN_TO)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    specs = [Metric(op, (1950, RUN_TO), baseline=(1850, 1900), threshold=0.9) for op in OPS]
    sorted_lanes = core.metrics("global_tas", specs)
    core.shutdown()
    # another lane order, the same members: the same bits
    plain = _core(n, lib)
    plain.set_member_sorting(False)
    plain.run(RUN_TO)
    assert np.array_equal(plain.lane_of_member(), np.arange(n))
    got = _check(plain, "global_tas", specs)
    if np.array_equal(plain.fetchvars("global_tas", (plain.strtdate, RUN_TO)), before["global_tas"]):
        assert np.array_equal(got, sorted_lanes, equal_nan=True)
    plain.shutdown()


def test_metrics_equal_numpy_bit_for_bit_in_the_emulation(emul_lib):
    _body(200, emul_lib)


@pytest.mark.gpu
def test_metrics_equal_numpy_bit_for_bit_on_the_gpu(hip_lib):
    _body(4096 + 37, None)


def test_nan_rule_of_the_checker_matches_the_definition():
    """The NaN rule on synthetic rows (no core): a NaN in the window or in the reference period
    makes every operation NaN, a NaN outside both does not."""
    rng = np.random.default_rng(1)
    x = rng.normal(0, 1, (30, 6))
    x[3, 1] = np.nan     # in the reference period 0..9 only
    x[15, 2] = np.nan    # in the window 10..19 only
    x[25, 3] = np.nan    # outside both
    for op in OPS:
        r = numpy_metric(x, 0, Metric(op, (10, 19), baseline=(0, 9), threshold=0.0))
        assert np.isnan(r[1]) and np.isnan(r[2])
        assert np.isfinite(np.delete(r, [1, 2])).all() or op == "first_ge"
        r = numpy_metric(x, 0, Metric(op, (10, 19), threshold=0.0))
        assert not np.isnan(r[1]) or op == "first_ge"
        assert np.isnan(r[2])


def test_sharded_core_metrics_equal_the_single_core(emul_lib):
    n = 11   # 4 + 4 + 3
    one = _core(n, emul_lib)
    many = _core(n, emul_lib, devices=[0, 0, 0])
    for c in (one, many):
        c.run(2020)
    specs = [Metric(op, (1900, 2020), baseline=(1850, 1900), threshold=0.5) for op in OPS] + \
            [Metric("mean", 2020), Metric("slope", (one.strtdate, 2020))]
    for var in VARS:
        a, b = one.metrics(var, specs), many.metrics(var, specs)
        assert a.shape == b.shape == (len(specs), n) and np.array_equal(a, b, equal_nan=True)
        x = many.fetchvars(var, (many.strtdate, 2020))
        for k, m in enumerate(specs):
            assert np.array_equal(b[k], numpy_metric(x, many.strtdate, m), equal_nan=True)
    with pytest.raises(hector_amd.HectorAmdError, match="hx_member_metrics.*window"):
        many.metrics("global_tas", [Metric("mean", 2021)])
    with pytest.raises(hector_amd.HectorAmdError, match="hx_member_metrics.*nspecs"):
        many.metrics("global_tas", [])
    assert np.array_equal(one.status(), many.status())   # the refused calls poisoned nothing
    assert np.array_equal(one.metrics("global_tas", specs), many.metrics("global_tas", specs), equal_nan=True)
    one.shutdown(); many.shutdown()


def test_cooperative_verbs_are_refused_in_the_emulation(emul_lib):
    """The select and bin kernels are cooperative (LDS atomics, cross-lane): one lane at a time
    cannot run them, and the emulation says so instead of returning numbers."""
    one = _core(5, emul_lib)
    many = _core(5, emul_lib, devices=[0, 0])
    spec = [Metric("mean", (1750, 1760))]
    for c in (one, many):
        c.run(1760)
        for call in (lambda: c.metric_quantiles("global_tas", spec, [0.5]),
                     lambda: c.probabilities("global_tas", [0.0, 1.0]),
                     lambda: c.metric_probabilities("global_tas", spec, [0.0, 1.0])):
            with pytest.raises(hector_amd.HectorAmdError, match="not available in the host-emulation build"):
                call()
        assert np.isfinite(c.fetchvars("global_tas", (1745, 1760))).all()
        assert np.isfinite(c.metrics("global_tas", spec)).all()
        c.shutdown()


def test_python_checks_shapes_before_the_call(emul_lib):
    c = _core(4, emul_lib)
    c.run(1760)
    spec = [Metric("mean", 1760)]
    E = hector_amd.HectorAmdError
    with pytest.raises(E, match="weights must have n_members"):
        c.metric_quantiles("global_tas", spec, [0.5], weights=np.ones(3))
    with pytest.raises(E, match="weights must have n_members"):
        c.probabilities("global_tas", [0.0], weights=np.ones(5))
    with pytest.raises(E, match="edges must be one-dimensional"):
        c.metric_probabilities("global_tas", spec, [[0.0, 1.0]])
    c.shutdown()


def test_metric_kernel_has_no_contracted_multiply_add():
    """fp contraction is off for the metric kernel: the slope's t * a and num + p are a v_mul_f64 and
    a v_add_f64.  The only fused multiply-adds belong to the compiler's correctly rounded expansion
    of the fp64 divisions (v_div_scale .. v_div_fmas, v_div_fixup), ahead of their v_div_fmas."""
    files = glob.glob(os.path.join(ROOT, "hector_amd", "build", "hx_post-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not files:
        pytest.skip("no assembly in hector_amd/build (the library was not built in this tree)")
    text = open(files[0], errors="replace").read()
    name = re.search(r"^(_Z\d+hx_metric_kernel\w*):", text, flags=re.M).group(1)
    k = text.index(name + ":")
    body = text[k:text.index(".Lfunc_end", k)]
    ops = re.findall(r"^\s+(v_\w+_f64\w*)", body, flags=re.M)
    assert "v_mul_f64" in ops and "v_add_f64" in ops
    in_div = False
    for op in ops:
        if op.startswith("v_div_scale"):
            in_div = True
        elif op.startswith("v_div_fmas") or op.startswith("v_div_fixup"):
            in_div = False
        elif op.startswith("v_fma") or op.startswith("v_mac") or op.startswith("v_pk_fma"):
            assert in_div, "a fused multiply-add outside a division: %r" % ops
    assert sum(o.startswith("v_div_fixup") for o in ops) >= 2
