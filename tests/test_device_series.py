"""hx_series_define / hx_series_drop / hx_series_list (Core.hold, Core.derive, Core.drop_series,
Core.series) and the one resolver of the per-member verbs.

include/hector_amd.h fixes the order of every series operation, in IEEE double without fused
multiply-add, so `numpy_series` below -- a literal restatement on fetchvars output -- reproduces
every block bit for bit: `np.array_equal(..., equal_nan=True)`, no tolerance anywhere.  The kernels
exchange nothing between lanes, so the host-emulation build runs them faithfully (CPU part); the same
bodies run on the GPU against the product library.
"""
import numpy as np
import pytest

import hector_amd
from hector_amd import Metric

RUN_TO = 2100
VARS = ("CO2_concentration", "global_tas")
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


# ---- the definitions of include/hector_amd.h, literally ------------------------------------------

def numpy_series(op, a, b=None, *, y0, years=None, width=None, align="trailing", lag=None, first_year=None):
    """a[year - y0, member] over startDate..the valid end -> z of the same shape.  b: an array of a's
    shape, a number, or a per-year vector that starts at first_year (NaN outside its span)."""
    ny, n = a.shape
    nan = np.full(n, np.nan)
    if op == "copy":
        return a.copy()
    if op in ("add", "sub", "mul", "div"):
        if np.ndim(b) == 0:
            bb = np.full((ny, 1), float(b))
        elif np.ndim(b) == 1:
            bb = np.full((ny, 1), np.nan)
            for i, v in enumerate(b):
                if 0 <= first_year + i - y0 < ny:
                    bb[first_year + i - y0, 0] = v
        else:
            bb = b
        with np.errstate(all="ignore"):
            return {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[op](a, bb)
    z = np.empty_like(a)
    if op == "anomaly":
        s = np.zeros(n)
        for y in range(years[0], years[1] + 1):
            s = s + a[y - y0]
        base = s / float(years[1] - years[0] + 1)
        for k in range(ny):
            z[k] = a[k] - base
    elif op == "cumsum":
        k0 = years - y0
        z[:k0] = np.nan
        z[k0:] = np.cumsum(a[k0:], axis=0)
    elif op == "runmean":
        back = width - 1 if align == "trailing" else (width - 1) // 2
        for k in range(ny):
            lo, hi = k - back, k - back + width - 1
            if lo < 0 or hi > ny - 1:
                z[k] = nan
                continue
            s = np.zeros(n)
            for j in range(lo, hi + 1):
                s = s + a[j]
            z[k] = s / float(width)
    elif op == "delta":
        z[:lag] = np.nan
        z[lag:] = a[lag:] - a[:ny - lag]
    else:
        raise ValueError(op)
    return z


def numpy_metric(x, y0, m):
    """hx_member_metrics' sequence (as tests/test_member_metrics.py states it), the ops used here."""
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
    acc = np.zeros(n)
    best = None
    when = np.full(n, np.nan)
    for y in range(year0, year1 + 1):
        bad |= np.isnan(x[y - y0])
        a = x[y - y0] - base if base is not None else x[y - y0]
        if m.op == "mean":
            acc = acc + a
        elif m.op == "max":
            if y == year0:
                best = a.copy()
            else:
                with np.errstate(invalid="ignore"):
                    best = np.where(a > best, a, best)
        elif m.op == "first_ge":
            with np.errstate(invalid="ignore"):
                when = np.where(np.isnan(when) & (a >= m.threshold), float(y), when)
        else:
            raise ValueError(m.op)
    out = acc / float(year1 - year0 + 1) if m.op == "mean" else best if m.op == "max" else when
    return np.where(bad, np.nan, out)


def numpy_score(x, y0, years, obs, sigma, baseline):
    """hx_member_score's sequence (as tests/test_member_score.py states it)."""
    n = x.shape[1]
    base = None
    if baseline is not None:
        s = np.zeros(n)
        for y in range(baseline[0], baseline[1] + 1):
            s = s + x[y - y0]
        base = s / float(baseline[1] - baseline[0] + 1)
    chi = np.zeros(n)
    for i, y in enumerate(years):
        if np.isnan(obs[i]):
            continue
        r = (x[y - y0] - base) - obs[i] if base is not None else x[y - y0] - obs[i]
        if sigma is not None:
            r = r / sigma[i]
        chi = chi + r * r
    return chi


def same(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got, ref, equal_nan=True), (what, np.nanmax(np.abs(got - ref)))


# ---- 1. every operation, bit for bit ----------------------------------------------------------------

def _check_ops(core):
    y0 = core.strtdate
    ny = RUN_TO - y0 + 1
    x = {v: core.fetchvars(v, (y0, RUN_TO)) for v in VARS}

    def run(name, op, a, b=None, ref_a=None, ref_b=None, **kw):
        core.derive(name, op, a, b, **kw)
        got = core.fetchvars(name, (y0, RUN_TO))
        nk = {k: v for k, v in kw.items()}
        ref = numpy_series(op, x[a] if ref_a is None else ref_a, b if ref_b is None else ref_b, y0=y0, **nk)
        same(got, ref, (name, op, a, kw))
        return got

    for var in VARS:
        core.hold("held", var)
        same(core.fetchvars("held", (y0, RUN_TO)), x[var], ("hold", var))
        assert core.series()["held"] == RUN_TO
        # scalar, vector and variable operands
        for op, c in (("add", 1.5), ("sub", 0.1), ("mul", 1.0 / 3.0), ("div", 3.0), ("div", 0.0)):
            run("s1", op, var, c)
        inside = 0.5 + 0.01 * np.arange(101)                         # 1800..1900: does not cover the run
        beyond = 2.0 + 0.003 * np.arange(2300 - 1700 + 1)            # 1700..2300: starts before, ends after
        for op in ("add", "sub", "mul", "div"):
            z = run("s2", op, var, inside, first_year=1800)
            assert np.isnan(z[:1800 - y0]).all() and np.isnan(z[1901 - y0:]).all() and np.isfinite(z[1800 - y0:1901 - y0]).all()
            z = run("s2", op, var, beyond, first_year=1700)
            assert np.isfinite(z).all()
            other = VARS[1 - VARS.index(var)]
            run("s3", op, var, other, ref_b=x[other])
        # anomaly, cumsum, delta
        for ref_period in ((1850, 1900), (y0, y0), (RUN_TO - 19, RUN_TO), (y0, RUN_TO)):
            run("s4", "anomaly", var, years=ref_period)
        for first in (y0, 1900, RUN_TO):
            core.derive("s5", "cumsum", var, years=first)
            same(core.fetchvars("s5", (y0, RUN_TO)), numpy_series("cumsum", x[var], y0=y0, years=first), ("cumsum", first))
        for k in (1, 10, ny - 1):
            run("s6", "delta", var, lag=k)
        # running means: windows at both edges, w = 1, w = the whole run, odd and even centred widths
        for w in (1, 2, 5, 16, 17, 20, 21, 33, ny - 1, ny):
            for align in ("trailing", "centred"):
                z = run("s7", "runmean", var, width=w, align=align)
                assert np.isfinite(z).any(axis=1).sum() == ny - w + 1
        same(run("s7", "runmean", var, width=1), x[var], "w = 1 is the operand")
    # chained definitions: RUNMEAN of ANOMALY of SUB
    t = x["global_tas"]
    offs = 0.002 * np.arange(ny)
    core.derive("c1", "sub", "global_tas", offs, first_year=y0)
    core.derive("c2", "anomaly", "c1", years=(1850, 1900))
    core.derive("c3", "runmean", "c2", width=20, align="centred")
    r1 = numpy_series("sub", t, offs, y0=y0, first_year=y0)
    r2 = numpy_series("anomaly", r1, y0=y0, years=(1850, 1900))
    r3 = numpy_series("runmean", r2, y0=y0, width=20, align="centred")
    same(core.fetchvars("c3", (y0, RUN_TO)), r3, "chain")
    # a running mean of a series with a NaN head, and a cumulative sum behind it
    core.derive("c4", "delta", "global_tas", lag=3)
    core.derive("c5", "runmean", "c4", width=4)
    core.derive("c6", "cumsum", "c5", years=y0 + 6)
    r5 = numpy_series("runmean", numpy_series("delta", t, y0=y0, lag=3), y0=y0, width=4)
    same(core.fetchvars("c5", (y0, RUN_TO)), r5, "runmean of delta")
    same(core.fetchvars("c6", (y0, RUN_TO)), numpy_series("cumsum", r5, y0=y0, years=y0 + 6), "cumsum of it")
    # replacing a series by an expression of itself
    core.hold("me", "global_tas")
    core.derive("me", "add", "me", "me")
    same(core.fetchvars("me", (y0, RUN_TO)), t + t, "me = me + me")
    core.derive("me", "runmean", "me", width=5)
    r = numpy_series("runmean", t + t, y0=y0, width=5)
    same(core.fetchvars("me", (y0, RUN_TO)), r, "me = runmean(me)")
    core.derive("me", "sub", "global_tas", "me")
    same(core.fetchvars("me", (y0, RUN_TO)), t - r, "me = tas - me")
    core.derive("me", "delta", "me", lag=2)
    same(core.fetchvars("me", (y0, RUN_TO)), numpy_series("delta", t - r, y0=y0, lag=2), "me = delta(me)")
    # metrics and score of a series: the existing definitions on the fetched series
    z = core.fetchvars("c3", (y0, RUN_TO))
    thr = float(np.nanmedian(z[-20]))
    specs = [Metric("mean", (2000, 2050)), Metric("max", (1950, 2080), baseline=(1900, 1950)),
             Metric("first_ge", (1900, 2090), threshold=thr), Metric("mean", (y0, 1800))]
    got = core.metrics("c3", specs)
    for k, m in enumerate(specs):
        same(got[k], numpy_metric(z, y0, m), ("metric of a series", m))
    assert np.isnan(got[3]).all() and np.isfinite(got[:2]).all()     # (the centred mean has no value at startDate)
    crossed = ~np.isnan(got[2])
    assert 0.1 < crossed.mean() < 0.9
    rng = np.random.default_rng(7)
    years = np.arange(1900, 2015)
    rng.shuffle(years)
    obs = 0.006 * (years - 1900) + rng.normal(0, 0.1, years.size)
    obs[::9] = np.nan
    sig = 0.05 + 0.1 * rng.random(years.size)
    for sigma in (None, sig):
        for baseline in (None, (1900, 1950)):
            same(core.score("c3", years, obs, sigma=sigma, baseline=baseline),
                 numpy_score(z, y0, years, obs, sigma, baseline), ("score of a series", baseline))
    for name in list(core.series()):
        core.drop_series(name)
    assert core.series() == {}


# ---- 2. a series is a snapshot of member m's trajectory ---------------------------------------------

def _check_snapshot(core, reorder):
    y0 = core.strtdate
    before = core.fetchvars("global_tas", (y0, RUN_TO))
    lanes_before = core.lane_of_member()
    core.hold("held", "global_tas")
    reorder(core)
    yrs = np.arange(2030, RUN_TO + 1)
    core.setvar_dated("ffi_emissions", yrs, np.full(yrs.size, 2.0), "Pg C/yr")
    core.reset(0)
    core.run(RUN_TO)
    lanes_after = core.lane_of_member()
    assert not np.array_equal(lanes_before, lanes_after)
    after = core.fetchvars("global_tas", (y0, RUN_TO))
    assert not np.array_equal(after, before)
    if reorder is _sorting_off:   # (results do not depend on the lane order: the years before the edit stand)
        assert np.array_equal(after[:2030 - y0 - 1], before[:2030 - y0 - 1])
    same(core.fetchvars("held", (y0, RUN_TO)), before, "held after a new lane order")
    core.derive("d", "sub", "global_tas", "held")
    same(core.fetchvars("d", (y0, RUN_TO)), after - before, "what-if difference")
    avoided = core.metrics("d", [Metric("mean", (2081, RUN_TO))])[0]
    same(avoided, numpy_metric(after - before, y0, Metric("mean", (2081, RUN_TO))), "avoided warming")
    if reorder is _sorting_off:
        assert (avoided < 0).all()
    assert core.series() == {"held": RUN_TO, "d": RUN_TO}


# ---- 3. the resolver ----------------------------------------------------------------------------------

DERIVED = ("slr", "ocean_tas", "RF_N2O", "pH")


def _check_resolver(core):
    y0 = core.strtdate
    rng = np.random.default_rng(3)
    years = np.arange(1900, 2015)
    obs = rng.normal(0, 1.0, years.size)
    for name in DERIVED:
        x = core.fetchvars(name, (y0, RUN_TO))
        assert np.isfinite(x).all() and x[-1].std() > 0
        specs = [Metric("mean", (2081, RUN_TO), baseline=(1986, 2005)), Metric("max", (y0, RUN_TO)),
                 Metric("first_ge", (1900, RUN_TO), threshold=float(np.median(x[-30])))]
        got = core.metrics(name, specs)
        for k, m in enumerate(specs):
            same(got[k], numpy_metric(x, y0, m), (name, m))
        same(core.score(name, years, obs, baseline=(1900, 1950)),
             numpy_score(x, y0, years, obs, None, (1900, 1950)), (name, "score"))
        core.derive("dz", "anomaly", name, years=(1986, 2005))
        same(core.fetchvars("dz", (y0, RUN_TO)), numpy_series("anomaly", x, y0=y0, years=(1986, 2005)), (name, "anomaly"))
    # a recorded output returns exactly what it did before a series with unrelated contents existed
    specs = [Metric("mean", (2000, 2050)), Metric("max", (1950, 2080), baseline=(1900, 1950))]
    core.drop_series("dz")
    m0, s0, f0 = (core.metrics("global_tas", specs), core.score("global_tas", years, obs),
                  core.fetchvars("global_tas", (y0, RUN_TO)))
    core.derive("unrelated", "mul", "CO2_concentration", -7.0)
    same(core.metrics("global_tas", specs), m0, "metrics unchanged")
    same(core.score("global_tas", years, obs), s0, "score unchanged")
    same(core.fetchvars("global_tas", (y0, RUN_TO)), f0, "fetchvars unchanged")
    core.drop_series("unrelated")


# ---- 5. errors -----------------------------------------------------------------------------------------

def _check_errors(core, fresh):
    y0 = core.strtdate
    fn = "hx_series_define"
    core.hold("keep", "global_tas")
    kept = core.fetchvars("keep", (y0, RUN_TO))
    bad = [("variable of the core", lambda: core.hold("global_tas", "CO2_concentration")),
           ("variable of the core", lambda: core.hold("slr", "global_tas")),
           ("variable of the core", lambda: core.hold("pH", "global_tas")),
           ("variable of the core", lambda: core.hold("RF_tot", "global_tas")),          # recorded, not enabled
           ("variable of the core", lambda: core.hold("ffi_emissions", "global_tas")),   # answered on the host
           ("bad series name", lambda: core.hold("9lives", "global_tas")),
           ("bad series name", lambda: core.hold("", "global_tas")),
           ("bad series name", lambda: core.hold("global.veg_c", "global_tas")),
           ("bad series name", lambda: core.hold("x" * 64, "global_tas")),
           ("unknown op", lambda: core.derive("z", "median", "global_tas")),
           ("width < 1", lambda: core.derive("z", "runmean", "global_tas", width=0)),
           ("width exceeds", lambda: core.derive("z", "runmean", "global_tas", width=100000)),
           ("lag must lie", lambda: core.derive("z", "delta", "global_tas", lag=0)),
           ("needs an operand b", lambda: core.derive("z", "add", "global_tas")),
           ("reference period", lambda: core.derive("z", "anomaly", "global_tas", years=(RUN_TO - 5, RUN_TO + 1))),
           ("reference period", lambda: core.derive("z", "anomaly", "global_tas", years=(y0 - 1, y0 + 5))),
           ("year0 must lie", lambda: core.derive("z", "cumsum", "global_tas", years=RUN_TO + 1)),
           ("unknown variable", lambda: core.hold("z", "never_defined")),
           ("not enabled", lambda: core.hold("z", "RF_tot")),
           ("same for every member", lambda: core.hold("z", "ffi_emissions")),
           ("same for every member", lambda: core.derive("z", "add", "global_tas", "ffi_emissions"))]
    for text, call in bad:
        with pytest.raises(E, match=fn + ".*" + text):
            call()
    assert core.series() == {"keep": RUN_TO}
    # a 17th series
    for k in range(15):
        core.derive("n%d" % k, "add", "keep", float(k))
    assert len(core.series()) == 16
    with pytest.raises(E, match=fn + ".*16 series"):
        core.hold("one_too_many", "global_tas")
    core.derive("n3", "mul", "n3", 2.0)                                  # replacing one of the 16 is no 17th
    same(core.fetchvars("n3", (y0, RUN_TO)), (kept + 3.0) * 2.0, "replaced")
    for k in range(15):
        core.drop_series("n%d" % k)
    # a dropped name, in a definition, in a verb and in drop itself
    with pytest.raises(E, match=fn + ".*unknown variable"):
        core.hold("z", "n3")
    with pytest.raises(E, match="hx_member_metrics.*unknown variable"):
        core.metrics("n3", [Metric("mean", 2000)])
    with pytest.raises(E, match="hx_series_drop.*n3"):
        core.drop_series("n3")
    # a verb asked for a year beyond a series' valid-to: the series was defined at 2050
    core.reset(0)
    core.run(2050)
    core.hold("early", "global_tas")
    core.run(RUN_TO)
    assert core.series() == {"keep": RUN_TO, "early": 2050}
    with pytest.raises(E, match="hx_member_metrics.*the window must lie"):
        core.metrics("early", [Metric("mean", (2040, 2051))])
    with pytest.raises(E, match="current date"):
        core.score("early", [2051], [1.0])
    with pytest.raises(E, match="fetchvars.*2050"):
        core.fetchvars("early", (y0, 2051))
    with pytest.raises(E, match=fn + ".*reference period"):
        core.derive("z", "anomaly", "early", years=(2040, 2060))
    full = core.fetchvars("global_tas", (y0, RUN_TO))
    same(core.fetchvars("early", (y0, 2050)), full[:2050 - y0 + 1], "the early series")
    core.derive("both", "sub", "global_tas", "early")                    # valid to the shorter operand
    assert core.series()["both"] == 2050
    same(core.metrics("early", [Metric("mean", (2040, 2050))])[0],
         numpy_metric(full, y0, Metric("mean", (2040, 2050))), "a window inside")
    # the host-answered variables stay refused by the verbs, with a message that says so
    with pytest.raises(E, match="hx_member_metrics.*same for every member"):
        core.metrics("ffi_emissions", [Metric("mean", 2000)])
    # everything above left the core and the first series usable
    same(core.fetchvars("keep", (y0, RUN_TO)), kept, "kept")
    # a core that has not run
    with pytest.raises(E, match=fn + ".*run the core first"):
        fresh.hold("z", "global_tas")
    with pytest.raises(E, match=fn + ".*run the core first"):
        fresh.hold("z", "slr")
    assert fresh.series() == {}


def _sorting_off(core):
    core.set_member_sorting(False)


def _new_varying_parameter(core):
    n = core.n_members
    core.setvar("diff", 2.3 * (0.5 + np.fmod(np.arange(n) * 0.3819660112501051, 1.0)), "cm2/s")


def _r_style(core):
    from hector_amd import core as api
    core.hold("held", "global_tas")
    d = api.fetchvars(core, (2000, 2010), ["held", "global_tas"])
    assert np.array_equal(d["held"], d["global_tas"]) and d["held"].shape == (11, core.n_members)
    assert core.getunits("held") == ""
    core.drop_series("held")


# ---- CPU: the host-emulation build -------------------------------------------------------------------

def test_every_operation_bit_for_bit_emulation(emul_lib):
    core = _core(200, emul_lib)
    core.run(RUN_TO)
    _check_ops(core)
    _r_style(core)
    core.shutdown()


@pytest.mark.parametrize("reorder", [_sorting_off, _new_varying_parameter])
def test_snapshot_survives_a_new_lane_order_emulation(emul_lib, reorder):
    core = _core(200, emul_lib)
    core.run(RUN_TO)
    _check_snapshot(core, reorder)
    core.shutdown()


def test_resolver_derived_diagnostics_emulation(emul_lib):
    core = _core(200, emul_lib)
    core.set_outputs(list(VARS) + list(DERIVED))
    core.run(RUN_TO)
    _check_resolver(core)
    core.shutdown()


def test_errors_emulation(emul_lib):
    core, fresh = _core(70, emul_lib), _core(70, emul_lib)
    core.run(RUN_TO)
    _check_errors(core, fresh)
    core.shutdown()
    fresh.shutdown()


def test_sharded_core_forwards_series_to_every_shard_emulation(emul_lib):
    n = 2 * 70 + 3
    one, many = _core(n, emul_lib), _core(n, emul_lib, devices=[0, 0])
    for c in (one, many):
        c.run(2020)
        c.hold("held", "global_tas")
        c.derive("rm", "runmean", "held", width=11, align="centred")
        c.derive("q", "div", "CO2_concentration", "rm")
    assert many.series() == {"held": 2020, "rm": 2020, "q": 2020}
    y0 = one.strtdate
    for name in ("held", "rm", "q"):
        same(many.fetchvars(name, (y0, 2020)), one.fetchvars(name, (y0, 2020)), name)
    spec = [Metric("mean", (1990, 2010))]
    same(many.metrics("q", spec), one.metrics("q", spec), "metrics of a series on two shards")
    with pytest.raises(E, match="hx_series_define.*variable of the core"):
        many.hold("slr", "global_tas")
    many.drop_series("rm")
    assert many.series() == {"held": 2020, "q": 2020}
    one.shutdown()
    many.shutdown()


# ---- GPU: the same bodies on the product library -----------------------------------------------------

@pytest.mark.gpu
def test_every_operation_bit_for_bit_gpu(hip_lib):
    core = _core(200, hip_lib)
    assert core.backend == "hip"
    core.run(RUN_TO)
    _check_ops(core)
    _r_style(core)
    core.shutdown()


@pytest.mark.gpu
@pytest.mark.parametrize("reorder", [_sorting_off, _new_varying_parameter])
def test_snapshot_survives_a_new_lane_order_gpu(hip_lib, reorder):
    core = _core(200, hip_lib)
    core.run(RUN_TO)
    _check_snapshot(core, reorder)
    core.shutdown()


@pytest.mark.gpu
def test_resolver_derived_diagnostics_gpu(hip_lib):
    core = _core(200, hip_lib)
    core.set_outputs(list(VARS) + list(DERIVED))
    core.run(RUN_TO)
    _check_resolver(core)
    core.shutdown()


@pytest.mark.gpu
def test_errors_gpu(hip_lib):
    core, fresh = _core(70, hip_lib), _core(70, hip_lib)
    core.run(RUN_TO)
    _check_errors(core, fresh)
    core.shutdown()
    fresh.shutdown()
