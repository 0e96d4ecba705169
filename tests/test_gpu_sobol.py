"""hx_ensemble_sobol / hx_metric_sobol (Core.sobol, Core.metric_sobol) on the GPU.

The authority is `checker` below: it applies the participation rule of include/hector_amd.h (the
group is in use and none of its k + 2 values is NaN), takes c_y as the exact minimum of x_A and x_B
over the participating groups, forms every difference in float64 (that rounding is part of the
definition) and accumulates the sums in np.longdouble.

Exact (`==`): n_part, shift; rows whose participating values are all equal (every sum 0); two
identical calls.  Sums: |S - S_ref| <= (n_part + 8) 2^-53 S_ref -- every term is >= 0, so the bound
holds for every summation order and lane order.

The parameters come from ensemble.saltelli: column 0 is S in 1.5..6, column 1 q10_rh in 1..3, column 2
beta in 0.2..0.8; further columns feed nothing (dummy factors).  The shapes are the smallest at which
the kernels can still go wrong: a group count that is no multiple of the wavefront or the chunk (1301:
two chunks, a ragged tail, three trailing members ignored), k = 1, k = 16 (two factor tiles), one
group, the pair and two-wave year-loop kernels, both lane orders.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import ROOT, SCENARIO

pytestmark = pytest.mark.gpu

E = hector_amd.HectorAmdError
U = 2.0 ** -53
LD = np.longdouble
RANGES = (("S", 1.5, 4.5, "degC"), ("q10_rh", 1.0, 2.0, None), ("beta", 0.2, 0.6, None))


def checker(x, k, nb, use=None):
    """x[ny, n] in member order -> dict of shift[ny], n_part[ny], sums[ny, 4 + 4k] (longdouble)."""
    ny = x.shape[0]
    g = x[:, :nb * (k + 2)].reshape(ny, nb, k + 2)
    used = np.ones(nb, dtype=bool) if use is None else np.asarray(use) != 0
    shift, npart = np.full(ny, np.nan), np.zeros(ny, dtype=np.int64)
    sums = np.zeros((ny, 4 + 4 * k), dtype=LD)
    for y in range(ny):
        on = used & ~np.isnan(g[y]).any(axis=1)
        if not on.any():
            continue
        v = g[y][on]
        c = min(v[:, 0].min(), v[:, 1].min())
        shift[y], npart[y] = c, on.sum()
        dA, dB = (v[:, 0] - c), (v[:, 1] - c)                   # float64: one IEEE subtraction
        assert (dA >= 0).all() and (dB >= 0).all()
        dA, dB = dA.astype(LD), dB.astype(LD)
        sums[y, :4] = dA.sum(), (dA * dA).sum(), dB.sum(), (dB * dB).sum()
        for i in range(k):
            e = (v[:, 0] - v[:, 2 + i]).astype(LD)              # float64 differences, longdouble products
            h = (v[:, 1] - v[:, 2 + i]).astype(LD)
            t, u = e * e, h * h
            sums[y, 4 + 4 * i:8 + 4 * i] = t.sum(), (t * t).sum(), u.sum(), (u * u).sum()
    return dict(shift=shift, n_part=npart, sums=sums)


def check_raw(s, x, k, nb, what, use=None):
    ref = checker(x, k, nb, use)
    assert s.sums.shape == ref["sums"].shape and len(s.names) == k, what
    assert np.array_equal(s.n_part, ref["n_part"]), (what, "n_part")
    assert np.array_equal(s.shift, ref["shift"], equal_nan=True), (what, "shift")
    got = s.sums.astype(LD)
    bound = (ref["n_part"].astype(LD)[:, None] + 8) * LD(U) * ref["sums"]
    err = np.abs(got - ref["sums"])
    worst = float(np.max(np.where(ref["sums"] > 0, err / np.where(ref["sums"] > 0, bound, 1), 0)))
    print("%s: worst sum error / bound %.3g" % (what, worst))
    assert (err <= bound).all(), (what, worst, np.argwhere(err > bound)[:5])
    # rows whose participating values are all equal: every sum exactly 0
    flat = (ref["n_part"] > 0) & (ref["sums"] == 0).all(axis=1)
    assert (s.sums[flat] == 0).all(), what
    empty = ref["n_part"] == 0
    assert (s.sums[empty] == 0).all() and np.isnan(s.shift[empty]).all(), what
    assert not (s.total < 0).any(), what
    return ref


def same_bits(a, b):
    return (np.array_equal(a.shift, b.shift, equal_nan=True) and np.array_equal(a.sums, b.sums) and
            np.array_equal(a.n_part, b.n_part))


def _core(hip_lib, k, nb, extra=0, pair_limit=None, sorting=None, **kw):
    n = nb * (k + 2) + extra
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    u = np.concatenate([ensemble.saltelli(nb, k), ensemble.uniform01(np.arange(extra), 99)[:, None] * np.ones((1, k))])
    for i, (name, lo, width, units) in enumerate(RANGES[:k]):
        if units:
            c.setvar(name, lo + width * u[:, i], units)
        else:
            c.setvar(name, lo + width * u[:, i])
    if pair_limit is not None:
        c.set_pair_kernel_limit(pair_limit)
    if sorting is not None:
        c.set_member_sorting(sorting)
    return c


def _check_window(core, k, nb, years, what, var="global_tas", use=None):
    x = core.fetchvars(var, years)
    s = core.sobol(var, k, years, n_base=nb, use=use)
    check_raw(s, x, k, nb, what, use)
    assert same_bits(s, core.sobol(var, k, years, n_base=nb, use=use)), what
    return x, s


@pytest.fixture(scope="module")
def ragged(hip_lib):
    """k = 3, 1301 groups in a 6 508-member core on the one-wavefront kernel, run to 2100."""
    core = _core(hip_lib, 3, 1301, extra=3, pair_limit=0)
    core.run(2100)
    assert core.n_members == 6508 and core.last_run_kernel() == "run"
    yield core
    core.shutdown()


def test_ragged_tail_and_trailing_members(ragged):
    for var in ("global_tas", "CO2_concentration"):
        x, s = _check_window(ragged, 3, 1301, (1745, 1900), ("ragged", var), var=var)
        assert (s.n_part == 1301).all()
    assert s.var[-1] > 0
    # names as labels, the default n_base, fewer groups than fit
    s2 = ragged.sobol("global_tas", ["S", "q10_rh", "beta"], (1745, 1900))
    assert s2.names == ["S", "q10_rh", "beta"]
    assert same_bits(s2, ragged.sobol("global_tas", 3, (1745, 1900), n_base=1301))
    _check_window(ragged, 3, 1024, (1890, 1900), "exactly one chunk")
    _check_window(ragged, 3, 1025, (1890, 1900), "one group into the second chunk")
    # the indices say what the model says: the climate sensitivity drives the warming of 1900
    s3 = ragged.sobol("global_tas", 3, (1900, 1900))
    print("1900: first %r total %r" % (s3.first[0], s3.total[0]))
    assert s3.total[0, 0] > s3.total[0, 1] and s3.total[0, 0] > s3.total[0, 2]


@pytest.mark.parametrize("k,nb", [(1, 700), (16, 150), (3, 1)])
def test_fewest_and_most_factors_and_one_group(hip_lib, k, nb):
    core = _core(hip_lib, k, nb)
    core.run(1900)
    _check_window(core, k, nb, (1745, 1900), ("k", k, "n_base", nb))
    x, s = _check_window(core, k, nb, (1900, 1900), ("single year", k, nb))
    assert s.sums.shape == (1, 4 + 4 * k) and s.n_part[0] == nb
    core.shutdown()


def test_pair_kernel_ensemble(hip_lib):
    core = _core(hip_lib, 2, 250)
    core.run(1900)
    assert core.n_members == 1000 and core.last_run_kernel() == "pair"
    _check_window(core, 2, 250, (1745, 1900), "pair")
    core.shutdown()


def test_two_wave_ensemble(hip_lib):
    core = _core(hip_lib, 6, 16384)
    core.run(1800)
    assert core.n_members == 131072 and core.last_run_kernel() == "run2"
    _check_window(core, 6, 16384, (1790, 1800), "two-wave")
    core.shutdown()


def test_member_sorting_on_and_off(hip_lib):
    res = []
    for sorting in (True, False):
        core = _core(hip_lib, 3, 1301, extra=3, pair_limit=0, sorting=sorting)
        core.run(1900)
        res.append(_check_window(core, 3, 1301, (1745, 1900), "sorting"))
        core.shutdown()
    (xa, a), (xb, b) = res
    if np.array_equal(xa, xb):   # (the same trajectories: then the same sums within twice the bound)
        assert np.array_equal(a.n_part, b.n_part) and np.array_equal(a.shift, b.shift, equal_nan=True)
        lim = 2 * (a.n_part[:, None] + 8) * U * np.maximum(a.sums, b.sums)
        assert (np.abs(a.sums - b.sums) <= lim).all()


def test_use_mask(ragged):
    rng = np.random.default_rng(7)
    use = np.ones(1301, dtype=np.uint8)
    use[rng.choice(1301, 1301 // 3, replace=False)] = 0
    x, s = _check_window(ragged, 3, 1301, (1850, 1900), "use mask", use=use)
    assert (s.n_part == 1301 - 1301 // 3).all()
    full = ragged.sobol("global_tas", 3, (1850, 1900))
    assert not np.array_equal(full.sums, s.sums)
    none = ragged.sobol("global_tas", 3, (1850, 1900), use=np.zeros(1301))
    assert (none.n_part == 0).all() and np.isnan(none.shift).all() and (none.sums == 0).all()
    assert np.isnan(none.first).all() and np.isnan(none.mean).all()


def test_metric_sobol_and_the_participation_rule(ragged):
    k, nb = 3, 1301
    specs = [Metric("mean", (2081, 2100), baseline=(1850, 1900)), Metric("max", (1745, 2100)),
             Metric("first_ge", (1850, 2100), baseline=(1850, 1900), threshold=2.0),
             Metric("slope", (2000, 2100))]
    rows = ragged.metrics("global_tas", specs)
    assert np.isnan(rows[2]).any() and not np.isnan(rows[2]).all()
    s = ragged.metric_sobol("global_tas", specs, ["S", "q10_rh", "beta"])
    assert s.sums.shape == (4, 16)
    ref = check_raw(s, rows, k, nb, "metric_sobol")
    assert same_bits(s, ragged.metric_sobol("global_tas", specs, 3, n_base=nb))
    whole = int((~np.isnan(rows[2, :nb * (k + 2)].reshape(nb, k + 2)).any(axis=1)).sum())
    assert 0 < whole < nb and s.n_part[2] == whole == ref["n_part"][2]
    assert (s.n_part[[0, 1, 3]] == nb).all()
    use = (np.arange(nb) % 3 != 1).astype(np.uint8)
    check_raw(ragged.metric_sobol("global_tas", specs, 3, use=use), rows, k, nb, "metric_sobol with use", use)
    assert np.isfinite(s.first).all() and np.isfinite(s.total_se).all()


def test_dummy_factor(hip_lib):
    k, nb = 4, 500
    core = _core(hip_lib, k, nb)
    core.run(2100)
    x, s = _check_window(core, k, nb, (1745, 2100), "dummy factor")
    g = x.reshape(x.shape[0], nb, k + 2)
    same = (g[:, :, 0] == g[:, :, 5]).all(axis=1) & (s.var > 0)
    print("rows whose A and AB_3 values are bitwise equal: %d of %d" % (same.sum(), same.size))
    assert (s.total[same, 3] == 0).all() and (s.sums[same, 4 + 4 * 3] == 0).all()
    assert abs(s.first[-1, 3]) <= 4 * s.first_se[-1, 3]
    assert not (s.total < 0).any() and np.isfinite(s.total[-1]).all()
    assert s.total[-1, 0] > s.total[-1, 3]
    core.shutdown()


def test_every_documented_error_and_nothing_changes(hip_lib, monkeypatch):
    k, nb = 2, 128
    core = _core(hip_lib, k, nb)
    fresh = _core(hip_lib, k, nb)
    ok = [Metric("mean", (1800, 1850))]
    for fn, call in (("hx_ensemble_sobol", lambda: fresh.sobol("global_tas", 2, (1745, 1745))),
                     ("hx_metric_sobol", lambda: fresh.metric_sobol("global_tas", [Metric("mean", 1745)], 2))):
        with pytest.raises(E, match=fn + ".*run the core first"):
            call()
    fresh.shutdown()
    core.run(1850)
    before = core.fetchvars("global_tas", (1745, 1850))
    status, ms = core.status(), core.last_run_ms()
    with pytest.raises(E, match="hx_ensemble_sobol.*k must lie in 1..16"):
        core.sobol("global_tas", 0, n_base=1)
    with pytest.raises(E, match="hx_metric_sobol.*k must lie in 1..16"):
        core.metric_sobol("global_tas", ok, 0, n_base=1)
    with pytest.raises(E, match="hx_ensemble_sobol.*n_base"):
        core.sobol("global_tas", 2, n_base=0)
    with pytest.raises(E, match="hx_ensemble_sobol.*exceeds the 512 members"):
        core.sobol("global_tas", 2, n_base=129)
    with pytest.raises(E, match="hx_metric_sobol.*exceeds the 512 members"):
        core.metric_sobol("global_tas", ok, 15, n_base=31)
    for dates in ((1745, 1851), (1700, 1800)):
        with pytest.raises(E, match="hx_ensemble_sobol.*current date"):
            core.sobol("global_tas", 2, dates)
    with pytest.raises(E, match="hx_metric_sobol.*current date"):
        core.metric_sobol("global_tas", [Metric("mean", (1800, 1851))], 2)
    with pytest.raises(E, match="hx_ensemble_sobol.*not enabled"):
        core.sobol("RF_tot", 2)
    with pytest.raises(E, match="hx_metric_sobol.*not enabled"):
        core.metric_sobol("RF_tot", ok, 2)
    with pytest.raises(E, match="hx_ensemble_sobol"):
        core.sobol("no_such_variable", 2)
    with pytest.raises(E, match="hx_metric_sobol.*nspecs"):
        core.metric_sobol("global_tas", [], 2)
    # k = 17 through the C ABI (the binding refuses more than 16 factors itself)
    dp, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)
    shift, sums, npart = np.empty(106), np.empty((106, 72)), np.zeros(106, dtype=np.int64)
    arr = (type(ok[0]._c()) * 1)(ok[0]._c())
    rc = core._lib.hx_ensemble_sobol(core._h, b"global_tas", 1745, 1850, 17, 1, None, shift.ctypes.data_as(dp),
                                     sums.ctypes.data_as(dp), npart.ctypes.data_as(lp))
    assert rc != 0 and "hx_ensemble_sobol: k must lie in 1..16" in core._lib.hx_last_error().decode()
    rc = core._lib.hx_metric_sobol(core._h, b"global_tas", ctypes.byref(arr), 1, 17, 1, None,
                                   shift.ctypes.data_as(dp), sums.ctypes.data_as(dp), npart.ctypes.data_as(lp))
    assert rc != 0 and "hx_metric_sobol: k must lie in 1..16" in core._lib.hx_last_error().decode()
    # a core of two shards
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    two = _core(hip_lib, k, nb, devices=[0, 0])
    two.run(1850)
    before2 = two.fetchvars("global_tas", (1745, 1850))
    with pytest.raises(E, match="hx_ensemble_sobol.*several shards"):
        two.sobol("global_tas", 2)
    with pytest.raises(E, match="hx_metric_sobol.*several shards"):
        two.metric_sobol("global_tas", ok, 2)
    assert np.array_equal(before2, two.fetchvars("global_tas", (1745, 1850))) and (two.status() == 0).all()
    two.shutdown()
    # the calls and the refused calls changed nothing
    good = core.sobol("global_tas", 2)
    core.metric_sobol("global_tas", ok, 2)
    assert same_bits(good, core.sobol("global_tas", ["S", "q10_rh"], n_base=nb))
    assert np.array_equal(before, core.fetchvars("global_tas", (1745, 1850)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    # ... and the core goes on as a fresh one does
    core.run(1900)
    other = _core(hip_lib, k, nb)
    other.run(1850)
    other.run(1900)
    assert np.array_equal(core.fetchvars("global_tas", (1745, 1900)), other.fetchvars("global_tas", (1745, 1900)))
    core.shutdown(); other.shutdown()


def test_the_sobol_indices_example_runs(hip_lib, capsys):
    spec = importlib.util.spec_from_file_location("example_sobol_indices", os.path.join(ROOT, "examples", "sobol_indices.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so, lin = mod.main(160, lib_path=hip_lib)
    out = capsys.readouterr().out
    assert "first-order" in out and "SRC^2" in out and "crosses 2 K" in out and "diff" in out
    assert so.names == ["S", "q10_rh", "beta", "diff"] and so.sums.shape == (2, 20) and lin.sums.shape == (2, 14)
    assert so.n_part[0] == 160 and 0 < so.n_part[1] <= 160
    assert np.isfinite(so.first).all() and np.isfinite(so.total).all() and (so.total >= 0).all()
    assert so.total[0, 0] == so.total[0].max()       # the climate sensitivity leads the 2100 warming
