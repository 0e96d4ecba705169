"""hx_ensemble_quantiles (Core.quantiles) on the GPU: exact weighted inverted-CDF quantiles.

The authority is `checker` below, a numpy implementation of the integer definition of
include/hector_amd.h: weights quantised to q = rint(w / wmax * 2^32), members with q > 0 and a
value that is not NaN take part, stable sort, cumulative sum of q in uint64, first index whose sum
reaches t = max(1, ceil(p * float(W))).  Everything is compared with `==`: the answer is a value
some member has (zeros of either sign compare equal).
"""
import ctypes
import math

import numpy as np
import pytest

import hector_amd
from hector_amd import ensemble
from conftest import SCENARIO

pytestmark = pytest.mark.gpu

PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
VARS = ("CO2_concentration", "global_tas")


def quantise(w):
    return np.rint(w / w.max() * 2.0 ** 32).astype(np.uint64)


def checker(x, q, probs):
    """x[n] values, q[n] uint64 weights -> (quantiles[len(probs)], members taking part)."""
    part = ~np.isnan(x) & (q > 0)
    v, w = x[part], q[part]
    if v.size == 0:
        return np.full(len(probs), np.nan), 0
    order = np.argsort(v, kind="stable")
    vs, cum = v[order], np.cumsum(w[order], dtype=np.uint64)
    W = int(cum[-1])
    assert W <= 2 ** 52
    out = np.empty(len(probs))
    for j, p in enumerate(probs):
        t = max(1, math.ceil(p * float(W)))
        out[j] = vs[int(np.searchsorted(cum, np.uint64(t), side="left"))]
    return out, int(v.size)


def check_rows(x, got, npart, weights, probs, what):
    """x[ny, n] (fetchvars), got[ny, np], npart[ny] against the checker, row by row."""
    q = np.ones(x.shape[1], dtype=np.uint64) if weights is None else quantise(weights)
    for y in range(x.shape[0]):
        ref, cnt = checker(x[y], q, probs)
        assert npart[y] == cnt, (what, y, npart[y], cnt)
        if cnt == 0:
            assert np.isnan(got[y]).all(), (what, y, got[y])
        else:
            assert (got[y] == ref).all(), (what, y, got[y], ref)


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


def _score_weights(core):
    """exp(-chi2 / 2) of CO2 1850-2014 against member 0 plus seeded noise, as a calibration does."""
    years = np.arange(1850, 2015)
    rng = np.random.default_rng(5)
    truth = core.fetchvars("CO2_concentration", (1850, 2014))[:, 0]
    obs = truth + rng.normal(0.0, 1.0, years.size)
    chi2 = core.score("CO2_concentration", years, obs, sigma=np.full(years.size, 4.0))
    w = np.exp(-0.5 * (chi2 - chi2.min()))
    w[core.status() != 0] = 0.0
    return w


def test_full_size_ensemble_on_the_one_wavefront_kernel(hip_lib):
    n = 65536
    core = _core(n, hip_lib)
    core.run(2300)
    assert core.last_run_kernel() == "run"
    w = _score_weights(core)
    assert (quantise(w) == 0).any() and (quantise(w) > 0).sum() > 10
    for var in VARS:
        x = core.fetchvars(var, (1745, 2300))
        for weights in (None, w):
            got, npart = core.quantiles(var, PROBS, (1745, 2300), weights=weights, counts=True)
            assert got.shape == (556, 5)
            check_rows(x, got, npart, weights, PROBS, (var, weights is not None))
        if np.__version__ >= "2.0" and not np.isnan(x[300]).any():   # a second opinion, one row
            ref = np.quantile(x[300], PROBS, method="inverted_cdf")
            assert (core.quantiles(var, PROBS, (2045, 2045))[0] == ref).all()
    # p = 0 and p = 1 are the min and max of the statistics kernel
    st = core.ensemble_stats(list(VARS), (1745, 2300))
    for k, var in enumerate(VARS):
        ends = core.quantiles(var, [0.0, 1.0], (1745, 2300))
        assert (ends[:, 0] == st[k][:, 3]).all() and (ends[:, 1] == st[k][:, 4]).all()
    core.shutdown()


def test_pair_kernel_ensemble(hip_lib):
    core = _core(1000, hip_lib)
    core.run(2300)
    assert core.last_run_kernel() == "pair"
    w = _score_weights(core)
    for var in VARS:
        x = core.fetchvars(var, (1745, 2300))
        for weights in (None, w):
            got, npart = core.quantiles(var, PROBS, (1745, 2300), weights=weights, counts=True)
            check_rows(x, got, npart, weights, PROBS, (var, weights is not None))
    core.shutdown()


def test_two_wave_ensemble_and_adopted_lane_calibration(hip_lib):
    n = 131072
    core = _core(n, hip_lib, beta=False)
    core.run(2300)
    assert core.last_run_kernel() == "run2"
    w = _score_weights(core)
    first = {}
    for var in VARS:
        x = core.fetchvars(var, (2200, 2300))
        for weights in (None, w):
            got, npart = core.quantiles(var, PROBS, (2200, 2300), weights=weights, counts=True)
            check_rows(x, got, npart, weights, PROBS, (var, weights is not None))
            first[(var, weights is not None)] = (x, got)
    # the lanes reordered by measured cost: other lanes, the same members, the same bits
    lanes = core.lane_of_member()
    core.reset(core.strtdate)
    core.run(2300)
    if core.lanes_calibrated():
        assert not np.array_equal(lanes, core.lane_of_member())
    for var in VARS:
        x = core.fetchvars(var, (2200, 2300))
        for weights in (None, w):
            got = core.quantiles(var, PROBS, (2200, 2300), weights=weights)
            x0, got0 = first[(var, weights is not None)]
            if np.array_equal(x, x0):
                assert np.array_equal(got, got0, equal_nan=True)
            got3, n3 = core.quantiles(var, PROBS, (2298, 2300), weights=weights, counts=True)
            check_rows(x[-3:], got3, n3, weights, PROBS, (var, "calibrated lanes"))
    core.shutdown()


def test_member_sorting_does_not_change_the_bits(hip_lib):
    res = []
    for sorting in (True, False):
        core = _core(3000, hip_lib, pair_limit=0)
        core.set_member_sorting(sorting)
        core.run(1900)
        rng = np.random.default_rng(11)
        w = rng.random(3000) ** 8
        res.append((core.fetchvars("global_tas", (1745, 1900)),
                    core.quantiles("global_tas", PROBS, (1745, 1900), weights=w),
                    core.quantiles("global_tas", PROBS, (1745, 1900))))
        check_rows(res[-1][0], res[-1][1], core.quantiles("global_tas", PROBS, (1745, 1900), weights=w,
                                                         counts=True)[1], w, PROBS, sorting)
        core.shutdown()
    if np.array_equal(res[0][0], res[1][0]):   # (the same trajectories: then the same quantiles)
        assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def _hip_runtime():
    """The HIP runtime that is already in the process (the library's own)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in the process")


def _write_row(core, var, year, values, pad_value):
    """values[n_members] (member order) into the recorded row of `year`, through the device
    pointer of hx_device_var; the padding lanes get pad_value (they never take part)."""
    ptr, npad = core.device_var(var)
    assert core.strtdate <= year <= core.current_date and npad >= core.n_members
    row = np.full(npad, pad_value)
    row[core.lane_of_member()] = values
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    dst = ptr + (year - core.strtdate) * npad * 8
    assert hip.hipMemcpy(ctypes.c_void_p(dst), row.ctypes.data_as(ctypes.c_void_p), npad * 8, 1) == 0


def test_hostile_rows(hip_lib):
    n = 777   # 13 wavefronts, 55 padding lanes
    core = _core(n, hip_lib)
    core.run(1800)
    rng = np.random.default_rng(3)
    tiny = 5e-324
    rows = {
        "all equal": np.full(n, 3.25),
        "two values": np.where(rng.random(n) < 0.3, 1.0, 1.0 + 2.0 ** -52),
        "negatives and both zeros": rng.choice([-2.5, -1.0, -0.0, 0.0, 1.0, -1e-300, 1e-300], n),
        "denormals": rng.integers(-40, 40, n) * tiny,
        "infinities": rng.choice([-np.inf, np.inf, 0.0, 1.0, -1.0], n),
        "NaN-laced": np.where(rng.random(n) < 0.4, np.nan, rng.normal(0, 1, n)),
        "all NaN": np.full(n, np.nan),
        "one value among NaN": np.where(np.arange(n) == 500, -7.0, np.nan),
        "full range": rng.normal(0, 1, n) * 10.0 ** rng.integers(-300, 300, n),
        "ties": np.round(rng.normal(0, 3, n)),
    }
    w_wide = 2.0 ** -rng.uniform(0, 40, n)      # some quantise to 0
    w_wide[rng.integers(0, n)] = 1.0
    w_one = np.zeros(n)
    w_one[123] = 0.7                            # one participating member
    probs = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
    assert (quantise(w_wide) == 0).any()
    for k, (name, values) in enumerate(rows.items()):
        year = 1750 + k
        _write_row(core, "global_tas", year, values, pad_value=-1e300 if k % 2 else np.nan)
        x = core.fetchvars("global_tas", (year, year))
        assert np.array_equal(x[0], values, equal_nan=True)
        for weights in (None, w_wide, w_one):
            got, npart = core.quantiles("global_tas", probs, (year, year), weights=weights, counts=True)
            check_rows(x, got, npart, weights, probs, (name, None if weights is None else weights.max()))
    # all of them in one call, next to untouched rows
    x = core.fetchvars("global_tas", (1745, 1800))
    for weights in (None, w_wide):
        got, npart = core.quantiles("global_tas", probs, weights=weights, counts=True)
        check_rows(x, got, npart, weights, probs, "all rows")
    got = core.quantiles("global_tas", tuple(np.linspace(0, 1, 16)), (1745, 1800))
    check_rows(x, got, core.quantiles("global_tas", [0.5], (1745, 1800), counts=True)[1], None,
               tuple(np.linspace(0, 1, 16)), "sixteen probabilities")
    core.shutdown()


@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_core_equals_one_core(hip_lib, monkeypatch, shards):
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
    w[:700] = 0.0                    # (the whole first shard of eight, and more, left out)
    w[n - 1] = 5.0                   # the largest weight lives on the last shard
    for weights in (None, w):
        a, na = one.quantiles("global_tas", PROBS, (1745, 1900), weights=weights, counts=True)
        b, nb = many.quantiles("global_tas", PROBS, (1745, 1900), weights=weights, counts=True)
        assert np.array_equal(a, b) and np.array_equal(na, nb)
        check_rows(x, b, nb, weights, PROBS, (shards, weights is not None))
    one.shutdown(); many.shutdown()


def test_errors_leave_the_core_usable_and_the_verbs_change_nothing(hip_lib):
    n = 512
    core = _core(n, hip_lib)
    core.run(1850)
    before = core.fetchvars("global_tas", (1745, 1850))
    status, ms = core.status(), core.last_run_ms()
    w = np.ones(n)
    bad = [dict(probs=[]), dict(probs=np.linspace(0, 1, 17)), dict(probs=[1.5]), dict(probs=[float("nan")]),
           dict(probs=[0.5], weights=np.where(np.arange(n) == 3, -1.0, w)),
           dict(probs=[0.5], weights=np.where(np.arange(n) == 3, np.nan, w)),
           dict(probs=[0.5], weights=np.where(np.arange(n) == 3, np.inf, w)),
           dict(probs=[0.5], weights=np.zeros(n)),
           dict(probs=[0.5], dates=(1745, 1851))]
    for kw in bad:
        with pytest.raises(hector_amd.HectorAmdError, match="hx_ensemble_quantiles"):
            core.quantiles("global_tas", **kw)
    with pytest.raises(hector_amd.HectorAmdError, match="not enabled"):
        core.quantiles("RF_tot", [0.5])
    good = core.quantiles("global_tas", PROBS, weights=w)
    assert np.array_equal(good, core.quantiles("global_tas", PROBS))
    core.score("global_tas", [1800, 1850], [0.1, 0.2])
    assert np.array_equal(before, core.fetchvars("global_tas", (1745, 1850)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    # ... and the core goes on as a fresh one does
    core.run(1900)
    fresh = _core(n, hip_lib)
    fresh.run(1850)
    fresh.run(1900)
    assert np.array_equal(core.fetchvars("global_tas", (1745, 1900)), fresh.fetchvars("global_tas", (1745, 1900)))
    core.shutdown(); fresh.shutdown()
