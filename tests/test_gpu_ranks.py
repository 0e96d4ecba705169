"""hx_series_rank / hx_metric_ranks / hx_ensemble_crps (Core.rank_series, Core.metric_ranks,
Core.crps, Core.spearman) on the GPU: the per-row radix sort and its two epilogues.

The authority is hector_amd.ensemble.midpit / .crps, the numpy restatements of the definitions of
include/hector_amd.h (tests/test_ensemble_ranks.py holds them against a brute-force count and the
energy form).  Every rank is compared with `==`; every CRPS within (m + 8) 2^-53, relatively, of
ensemble.crps evaluated in longdouble, m the number of distinct participating values; pit_obs and
n_part with `==`.

Rows are injected through the device pointer as tests/test_gpu_quantiles.py does it (_write_row is a
copy of its helper).  The sort takes a row in chunks of 2048 pairs (hx_dev_post.h: HXR_CHUNK), a
workgroup's gather and sweeps 512 at a time: the sizes below are one member, a pair, one wavefront
less one / exactly / plus one, and five more than four chunks.

The observations of a row are chosen by `observations`: below every participating value, above every
one, equal to a member's, strictly between two, and NaN.  One row takes the first two and NaN only:
"denormals", whose every value is a multiple of 2^-1074 of at most 40.  With an observation inside
that row the CRPS itself lies below 2^-1022 (3.48e-323 for an observation of 0.0), where a double
is a multiple of 2^-1074 and holds no value to 2^-53 relatively -- the bound cannot be asked of any
result in that format (numpy's float64 evaluation of the definition gives the device's bits there,
0.0).  The row's ranks, which the sort decides, are held like every other row's, and the row
"denormals among normal values" takes all five observations: its gaps between denormals underflow in
the same way, but against a score in the normal range.
"""
import ctypes

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import SCENARIO

pytestmark = pytest.mark.gpu

E = hector_amd.HectorAmdError
LD = np.longdouble
U = 2.0 ** -53
CHUNK = 2048
KINDS = ("pit", "numerator")


def _core(n, hip_lib, pair_limit=None, sorting=None, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    c.setvar("beta", 0.2 + 0.6 * np.fmod(np.arange(n) * 0.7548776662466927, 1.0))
    if pair_limit is not None:
        c.set_pair_kernel_limit(pair_limit)
    if sorting is not None:
        c.set_member_sorting(sorting)
    return c


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


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check_ranks(core, var, window, weights, what, name="r"):
    """rank_series of `window` for both kinds against midpit of fetchvars, with ==; the rows of the
    series outside the window are NaN."""
    x = core.fetchvars(var, window)
    for kind in KINDS:
        core.rank_series(name, var, window, weights=weights, kind=kind)
        assert core.series()[name] == window[1], (what, kind)
        got = core.fetchvars(name, window)
        ref = ensemble.midpit(x, weights, kind)
        bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
        assert not bad.any(), (what, kind, np.argwhere(bad)[:5], got[bad][:5], ref[bad][:5])
        if window[0] > core.strtdate:
            assert np.isnan(core.fetchvars(name, (core.strtdate, window[0] - 1))).all(), (what, kind)
    core.drop_series(name)


def observations(x, q):
    """Below every participating value, above every one, equal to a member's, strictly between two
    (where two distinct values have a double between them), and NaN."""
    v = np.unique(x[~np.isnan(x) & (q > 0)] + 0.0)
    if v.size == 0:
        return np.array([0.0, np.nan])
    obs = [v[0] - abs(v[0]) - 1.0, v[-1] + abs(v[-1]) + 2.0, v[v.size // 2]]
    if v.size > 1:
        k = v.size // 2 - 1
        obs += [v[k] + (v[k + 1] - v[k]) / 2, v[0] + (v[1] - v[0]) / 4]
    return np.array(obs + [np.nan])


def check_crps(core, var, years, obs, weights, what):
    """crps / pit_obs / n_part of (years[i], obs[i]) against ensemble.crps in longdouble -> the worst
    error over its bound."""
    years, obs = np.asarray(years), np.asarray(obs, dtype=np.float64)
    got, pit, npart = core.crps(var, years, obs, weights=weights, return_pit=True, counts=True)
    assert got.shape == pit.shape == npart.shape == years.shape
    worst = 0.0
    for i, (year, y) in enumerate(zip(years, obs)):
        x = core.fetchvars(var, (int(year), int(year)))[0]
        ref, rpit, rn, m = ensemble.crps(x, y, weights, dtype=LD, full=True)
        assert npart[i] == rn, (what, i, npart[i], rn)
        if rn == 0:
            assert np.isnan(got[i]) and np.isnan(pit[i]), (what, i, got[i], pit[i])
            continue
        assert pit[i] == rpit, (what, i, pit[i], rpit)
        err, bound = abs(LD(got[i]) - ref), (m + 8) * LD(U) * ref
        if bound > 0:
            worst = max(worst, float(err / bound))
        assert err <= bound, (what, i, year, y, got[i], ref, float(err), float(bound), m)
    return worst


def hostile_rows(n, rng):
    tiny = 5e-324
    return {
        "all equal": np.full(n, 3.25),                                        # no pass runs
        "two values": np.where(rng.random(n) < 0.3, 1.0, 1.0 + 2.0 ** -52),   # one ulp apart
        "negatives and both zeros": rng.choice([-2.5, -1.0, -0.0, 0.0, 1.0, -1e-300, 1e-300], n),
        "denormals": rng.integers(-40, 40, n) * tiny,
        "infinities": rng.choice([-np.inf, np.inf, 0.0, 1.0, -1.0], n),
        "NaN-laced": np.where(rng.random(n) < 0.4, np.nan, rng.normal(0, 1, n)),
        "all NaN": np.full(n, np.nan),
        "one value among NaN": np.where(np.arange(n) == 500, -7.0, np.nan),
        "full range": rng.normal(0, 1, n) * 10.0 ** rng.integers(-300, 300, n),   # all eight passes
        "ties": np.round(rng.normal(0, 3, n)),
        "denormals among normal values": np.where(rng.random(n) < 0.5, rng.integers(-40, 40, n) * tiny,
                                                  rng.choice([-1.5, 0.25, 2.0], n)),
    }


def hostile_weights(n, rng):
    w_wide = 2.0 ** -rng.uniform(0, 40, n)      # some quantise to 0
    w_wide[rng.integers(0, n)] = 1.0
    w_one = np.zeros(n)
    w_one[123] = 0.7                            # one participating member
    assert (ensemble.quantise(w_wide, n) == 0).any()
    return w_wide, w_one


@pytest.fixture(scope="module")
def hostile(hip_lib):
    """n = 777 (13 wavefronts, 55 padding lanes): the hostile rows in the years 1750.., the padding
    alternately NaN and -1e300 -> core, {name: year}, the two weight vectors."""
    n = 777
    core = _core(n, hip_lib)
    core.run(1800)
    rng = np.random.default_rng(3)
    years = {}
    for k, (name, values) in enumerate(hostile_rows(n, rng).items()):
        years[name] = 1750 + k
        _write_row(core, "global_tas", years[name], values, pad_value=-1e300 if k % 2 else np.nan)
        assert same(core.fetchvars("global_tas", (years[name],) * 2)[0], values)
    yield core, years, hostile_weights(n, rng)
    core.shutdown()


def test_hostile_rows(hostile):
    core, years, (w_wide, w_one) = hostile
    n = core.n_members
    worst = 0.0
    for name, year in years.items():
        for weights in (None, w_wide, w_one):
            what = (name, None if weights is None else weights.max())
            check_ranks(core, "global_tas", (year, year), weights, what)
            if name == "infinities":   # ranks only
                continue
            x = core.fetchvars("global_tas", (year, year))[0]
            obs = observations(x, ensemble.quantise(weights, n))
            if name == "denormals":    # an observation inside the row: a score no double holds (see above)
                obs = obs[[0, 1, -1]]
            worst = max(worst, check_crps(core, "global_tas", np.full(obs.size, year), obs, weights, what))
    print("hostile rows: worst CRPS error / bound %.3g" % worst)
    # all of them in one call, next to untouched model rows
    for weights in (None, w_wide):
        check_ranks(core, "global_tas", (1745, 1800), weights, "all rows")
        check_ranks(core, "global_tas", (1748, 1762), weights, "a window")
    ys = [y for name, y in years.items() if name not in ("infinities", "denormals")] + [1800, 1746, 1799]
    ys = np.array(ys[::-1] + ys[:3])             # neither ascending nor distinct
    x = core.fetchvars("global_tas", (1745, 1800))
    obs = np.array([np.nanmedian(x[y - 1745]) if not np.isnan(x[y - 1745]).all() else 1.0 for y in ys])
    for weights in (None, w_wide):
        check_crps(core, "global_tas", ys, obs, weights, "listed years")
    assert core.series() == {}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4 * CHUNK + 5])
def test_sizes(hip_lib, n):
    core = _core(n, hip_lib)
    core.run(1760)
    rng = np.random.default_rng(100 + n)
    rows = {
        1750: np.round(rng.normal(1.5, 0.6, n), 2),                     # ties
        1751: rng.normal(1.5, 0.6, n),
        1752: np.where(rng.random(n) < 0.3, np.nan, np.round(rng.normal(0, 3, n))),
        1753: rng.normal(0, 1, n) * 10.0 ** rng.integers(-30, 30, n),
    }
    for k, (year, values) in enumerate(rows.items()):
        _write_row(core, "global_tas", year, values, pad_value=-1e300 if k % 2 else np.nan)
    w = rng.random(n) ** 6
    w[rng.integers(0, n)] = 1.0
    w[rng.random(n) < 0.1] = 0.0
    if not w.any():
        w[:] = 1.0
    worst = 0.0
    for weights in (None, w):
        check_ranks(core, "global_tas", (1749, 1754), weights, (n, weights is not None))
        q = ensemble.quantise(weights, n)
        ys, obs = [], []
        for year in (1753, 1750, 1752, 1751, 1755):                     # not ascending
            o = observations(core.fetchvars("global_tas", (year, year))[0], q)
            ys += [year] * o.size
            obs += list(o)
        worst = max(worst, check_crps(core, "global_tas", ys, obs, weights, (n, weights is not None)))
    print("n = %d: worst CRPS error / bound %.3g" % (n, worst))
    core.shutdown()


def _weighted_corr(a, b, q):
    on = (q > 0) & np.isfinite(a) & np.isfinite(b)
    w = q[on].astype(LD)
    w = w / w.sum()
    al, bl = a[on].astype(LD), b[on].astype(LD)
    ma, mb = (w * al).sum(), (w * bl).sum()
    va, vb = (w * (al - ma) ** 2).sum(), (w * (bl - mb) ** 2).sum()
    # the cancellation factors of tests/test_gpu_moments.py: (second moment about the minimum) / variance
    ka = float((w * (al - al.min()) ** 2).sum() / va)
    kb = float((w * (bl - bl.min()) ** 2).sum() / vb)
    return (w * (al - ma) * (bl - mb)).sum() / np.sqrt(va * vb), ka * kb, int(on.sum())


def test_series_behaviour_spearman_and_metric_ranks(hip_lib, monkeypatch):
    n = 1000
    core = _core(n, hip_lib)
    core.run(2100)
    assert core.last_run_kernel() == "pair"
    rng = np.random.default_rng(7)
    w = rng.random(n) ** 4
    w[rng.random(n) < 0.05] = 0.0
    window = (1850, 2100)
    x = core.fetchvars("global_tas", window)
    assert not np.isnan(x).any()
    ref = ensemble.midpit(x, w)
    core.rank_series("pit", "global_tas", window, weights=w)
    assert core.series() == {"pit": 2100}
    assert same(core.fetchvars("pit", window), ref)
    assert np.isnan(core.fetchvars("pit", (1745, 1849))).all()
    # the other verbs take it like a variable
    got = core.quantiles("pit", (0.1, 0.5, 0.9), window)
    assert (got == np.quantile(ref, (0.1, 0.5, 0.9), axis=1, method="inverted_cdf").T).all()
    core.derive("depth", "mul", "pit", "pit").derive("depth", "sub", "pit", "depth")
    assert same(core.fetchvars("depth", window), ref - ref * ref)
    mbd = core.metrics("depth", [Metric("mean", window)])[0]
    assert np.allclose(mbd, (ref - ref * ref).mean(axis=0), rtol=1e-12, atol=0)
    hist = core.probabilities("pit", np.linspace(0.1, 0.9, 9), (2100, 2100))
    assert hist.shape == (1, 10) and abs(hist.sum() - 1.0) < 1e-12
    # a rank of a series, under its own name
    core.rank_series("depth", "depth", (2000, 2100), kind="numerator")
    assert core.series() == {"pit": 2100, "depth": 2100}
    assert same(core.fetchvars("depth", (2000, 2100)), ensemble.midpit((ref - ref * ref)[150:], kind="numerator"))
    assert np.isnan(core.fetchvars("depth", (1745, 1999))).all()
    core.drop_series("depth")
    # Spearman: numpy's weighted Pearson correlation of the reference ranks, the tolerance of corr in
    # tests/test_gpu_moments.py: 4 kappa (n_part + 8) 2^-53, relatively
    tas_2100 = Metric("mean", (2090, 2100))
    against = ["S", "q10_rh", rng.normal(0, 1, n), ("CO2_concentration", tas_2100)]
    rho = core.spearman("global_tas", against, window, weights=w)
    assert rho.shape == (251, 4) and core.series() == {"pit": 2100}
    q = ensemble.quantise(w, n)
    preds = [core.getvar("S"), core.getvar("q10_rh"), against[2], core.metrics("CO2_concentration", [tas_2100])[0]]
    for j, p in enumerate(preds):
        rp = ensemble.midpit(p, w)
        for y in (0, 100, 250):
            r, kappa, cnt = _weighted_corr(ref[y], rp, q)
            assert abs(LD(rho[y, j]) - r) <= 4.0 * kappa * (cnt + 8) * U * abs(r), (j, y, rho[y, j], r, kappa)
    pear = core.moments("global_tas", (2100, 2100), against=["S"]).corr[0, 0]
    spear = core.spearman("global_tas", "S", (2100, 2100))[0, 0]
    print("S against global_tas in 2100: Pearson %.6f Spearman %.6f" % (pear, spear))
    assert -1.0 <= pear <= 1.0 and -1.0 <= spear <= 1.0 and pear * spear > 0
    # a call that raises drops its temporary series too
    with pytest.raises(E, match="hx_series_rank: dates"):
        core.spearman("global_tas", "S", (1850, 2200))
    seen = []

    def failing_moments(name, *a, **k):
        seen.append((name, dict(core.series())))
        raise E("moments failed")
    with monkeypatch.context() as mp:
        mp.setattr(core, "moments", failing_moments)
        with pytest.raises(E, match="moments failed"):
            core.spearman("global_tas", "S", window)
    assert len(seen) == 1 and seen[0][1] == {"pit": 2100, seen[0][0]: 2100} and seen[0][0] != "pit"
    assert core.series() == {"pit": 2100}
    # metric_ranks against midpit of Core.metrics' own output
    specs = [Metric("mean", (2081, 2100), baseline=(1850, 1900)), Metric("max", (1850, 2100)),
             Metric("first_ge", (1850, 2100), threshold=2.0), Metric("slope", (2000, 2100))]
    met = core.metrics("global_tas", specs)
    assert np.isnan(met[2]).any() and not np.isnan(met[2]).all()
    for weights in (None, w):
        for kind in KINDS:
            assert same(core.metric_ranks("global_tas", specs, weights=weights, kind=kind),
                        ensemble.midpit(met, weights, kind)), (weights is not None, kind)
    assert same(core.metric_ranks("pit", [Metric("mean", window)]),
                ensemble.midpit(core.metrics("pit", [Metric("mean", window)])))
    # the series is a snapshot: reset, run and a lane reorder leave member m's ranks with member m
    lanes = core.lane_of_member().copy()
    core.set_member_sorting(False)
    core.reset(0)
    core.run(1900)
    assert not np.array_equal(core.lane_of_member(), lanes)
    assert core.series() == {"pit": 2100}
    assert same(core.fetchvars("pit", window), ref)
    m2 = core.moments("pit", (2000, 2100), weights=w)
    assert (m2.n_part == (q > 0).sum()).all()
    core.rank_series("again", "pit", (2050, 2100), weights=w)
    assert same(core.fetchvars("again", (2050, 2100)), ensemble.midpit(ref[200:], w))
    core.shutdown()


def test_the_same_bits_on_every_lane_order_and_kernel(hip_lib):
    n = 1000
    rng = np.random.default_rng(9)
    w = rng.random(n) ** 4
    years = np.arange(1850, 2015)
    obs = 0.2 + 0.006 * (years - 1850)
    common = np.where(rng.random(n) < 0.1, np.nan, np.round(rng.normal(0.5, 0.4, n), 2))
    res = {}
    for key, kw, kernel in (("pair", {}, "pair"), ("pair unsorted", {"sorting": False}, "pair"),
                            ("run", {"pair_limit": 0}, "run"), ("run unsorted", {"pair_limit": 0, "sorting": False},
                                                               "run")):
        core = _core(n, hip_lib, **kw)
        core.run(2100)
        assert core.last_run_kernel() == kernel
        _write_row(core, "global_tas", 2050, common, pad_value=np.nan)   # one row every core shares
        core.rank_series("r", "global_tas", (1850, 2100), weights=w)
        res[key] = (core.lane_of_member().copy(), core.fetchvars("global_tas", (1850, 2100)),
                    core.fetchvars("r", (1850, 2100)), core.crps("global_tas", years, obs, weights=w, return_pit=True),
                    core.crps("global_tas", [2050, 2050], [0.3, 1.0], weights=w, return_pit=True))
        assert same(res[key][2], ensemble.midpit(res[key][1], w)), key
        core.shutdown()
    assert not np.array_equal(res["pair"][0], res["pair unsorted"][0])
    for key in res:   # the shared row: the same bits from both kernels' cores, in either lane order
        assert same(res[key][2][200], res["pair"][2][200]) and same(res[key][2][200], ensemble.midpit(common, w)), key
        assert same(res[key][4][0], res["pair"][4][0]) and same(res[key][4][1], res["pair"][4][1]), key
    for a, b in (("pair", "pair unsorted"), ("run", "run unsorted")):   # one kernel flavour: the same trajectories
        assert same(res[a][1], res[b][1]) and same(res[a][2], res[b][2]), (a, b)
        assert np.array_equal(res[a][3][0], res[b][3][0]) and np.array_equal(res[a][3][1], res[b][3][1]), (a, b)
    # pair and run kernel: wherever the trajectories agree to the bit, so do the ranks of a year
    # (each was held to midpit of its own trajectories above)
    agree = (res["pair"][1] == res["run"][1]).all(axis=1)
    print("pair and run kernel agree to the bit in %d of %d years" % (agree.sum(), agree.size))
    assert same(res["pair"][2][agree], res["run"][2][agree])


def test_refusals_change_nothing(hip_lib, monkeypatch):
    n = 130
    core = _core(n, hip_lib)
    core.run(1800)
    core.hold("kept", "global_tas")
    before = core.series()
    with pytest.raises(E, match="hx_series_rank: dates must lie between startDate and the current date"):
        core.rank_series("r", "global_tas", (1790, 1801))
    with pytest.raises(E, match="hx_series_rank: dates must lie"):
        core.rank_series("r", "global_tas", (1700, 1750))
    with pytest.raises(E, match="hx_ensemble_crps: dates must lie"):
        core.crps("global_tas", [1750, 1801], [0.0, 0.0])
    with pytest.raises(E, match="hx_metric_ranks: the window must lie"):
        core.metric_ranks("global_tas", [Metric("mean", (1790, 1801))])
    with pytest.raises(E, match="hx_series_rank: bad series name"):
        core.rank_series("9r", "global_tas")
    with pytest.raises(E, match="hx_series_rank: 'global_tas' is a variable of the core"):
        core.rank_series("global_tas", "global_tas")
    with pytest.raises(E, match="hx_series_rank"):
        core.rank_series("r", "no_such_variable")
    with pytest.raises(E, match="hx_series_rank: a weight is negative"):
        core.rank_series("r", "global_tas", weights=-np.ones(n))
    rc = core._lib.hx_series_rank(core._h, b"r", b"global_tas", 1750, 1760, None, 2)
    assert rc != 0 and "hx_series_rank: unknown kind 2" in core._lib.hx_last_error().decode()
    out = np.zeros(n)
    arr, ns = Metric("mean", (1750, 1760))._c(), 1   # (one hx_metric)
    rc = core._lib.hx_metric_ranks(core._h, b"global_tas", ctypes.byref(arr), ns, None, 5,
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc != 0 and "hx_metric_ranks: unknown kind 5" in core._lib.hx_last_error().decode()
    assert core.series() == before
    # a 17th series
    for i in range(15):
        core.rank_series("r%d" % i, "global_tas", (1790, 1800))
    full = core.series()
    assert len(full) == 16
    with pytest.raises(E, match="hx_series_rank: the core holds 16 series already"):
        core.rank_series("one_more", "global_tas")
    with pytest.raises(E, match="hx_series_rank: the core holds 16 series already"):
        core.spearman("global_tas", "S")
    core.rank_series("r3", "kept", (1795, 1800), kind="numerator")      # replacing one is no 17th
    assert core.series() == dict(full, r3=1800)
    assert same(core.fetchvars("r3", (1795, 1800)),
                ensemble.midpit(core.fetchvars("global_tas", (1795, 1800)), kind="numerator"))
    core.shutdown()
    # a core of two shards on one device
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    two = _core(2 * 64 + 5, hip_lib, pair_limit=0, devices=[0, 0])
    two.run(1800)
    two.hold("kept", "global_tas")
    data = two.fetchvars("global_tas", (1745, 1800))
    with pytest.raises(E, match="hx_series_rank.*several shards"):
        two.rank_series("r", "global_tas")
    with pytest.raises(E, match="hx_metric_ranks.*several shards"):
        two.metric_ranks("global_tas", [Metric("mean", (1750, 1760))])
    with pytest.raises(E, match="hx_ensemble_crps.*several shards"):
        two.crps("global_tas", [1750], [0.0])
    with pytest.raises(E, match="hx_series_rank.*several shards"):
        two.spearman("global_tas", "S")
    assert two.series() == {"kept": 1800}
    assert np.array_equal(data, two.fetchvars("global_tas", (1745, 1800)))
    two.shutdown()
