"""hx_ensemble_comoments (Core.comoments) on the GPU.

Exact part: integer rows 0..4095 written through the device pointer of Core.device_var, weights None
(q = 1) or drawn from {1, 1/2, 1/4, 0} (q = 2^32, 2^31, 2^30, 0).  Every product q d_a d_b and every
partial sum is then an integer below 2^53 times a power of two -- exactly representable, whatever the
order -- so cross, sums_a, sums_b, wsum, n_part and the shifts must EQUAL a pure-integer numpy
reference: a dropped or doubled member, a wrong tile edge, a mis-mirrored block or a padding-lane leak
changes an integer.  The padding lanes hold poison (NaN and -1e300 alternately); member sorting is
off, so lane order is member order and 'the last lane of a chunk' is a member index.  RT (rows of a
workgroup's tile) and MC (its member chunk) are read from hx_dev_post.h.

Real trajectories: the authority is `checker` below, written by the definition of
include/hector_amd.h: complete cases, shifts as exact minima, d in float64 (one IEEE subtraction),
sums in np.longdouble.  |S - S_ref| <= (n_part + 8) 2^-53 S_ref for every sum: every term is >= 0.
Two layouts of the same members (shards, lane orders, the symmetric against the explicit call) agree
within twice that bound.
"""
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import ROOT, SCENARIO
from test_gpu_quantiles import _write_row
from test_gpu_moments import quantise, _score_weights

pytestmark = pytest.mark.gpu

E = hector_amd.HectorAmdError
LD = np.longdouble
U = 2.0 ** -53
_HDR = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_post.h")).read()
RT = int(re.search(r"^#define HXC_TILE (\d+)", _HDR, re.M).group(1))
MC = int(re.search(r"^#define HXC_CHUNK (\d+)", _HDR, re.M).group(1))
ROWS = 2 * RT + 1
SIZES = (1, 15, 16, 17, RT - 1, RT, RT + 1, 2 * RT + 1)
MEMBERS = (1, 63, 64, 65, MC - 1, MC, MC + 1, 2 * MC + 3)
Y0 = 1745
V1, V2 = "global_tas", "CO2_concentration"
_worst = {"ratio": 0.0}


def _core(n, hip_lib, pair_limit=None, sorting=None, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    if pair_limit is not None:
        c.set_pair_kernel_limit(pair_limit)
    if sorting is not None:
        c.set_member_sorting(sorting)
    return c


def _q(n, weights):
    return np.ones(n, dtype=np.uint64) if weights is None else quantise(np.asarray(weights, dtype=np.float64))


# ---- 1. the exact test -------------------------------------------------------------------------------

def _integer_rows(n, seed):
    """[ROWS, n] integers 0..4095 as float64, NaN scattered: the first and the last member, the last
    lane of a chunk, a whole chunk (where n has one to spare), single members in single rows."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4096, (ROWS, n)).astype(np.float64)
    # (the members differ from variable to variable: some are NaN in A only, some in B only, some in both)
    first, last, mid = {0}, {n - 1}, {(n // 2 + seed) % n}
    nan = {1: first | (last if seed == 3 else set()), RT: last if seed != 1 else mid, ROWS - 1: mid}
    if n >= MC:
        nan[3] = {MC - 1} if seed != 2 else {MC - 2}
    if n >= 2 * MC and seed != 2:
        nan[RT + 2] = set(range(MC, 2 * MC))
    if n <= 2:                       # (one member: keep it)
        nan = {}
    for row, members in nan.items():
        x[(row * (seed + 1)) % ROWS, sorted(members)] = np.nan
    return x


def _integer_reference(xa, xb, q):
    """Pure integers: shifts, sums and cross with q / min(q > 0) folded out as a power of two."""
    na, nb = xa.shape[0], xb.shape[0]
    part = (q > 0) & ~np.isnan(xa).any(axis=0) & ~np.isnan(xb).any(axis=0)
    if not part.any():
        return dict(n_part=0, wsum=0, shift_a=np.full(na, np.nan), shift_b=np.full(nb, np.nan),
                    sums_a=np.zeros((na, 2)), sums_b=np.zeros((nb, 2)), cross=np.zeros((na, nb)))
    qi = [int(v) for v in q[part]]
    unit = min(qi)                                      # 1 or 2^30 .. 2^32: a power of two
    assert unit & (unit - 1) == 0
    k = np.array([v // unit for v in qi], dtype=np.int64)   # 1, 2 or 4
    A, B = xa[:, part].astype(np.int64), xb[:, part].astype(np.int64)
    ca, cb = A.min(axis=1), B.min(axis=1)
    da, db = A - ca[:, None], B - cb[:, None]
    kda = k * da
    cross = kda @ db.T
    sa = np.stack([kda.sum(axis=1), (kda * da).sum(axis=1)], axis=1)
    sb = np.stack([(k * db).sum(axis=1), (k * db * db).sum(axis=1)], axis=1)
    assert max(int(cross.max()), int(sa.max()), int(sb.max())) < 2 ** 53
    f = float(unit)
    return dict(n_part=int(part.sum()), wsum=sum(qi), shift_a=ca.astype(np.float64), shift_b=cb.astype(np.float64),
                sums_a=sa.astype(np.float64) * f, sums_b=sb.astype(np.float64) * f, cross=cross.astype(np.float64) * f)


def _equal(cm, ref, what):
    assert cm.n_part == ref["n_part"], (what, "n_part", cm.n_part, ref["n_part"])
    assert cm.wsum == ref["wsum"], (what, "wsum")
    for f in ("shift_a", "shift_b", "sums_a", "sums_b", "cross"):
        got = getattr(cm, f)
        assert got.shape == ref[f].shape and np.array_equal(got, ref[f], equal_nan=True), \
            (what, f, np.argwhere(~((got == ref[f]) | (np.isnan(got) & np.isnan(ref[f]))))[:5])


def _exact_core(n, hip_lib):
    c = _core(n, hip_lib, sorting=False)
    c.run(Y0 + ROWS - 1)
    assert np.array_equal(c.lane_of_member(), np.arange(n))
    data = {}
    poison = (np.nan, -1e300)
    x3 = _integer_rows(n, 3)
    for r in range(ROWS):
        _write_row(c, V1, Y0 + r, x3[r], pad_value=poison[r & 1])
    c.hold("held", V1)
    data["held"] = x3
    for var, seed in ((V1, 1), (V2, 2)):
        data[var] = _integer_rows(n, seed)
        for r in range(ROWS):
            _write_row(c, var, Y0 + r, data[var][r], pad_value=poison[(r + seed) & 1])
    for var in data:
        assert np.array_equal(c.fetchvars(var, (Y0, Y0 + ROWS - 1)), data[var], equal_nan=True)
    return c, data


@pytest.mark.parametrize("n", MEMBERS)
def test_integer_rows_are_exact(hip_lib, n):
    core, data = _exact_core(n, hip_lib)
    rng = np.random.default_rng(n)
    w = rng.choice([1.0, 0.5, 0.25, 0.0], n)
    w[0] = 1.0
    # every pair of sizes at the largest ensemble; elsewhere every size once in each role
    pairs = [(a, b) for a in SIZES for b in SIZES] if n == MEMBERS[-1] else \
        [(SIZES[i], SIZES[(i + 3) % len(SIZES)]) for i in range(len(SIZES))]
    kinds = ((V1, V1), (V1, V2), ("held", V2), (V2, "held"))   # overlapping windows; two variables; a series
    calls = 0
    for weights in (None, w):
        q = _q(n, weights)
        for i, (na, nb) in enumerate(pairs):
            va, vb = kinds[(i + i // len(SIZES)) % len(kinds)]
            ra, rb = (i * 7) % (ROWS - na + 1), (ROWS - nb) - (i * 5) % (ROWS - nb + 1)
            if va == vb:                                  # overlapping windows of one variable
                rb = min(ra + na // 2, ROWS - nb)
            cm = core.comoments(va, (Y0 + ra, Y0 + ra + na - 1), vb, (Y0 + rb, Y0 + rb + nb - 1), weights=weights)
            assert not cm.symmetric and cm.years_a[0] == Y0 + ra and cm.years_b[-1] == Y0 + rb + nb - 1
            _equal(cm, _integer_reference(data[va][ra:ra + na], data[vb][rb:rb + nb], q),
                   (n, na, nb, va, vb, ra, rb, weights is not None))
            calls += 1
        for i, na in enumerate(SIZES):                    # the symmetric call
            var = (V1, V2, "held")[i % 3]
            ra = (i * 11) % (ROWS - na + 1)
            cm = core.comoments(var, (Y0 + ra, Y0 + ra + na - 1), weights=weights)
            x = data[var][ra:ra + na]
            _equal(cm, _integer_reference(x, x, q), (n, na, "symmetric", var, weights is not None))
            assert cm.symmetric and np.array_equal(cm.cross, cm.cross.T)
            assert np.array_equal(cm.sums_a[:, 1], np.diag(cm.cross)) and np.array_equal(cm.sums_a, cm.sums_b)
    # n_part drops by exactly the members that are NaN in a row of A only, of B only, of both
    if n > 2:
        xa, xb = data[V1], data[V2]
        lost = np.isnan(xa).any(axis=0) | np.isnan(xb).any(axis=0)
        only_a, only_b = np.isnan(xa).any(axis=0) & ~np.isnan(xb).any(axis=0), np.isnan(xb).any(axis=0) & ~np.isnan(xa).any(axis=0)
        assert only_a.any() and only_b.any()
        cm = core.comoments(V1, (Y0, Y0 + ROWS - 1), V2, (Y0, Y0 + ROWS - 1))
        assert cm.n_part == n - int(lost.sum())
    print("n = %d: %d cross calls, %d symmetric" % (n, calls, 2 * len(SIZES)))
    core.shutdown()


# ---- the longdouble checker ----------------------------------------------------------------------------

def checker(xa, xb, q):
    part = (q > 0) & ~np.isnan(xa).any(axis=0) & ~np.isnan(xb).any(axis=0)
    na, nb = xa.shape[0], xb.shape[0]
    if not part.any():
        return dict(n_part=0, wsum=0, shift_a=np.full(na, np.nan), shift_b=np.full(nb, np.nan),
                    sums_a=np.zeros((na, 2), dtype=LD), sums_b=np.zeros((nb, 2), dtype=LD),
                    cross=np.zeros((na, nb), dtype=LD))
    w = q[part].astype(LD)
    ca, cb = xa[:, part].min(axis=1), xb[:, part].min(axis=1)
    da = (xa[:, part] - ca[:, None]).astype(LD)           # float64: one IEEE subtraction
    db = (xb[:, part] - cb[:, None]).astype(LD)
    wda = w * da
    return dict(n_part=int(part.sum()), wsum=sum(int(v) for v in q[part]), shift_a=ca, shift_b=cb,
                sums_a=np.stack([wda.sum(axis=1), (wda * da).sum(axis=1)], axis=1),
                sums_b=np.stack([(w * db).sum(axis=1), (w * db * db).sum(axis=1)], axis=1), cross=wda @ db.T)


def check_against(cm, ref, what):
    assert cm.n_part == ref["n_part"] and cm.wsum == ref["wsum"], what
    assert np.array_equal(cm.shift_a, ref["shift_a"], equal_nan=True), (what, "shift_a")
    assert np.array_equal(cm.shift_b, ref["shift_b"], equal_nan=True), (what, "shift_b")
    worst = 0.0
    for f in ("sums_a", "sums_b", "cross"):
        r = ref[f]
        err = np.abs(getattr(cm, f).astype(LD) - r)
        bound = (cm.n_part + 8) * LD(U) * r
        worst = max(worst, float(np.max(np.where(r > 0, err / np.where(r > 0, bound, 1), 0))))
        assert (err <= bound).all(), (what, f, worst, np.argwhere(err > bound)[:5])
    _worst["ratio"] = max(_worst["ratio"], worst)
    print("%s: worst sum error / bound %.3g" % (what, worst))


def same_bits(a, b):
    return (a.n_part == b.n_part and a.wsum == b.wsum and
            all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True)
                for f in ("shift_a", "shift_b", "sums_a", "sums_b", "cross")))


def within_twice(a, b, what):
    """Two layouts of the same members: the exact fields equal, the sums within twice the bound."""
    assert a.n_part == b.n_part and a.wsum == b.wsum, what
    assert np.array_equal(a.shift_a, b.shift_a, equal_nan=True) and np.array_equal(a.shift_b, b.shift_b, equal_nan=True), what
    for f in ("sums_a", "sums_b", "cross"):
        x, y = getattr(a, f), getattr(b, f)
        assert (np.abs(x - y) <= 2 * (a.n_part + 8) * U * np.maximum(x, y)).all(), (what, f)


# ---- 2. and 3. real trajectories -----------------------------------------------------------------------

@pytest.mark.parametrize("n,pair_limit,kernel", [(1000, None, "pair"), (3000, 0, "run")])
def test_real_trajectories(hip_lib, n, pair_limit, kernel):
    core = _core(n, hip_lib, pair_limit=pair_limit)
    core.run(2100)
    assert core.last_run_kernel() == kernel
    w = _score_weights(core)
    assert (quantise(w) == 0).any() and (quantise(w) > 0).sum() > 10
    tas = core.fetchvars("global_tas", (1850, 2100))
    slr = core.fetchvars("slr", (2050, 2100))
    for weights in (None, w):
        q = _q(n, weights)
        what = (kernel, "weighted" if weights is not None else "unweighted")
        sym = core.comoments("global_tas", (1850, 2100), weights=weights)
        check_against(sym, checker(tas, tas, q), what + ("symmetric",))
        assert same_bits(sym, core.comoments("global_tas", (1850, 2100), weights=weights))
        assert np.array_equal(sym.cross, sym.cross.T) and np.array_equal(sym.sums_a[:, 1], np.diag(sym.cross))
        assert np.array_equal(sym.years_a, np.arange(1850, 2101)) and sym.cross.shape == (251, 251)
        # the explicit call of the same window against itself: every block computed, nothing mirrored
        within_twice(sym, core.comoments("global_tas", (1850, 2100), "global_tas", (1850, 2100), weights=weights),
                     what + ("symmetric against explicit",))
        cr = core.comoments("global_tas", (1980, 2020), "slr", (2050, 2100), weights=weights)
        assert cr.cross.shape == (41, 51) and not cr.symmetric
        check_against(cr, checker(tas[130:171], slr, q), what + ("tas x slr",))
        assert same_bits(cr, core.comoments("global_tas", (1980, 2020), "slr", (2050, 2100), weights=weights))
        # the shipped verb: one B year as a predictor of Core.moments (the same shift: the smallest
        # participating value of that year; nothing here is NaN, so the participants coincide)
        j = 33
        m = core.moments("global_tas", (1980, 2020), weights=weights, against=[("slr", Metric("mean", 2050 + j))])
        assert m.pshift[0] == cr.shift_b[j] and (m.n_part == cr.n_part).all() and np.array_equal(m.shift, cr.shift_a)
        ek = m.sums[:, 4]
        assert (np.abs(ek - cr.cross[:, j]) <= 2 * (cr.n_part + 8) * U * np.maximum(ek, cr.cross[:, j])).all()
        val, share, pat = sym.pca(3)
        assert (val > 0).all() and (np.diff(val) <= 0).all() and 0 < share.sum() <= 1.0 + 1e-9 and pat.shape == (3, 251)
    core.shutdown()


# ---- 4. a sharded core ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_core_against_one_core(hip_lib, monkeypatch, shards):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    n = shards * 512 + 5
    one = _core(n, hip_lib, pair_limit=0)
    many = _core(n, hip_lib, pair_limit=0, devices=[0] * shards)
    for c in (one, many):
        c.run(1900, wait=False)
    tas = one.fetchvars("global_tas", (1745, 1900))
    co2 = one.fetchvars("CO2_concentration", (1745, 1900))
    assert np.array_equal(tas, many.fetchvars("global_tas", (1745, 1900)))
    rng = np.random.default_rng(shards)
    w = rng.random(n) ** 12
    w[:700] = 0.0                    # zeroes whole shards (the first of two, more of eight)
    w[n - 1] = 5.0                   # the largest weight lives on the last shard
    for weights in (None, w):
        q = _q(n, weights)
        for args, xa, xb in ((("global_tas", (1760, 1900)), tas[15:], tas[15:]),
                             (("global_tas", (1800, 1870), "CO2_concentration", (1850, 1900)), tas[55:126], co2[105:])):
            a, b = one.comoments(*args, weights=weights), many.comoments(*args, weights=weights)
            within_twice(a, b, (shards, args, weights is not None))
            ref = checker(xa, xb, q)
            check_against(a, ref, ("one", shards, len(args), weights is not None))
            check_against(b, ref, ("many", shards, len(args), weights is not None))
            assert same_bits(b, many.comoments(*args, weights=weights))
            if len(args) == 2:
                assert np.array_equal(b.cross, b.cross.T) and np.array_equal(b.sums_a[:, 1], np.diag(b.cross))
    one.shutdown(); many.shutdown()


# ---- 5. lane order -------------------------------------------------------------------------------------

def test_member_sorting_on_and_off(hip_lib):
    res = []
    for sorting in (True, False):
        core = _core(3000, hip_lib, pair_limit=0, sorting=sorting)
        core.run(1900)
        rng = np.random.default_rng(11)
        w = rng.random(3000) ** 8
        x = core.fetchvars("global_tas", (1760, 1900))
        y = core.fetchvars("CO2_concentration", (1850, 1900))
        s = core.comoments("global_tas", (1760, 1900), weights=w)
        c = core.comoments("global_tas", (1760, 1900), "CO2_concentration", (1850, 1900), weights=w)
        check_against(s, checker(x, x, _q(3000, w)), ("sorting", sorting, "symmetric"))
        check_against(c, checker(x, y, _q(3000, w)), ("sorting", sorting, "cross"))
        res.append((x, y, s, c))
        core.shutdown()
    if np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]):
        within_twice(res[0][2], res[1][2], "sorting on against off, symmetric")
        within_twice(res[0][3], res[1][3], "sorting on against off, cross")


# ---- 6. every documented error -------------------------------------------------------------------------

def test_every_documented_error_and_nothing_changes(hip_lib):
    n = 512
    fn = "hx_ensemble_comoments"
    fresh = _core(n, hip_lib)
    with pytest.raises(E, match=fn + ".*run the core first"):
        fresh.comoments("global_tas", (1745, 1745))
    fresh.shutdown()
    core = _core(n, hip_lib, sorting=False)
    core.run(1850)
    core.hold("held", "global_tas")
    before = core.fetchvars("global_tas", (1745, 1850))
    status, ms = core.status(), core.last_run_ms()
    good = core.comoments("global_tas", (1745, 1850), "held", (1800, 1850))
    w = np.ones(n)
    for bad in (np.where(np.arange(n) == 3, -1.0, w), np.where(np.arange(n) == 3, np.nan, w),
                np.where(np.arange(n) == 3, np.inf, w), np.zeros(n)):
        with pytest.raises(E, match=fn):
            core.comoments("global_tas", weights=bad)
    for dates in ((1745, 1851), (1700, 1800)):
        with pytest.raises(E, match=fn + ".*current date"):
            core.comoments("global_tas", dates)
        with pytest.raises(E, match=fn + ".*current date"):
            core.comoments("global_tas", (1800, 1850), "held", dates)
    with pytest.raises(E, match=fn + ".*not enabled"):
        core.comoments("RF_tot")
    with pytest.raises(E, match=fn + ".*not enabled"):
        core.comoments("global_tas", (1800, 1850), "RF_tot", (1800, 1850))
    with pytest.raises(E, match=fn):
        core.comoments("no_such_variable")
    with pytest.raises(E, match=fn):
        core.comoments("global_tas", None, "no_such_variable", None)
    again = core.comoments("global_tas", (1745, 1850), "held", (1800, 1850))
    assert same_bits(good, again)
    # var = 0: the rows of global_tas before 1751 are all-equal rows
    assert (good.var_a[:6] == 0).all() and np.isnan(good.corr[:6]).all() and (good.slope[:6] == 0).all()
    assert np.isfinite(good.corr[10:]).all() and np.isfinite(good.slope[10:]).all()
    sym = core.comoments("global_tas", (1745, 1850))
    assert np.isnan(sym.corr[:6]).all() and np.isnan(sym.corr[:, :6]).all() and np.isnan(sym.slope[:, :6]).all()
    # nobody takes part: all the weight on members that are NaN somewhere in the window
    x = before[100].copy()
    x[::2] = np.nan
    _write_row(core, "global_tas", 1845, x, pad_value=np.nan)
    wn = np.where(np.arange(n) % 2 == 0, 1.0, 0.0)
    for args in (("global_tas", (1800, 1850)), ("held", (1800, 1850), "global_tas", (1840, 1850))):
        e = core.comoments(*args, weights=wn)
        assert e.n_part == 0 and e.wsum == 0 and np.isnan(e.shift_a).all() and np.isnan(e.shift_b).all()
        assert (e.cross == 0).all() and (e.sums_a == 0).all() and (e.sums_b == 0).all()
        assert np.isnan(e.cov).all() and np.isnan(e.corr).all() and np.isnan(e.slope).all() and np.isnan(e.mean_a).all()
        half = core.comoments(*args)
        assert half.n_part == n // 2
    _write_row(core, "global_tas", 1845, before[100], pad_value=np.nan)
    # the calls and the refused calls changed nothing
    assert same_bits(good, core.comoments("global_tas", (1745, 1850), "held", (1800, 1850)))
    assert np.array_equal(before, core.fetchvars("global_tas", (1745, 1850)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    core.run(1900)
    assert core.comoments("global_tas").cross.shape == (156, 156)
    core.shutdown()


def test_zz_report_the_worst_error():
    print("hx_ensemble_comoments: worst sum error / bound over this module %.3g" % _worst["ratio"])
    assert _worst["ratio"] <= 1.0
