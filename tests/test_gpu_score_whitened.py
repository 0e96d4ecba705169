"""hx_member_score_whitened (Core.score with whiten=, cov=, ar1=) on the GPU.

Exact part: rows of integers 0..255 written through the device pointer of Core.device_var, integer
observations 0..255, no baseline or a 4-year one (its mean a multiple of 1/4), W lower-triangular
integers in -3..3 with a non-zero diagonal and NaN everywhere above it.  |r| <= 511, |y| <= 3 * 256 * 511
< 2^19 in quarters, y^2 < 2^38 in sixteenths and chi2 < 2^46 in sixteenths: every product and every
partial sum, in any order, fused or not, is exactly representable, so chi2 must EQUAL an int64 numpy
reference.  A dropped or doubled year, a wrong tile edge, an entry of the upper triangle read, a
padding-lane leak or a neighbour's NaN changes an integer.  The padding lanes hold poison (NaN and
-1e300 alternately); member sorting is off, so lane order is member order.  The tile sizes and the
thresholds between the kernel's flavours are read from hx_dev_post.h.

Real trajectories: the authority is `checker`, written by the definition of include/hector_amd.h: r
in float64 (two IEEE subtractions, base by the sequential sum), y and chi2 in np.longdouble from the
float64 W, s_i = sum_k |W_ik r_k|.  Required: |chi2 - ref| <= (3 n + 8) 2^-53 sum_i s_i^2, which holds
for any order of the sums and any use of fused multiply-adds (each y_i within n u s_i, |y_i| <= s_i,
the square and the n additions of non-negative terms another (n + 1) u).

Against Core.score (W = diag(1 / sigma)): the two agree within the sum of both bounds; Core.score's
own distance from the exact sum of (W_ii r_i)^2 is (n + 5) u chi2 -- W_ii = fl(1 / sigma_i) and
fl(r / sigma) differ from r / sigma by u each (so their squares by 4 u between them), the square
rounds once and the n - 1 additions of non-negative terms add (n - 1) u.
"""
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import ensemble
from conftest import ROOT, SCENARIO
from test_gpu_quantiles import _write_row

pytestmark = pytest.mark.gpu

E = hector_amd.HectorAmdError
LD = np.longdouble
U = 2.0 ** -53
_HDR = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_post.h")).read()
TILE = int(re.search(r"^#define HXW_TILE (\d+)", _HDR, re.M).group(1))
ACC = int(re.search(r"^#define HXW_ACC (\d+)", _HDR, re.M).group(1))
NMAX = int(re.search(r"^#define HXW_MAX (\d+)", _HDR, re.M).group(1))
_launch = _HDR[_HDR.index("hipError_t hx_launch_score_whiten("):]
FLAVOURS = [(int(a), int(b)) for a, b in re.findall(r"HXW_CASE\((\d+), (\d+)\);", _launch)]   # (NT, MT)
assert len(FLAVOURS) >= 3 and all(nt * mt <= ACC for nt, mt in FLAVOURS) and FLAVOURS[-1][0] * TILE == NMAX


def _edges(values, lo, hi):
    return sorted({v + d for v in values for d in (-1, 0, 1) if lo <= v + d <= hi})


# the issue's sizes, and the -1 / 0 / +1 edges of: an output tile, every flavour's size, a wavefront's members
NS = sorted(set((1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 128, 129, 255, 256)) |
            set(_edges([TILE] + [nt * TILE for nt, _ in FLAVOURS], 1, NMAX)))
MEMBERS = sorted(set((1, 15, 16, 17, 63, 64, 65, 1023, 1025, 2051)) |
                 set(_edges([mt * TILE for _, mt in FLAVOURS], 1, 4096)))
ROWS = NMAX
Y0 = 1745
BASE = (Y0 + ROWS - 4, Y0 + ROWS - 1)
V1, V2 = "global_tas", "CO2_concentration"
_worst = {"ratio": 0.0}


def _core(n, hip_lib, pair_limit=None, sorting=None, params=None, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib, **kw)
    S, q10 = ensemble.ecs_q10(n) if params is None else params
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    if pair_limit is not None:
        c.set_pair_kernel_limit(pair_limit)
    if sorting is not None:
        c.set_member_sorting(sorting)
    return c


# ---- 1. the exact test -------------------------------------------------------------------------------

def _integer_rows(nm, seed):
    """[ROWS, nm] integers 0..255 as float64; NaN at the first member, the last member, the last
    member of a 16-tile and a whole 16-tile (all in rows every call scores), and at one member in a
    row that only the reference period reads."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (ROWS, nm)).astype(np.float64)
    if nm > 2:
        x[0, 0] = np.nan
        x[0, nm - 1] = np.nan
        x[ROWS - 3, nm // 2] = np.nan
    if nm > TILE:
        x[0, TILE - 1] = np.nan
    if nm >= 3 * TILE:
        x[0, TILE:2 * TILE] = np.nan
    return x


def _integer_w(n, rng):
    W = rng.integers(-3, 4, (n, n)).astype(np.float64)
    d = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], n)
    W[np.arange(n), np.arange(n)] = d
    Wint = np.tril(W).astype(np.int64)
    W[np.triu_indices(n, 1)] = np.nan
    return W, Wint


def _integer_reference(x, rows, obs, Wint, base_rows):
    """int64 throughout, in sixteenths: -> float64 chi2, NaN where the member has a NaN in a row read."""
    X = x[rows]
    bad = np.isnan(X).any(axis=0)
    r4 = 4 * (np.nan_to_num(X).astype(np.int64) - obs.astype(np.int64)[:, None])
    if base_rows is not None:
        B = x[base_rows[0]:base_rows[1] + 1]
        assert B.shape[0] == 4
        bad |= np.isnan(B).any(axis=0)
        r4 = r4 - np.nan_to_num(B).astype(np.int64).sum(axis=0)[None, :]
    y4 = Wint @ r4
    chi16 = (y4 * y4).sum(axis=0)
    assert int(np.abs(y4).max()) < 2 ** 31 and int(chi16.max()) < 2 ** 53
    out = chi16.astype(np.float64) / 16.0
    out[bad] = np.nan
    return out


@pytest.mark.parametrize("nm", MEMBERS)
def test_integer_rows_are_exact(hip_lib, nm):
    core = _core(nm, hip_lib, sorting=False)
    core.run(Y0 + ROWS - 1)
    assert np.array_equal(core.lane_of_member(), np.arange(nm))
    x = _integer_rows(nm, nm)
    poison = (np.nan, -1e300)
    for r in range(ROWS):
        _write_row(core, V1, Y0 + r, x[r], pad_value=poison[r & 1])
    assert np.array_equal(core.fetchvars(V1, (Y0, Y0 + ROWS - 1)), x, equal_nan=True)
    rng = np.random.default_rng(1000 + nm)
    calls = nans = 0
    for j, n in enumerate(NS):
        W, Wint = _integer_w(n, rng)
        obs = rng.integers(0, 256, n).astype(np.float64)
        orders = {"ascending": np.arange(n), "descending": np.arange(n)[::-1].copy(), "shuffled": rng.permutation(n)}
        if n >= 2:
            orders["shuffled"][1] = orders["shuffled"][0]        # a repeated year
        for k, (name, rows) in enumerate(orders.items()):
            if 0 not in rows:
                rows[-1] = 0                                     # (every call reads the row that holds the NaNs)
            base = (None, BASE)[(j + k) & 1]
            got = core.score(V1, Y0 + rows, obs, baseline=base, whiten=W)
            ref = _integer_reference(x, rows, obs, Wint, None if base is None else (ROWS - 4, ROWS - 1))
            assert got.shape == (nm,) and np.array_equal(got, ref, equal_nan=True), \
                (nm, n, name, base, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5].ravel(),
                 got[:4], ref[:4])
            calls += 1
            nans += int(np.isnan(ref).sum())
    if nm > 2:
        assert nans > 0
    print("members = %d: %d calls over n in %s, %d NaN results" % (nm, calls, NS, nans))
    core.shutdown()


# ---- the longdouble checker ----------------------------------------------------------------------------

def checker(x, y0, years, obs, W, baseline=None):
    """x[year - y0, member] -> (chi2_ref, sum_i s_i^2), both longdouble [members]."""
    years = np.asarray(years)
    X = x[years - y0]
    if baseline is not None:
        s = np.zeros(x.shape[1])
        for y in range(baseline[0], baseline[1] + 1):
            s = s + x[y - y0]
        base = s / float(baseline[1] - baseline[0] + 1)
        r = (X - base[None, :]) - np.asarray(obs)[:, None]
    else:
        r = X - np.asarray(obs)[:, None]
    Wl = np.tril(np.nan_to_num(np.asarray(W, dtype=np.float64))).astype(LD)
    rl = r.astype(LD)
    y = Wl @ rl
    s = np.abs(Wl) @ np.abs(rl)
    return (y * y).sum(axis=0), (s * s).sum(axis=0)


def check_against(got, ref, s2, n, what, extra=0):
    err = np.abs(got.astype(LD) - ref)
    bound = (3 * n + 8 + extra) * LD(U) * s2
    assert np.isfinite(got).all() and (s2 > 0).all(), what
    worst = float(np.max(err / bound))
    print("%s: worst error / bound %.3g" % (what, worst))
    assert (err <= bound).all(), (what, worst, np.argwhere(err > bound)[:5].ravel())
    if not extra:
        _worst["ratio"] = max(_worst["ratio"], worst)


def _ar1(years, sigma, rho):
    years = np.asarray(years)
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), years.shape)
    return s[:, None] * s[None, :] * rho ** np.abs(years[:, None] - years[None, :])


def _pseudo_obs(x, y0, years, member, sigma, rho, seed, baseline=None):
    """A held-out member's trajectory plus seeded AR(1) noise."""
    rng = np.random.default_rng(seed)
    e = np.zeros(len(years))
    for i in range(len(years)):
        e[i] = (rho * e[i - 1] if i else 0.0) + rng.normal() * sigma * (np.sqrt(1 - rho * rho) if i else 1.0)
    t = x[np.asarray(years) - y0, member]
    if baseline is not None:
        t = t - x[baseline[0] - y0:baseline[1] - y0 + 1, member].mean()
    return t + e


# ---- 2., 3., 5. and 6.: real trajectories ----------------------------------------------------------------

@pytest.fixture(scope="module")
def real(hip_lib):
    core = _core(777, hip_lib)
    core.run(2105)
    data = {v: core.fetchvars(v, (1745, 2105)) for v in (V1, V2, "slr")}
    yield core, data
    core.shutdown()


@pytest.mark.parametrize("var,baseline,sigma", [(V1, (1850, 1900), 0.1), (V2, None, 1.5)])
def test_real_trajectories(real, var, baseline, sigma):
    core, data = real
    x = data[var]
    for years in (np.arange(1850, 2015), np.arange(1850, 2106)):
        n = len(years)
        assert n in (165, 256)
        W, logdet = hector_amd.whiten(_ar1(years, sigma, 0.6))
        obs = _pseudo_obs(x, 1745, years, 5, sigma, 0.6, n, baseline)
        got = core.score(var, years, obs, baseline=baseline, whiten=W)
        ref, s2 = checker(x, 1745, years, obs, W, baseline)
        check_against(got, ref, s2, n, (var, n))
        assert np.array_equal(got, core.score(var, years, obs, baseline=baseline, whiten=W))
        # the keywords are three spellings of one call
        C = _ar1(years, sigma, 0.6)
        a, used = core.score(var, years, obs, baseline=baseline, cov=C, return_used=True)
        assert used == n and np.array_equal(a, got)
        assert np.array_equal(core.score(var, years, obs, sigma=sigma, baseline=baseline, ar1=0.6), got)
        # a shuffled record with W of the shuffled covariance: the same chi2 within both bounds
        p = np.random.default_rng(n).permutation(n)
        Wp = hector_amd.whiten(_ar1(years[p], sigma, 0.6))[0]
        b = core.score(var, years[p], obs[p], baseline=baseline, whiten=Wp)
        refp, s2p = checker(x, 1745, years[p], obs[p], Wp, baseline)
        check_against(b, refp, s2p, n, (var, n, "shuffled"))


@pytest.mark.parametrize("sigma_kind", ["per year", "one"])
def test_a_diagonal_w_against_core_score(real, sigma_kind):
    core, data = real
    years = np.arange(1850, 2015)
    n = len(years)
    for var, baseline in ((V1, (1850, 1900)), (V2, None)):
        x = data[var]
        sigma = np.ones(n) if sigma_kind == "one" else 0.05 + 0.003 * np.arange(n)
        obs = _pseudo_obs(x, 1745, years, 9, 0.1, 0.0, 3, baseline)
        W = np.diag(1.0 / sigma)
        got = core.score(var, years, obs, baseline=baseline, whiten=W)
        old = core.score(var, years, obs, sigma=None if sigma_kind == "one" else sigma, baseline=baseline)
        ref, s2 = checker(x, 1745, years, obs, W, baseline)
        check_against(got, ref, s2, n, (var, sigma_kind, "whitened"))
        check_against(old, ref, s2, n, (var, sigma_kind, "Core.score against the checker"), extra=-(3 * n + 8) + n + 5)
        assert (np.abs(got.astype(LD) - old.astype(LD)) <= ((3 * n + 8) + (n + 5)) * LD(U) * s2).all()


def test_sources_held_derived_and_slr(real):
    core, data = real
    years = np.arange(1900, 2001)
    n = len(years)
    core.hold("sw_held", V1)
    core.derive("sw_anom", "anomaly", V1, years=(1850, 1900))
    try:
        anom = core.fetchvars("sw_anom", (1745, 2105))
        W = hector_amd.whiten(_ar1(years, 0.1, 0.6))[0]
        for var, x, baseline in (("sw_held", data[V1], (1850, 1900)), ("sw_anom", anom, None), ("slr", data["slr"], (1900, 1920))):
            assert np.isfinite(x[years - 1745]).all(), var
            obs = _pseudo_obs(x, 1745, years, 11, 0.1, 0.6, 5, baseline)
            got = core.score(var, years, obs, baseline=baseline, whiten=W)
            ref, s2 = checker(x, 1745, years, obs, W, baseline)
            check_against(got, ref, s2, n, (var, n))
        assert np.array_equal(core.score("sw_held", years, np.zeros(n), whiten=W),
                              core.score(V1, years, np.zeros(n), whiten=W))
    finally:
        core.drop_series("sw_held")
        core.drop_series("sw_anom")


def test_ar1_with_a_nan_observation_in_the_middle(real):
    core, data = real
    years = np.arange(1850, 2015)
    n = len(years)
    sigma = 0.08 + 0.0005 * np.arange(n)
    obs = _pseudo_obs(data[V1], 1745, years, 7, 0.1, 0.6, 6, (1850, 1900))
    obs[n // 2] = np.nan
    keep = ~np.isnan(obs)
    got, used = core.score(V1, years, obs, sigma=sigma, baseline=(1850, 1900), ar1=0.6, return_used=True)
    Wsub = hector_amd.whiten(_ar1(years, sigma, 0.6)[np.ix_(keep, keep)])[0]
    want = core.score(V1, years[keep], obs[keep], baseline=(1850, 1900), whiten=Wsub)
    assert used == n - 1 and np.isfinite(got).all() and np.array_equal(got, want)
    with pytest.raises(E, match="a NaN observation cannot be skipped under whiten"):
        core.score(V1, years, obs, baseline=(1850, 1900), whiten=np.eye(n))
    # (for the record: the independent score counts the evidence several times over)
    ind = core.score(V1, years[keep], obs[keep], sigma=sigma[keep], baseline=(1850, 1900))

    def ess(chi):
        w = np.exp(-0.5 * (chi - chi.min()))
        return w.sum() ** 2 / (w * w).sum()
    print("effective sample size: independent %.1f, AR(1) %.1f of %d" % (ess(ind), ess(got), core.n_members))


# ---- 4. one member, any company --------------------------------------------------------------------------

def test_a_members_chi2_does_not_depend_on_its_company(hip_lib):
    """Written rows (the same doubles in every core by construction): sorting on and off, and the
    ensemble cut to its first 100 members."""
    nm, rows = 1029, 70
    rng = np.random.default_rng(4)
    x = rng.normal(size=(rows, nm)) * 3.0 + 280.0
    x[5, 40] = np.nan                                   # a NaN member among the first 100, and one beyond
    x[6, 500] = np.nan
    years = Y0 + rng.permutation(rows)[:66]
    n = len(years)
    obs = rng.normal(size=n) + 280.0
    W = hector_amd.whiten(_ar1(years, 0.7, 0.6))[0]
    S, q10 = ensemble.ecs_q10(nm)
    res = {}
    for name, members, sorting in (("sorted", nm, True), ("unsorted", nm, False), ("cut", 100, True), ("cut unsorted", 100, False)):
        core = _core(members, hip_lib, sorting=sorting, params=(S[:members], q10[:members]))
        core.run(Y0 + rows - 1)
        for r in range(rows):
            _write_row(core, V1, Y0 + r, x[r, :members], pad_value=(np.nan, -1e300)[r & 1])
        assert np.array_equal(core.fetchvars(V1, (Y0, Y0 + rows - 1)), x[:, :members], equal_nan=True)
        a = core.score(V1, years, obs, baseline=(Y0 + 60, Y0 + 69), whiten=W)
        assert np.array_equal(a, core.score(V1, years, obs, baseline=(Y0 + 60, Y0 + 69), whiten=W), equal_nan=True)
        res[name] = a
        if name == "sorted":
            print("lanes permuted by the sorting: %s" % (not np.array_equal(core.lane_of_member(), np.arange(nm))))
            ref, s2 = checker(np.nan_to_num(x, nan=280.0), Y0, years, obs, W, (Y0 + 60, Y0 + 69))
            ok = ~np.isnan(a)
            check_against(a[ok], ref[ok], s2[ok], n, ("written rows", n))
        core.shutdown()
    assert np.isnan(res["sorted"][[40, 500]]).all() and np.isnan(res["sorted"]).sum() == 2
    assert np.array_equal(res["sorted"], res["unsorted"], equal_nan=True)
    assert np.array_equal(res["cut"], res["sorted"][:100], equal_nan=True)
    assert np.array_equal(res["cut unsorted"], res["sorted"][:100], equal_nan=True)


def test_shards_on_one_device_give_the_same_bits(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    nm = 1029
    years = np.arange(1760, 1900)
    n = len(years)
    W = hector_amd.whiten(_ar1(years, 0.1, 0.6))[0]
    res = []
    for shards in (1, 2, 3):
        core = _core(nm, hip_lib, pair_limit=0, devices=[0] * shards)
        core.run(1900)
        x = core.fetchvars(V1, (1745, 1900))
        if not res:
            obs = _pseudo_obs(x, 1745, years, 3, 0.1, 0.6, 8, (1745, 1760))
        a = core.score(V1, years, obs, baseline=(1745, 1760), whiten=W)
        assert np.array_equal(a, core.score(V1, years, obs, baseline=(1745, 1760), whiten=W))
        ref, s2 = checker(x, 1745, years, obs, W, (1745, 1760))
        check_against(a, ref, s2, n, ("shards", shards))
        res.append((x, a))
        core.shutdown()
    for x, a in res[1:]:
        assert np.array_equal(x, res[0][0])             # (the same trajectories, as tests/test_gpu_quantiles.py holds)
        assert np.array_equal(a, res[0][1])


def test_zz_report():
    print("hx_member_score_whitened: worst error / bound over this module %.3g" % _worst["ratio"])
    assert _worst["ratio"] <= 1.0
