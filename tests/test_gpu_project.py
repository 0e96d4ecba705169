"""hx_member_project (Core.project, CoMoments.scores) on the GPU.

Exact part: rows of integers 0..255 written through the device pointer of Core.device_var, an integer
centre 0..255, no baseline or a 4-year one (its mean a multiple of 1/4), a basis of integers in -3..3
with one all-zero row and one all-zero column.  |r| <= 510, i.e. 2040 quarters, and |out| <= 1024 * 3 *
2040 < 2^23 in quarters: every product and every partial sum, in any order, fused or not, is exactly
representable, so the result must EQUAL an int64 numpy reference.  A dropped or doubled year, a wrong
tile edge, a basis row or column shifted by one, a padding-lane leak or a neighbour's NaN changes an
integer.  The padding lanes hold poison (NaN and -1e300 alternately); member sorting is off, so lane
order is member order.  NaN is planted at the first and the last member, at a tile's last member and
in a whole 16-tile, all in the written row 0, which every call reads -- at the basis' all-zero COLUMN,
so that only 0 * NaN carries it -- and at one member in a row that only the reference period reads.
The tile sizes and the kernel's flavours are read from hx_dev_post.h.  The (n, m) pairs are cycled,
not crossed: the list below is extended until every n, every m and every (flavour, n mod 4) has
occurred, and every member count runs all of it.

Real trajectories: the authority is `checker`, written by the definition of include/hector_amd.h: r
in float64 (two IEEE subtractions, base by the sequential sum), products and sums in np.longdouble,
s_j = sum_k |basis[j, k] r_k|.  Required: |out - ref| <= (n + 2) 2^-53 s_j, which holds for any order
of the sum and any use of fused multiply-adds (the header gives the reason).

Against Metric("mean") over a window of n years (basis row fl(1 / n)): the metric is the sequential
sum and ONE division, within n u S / n of the exact mean E (n - 1 additions and the division; S = sum
|x|); the exact sum of fl(1 / n) x_k is within u S / n of E, and project within (n + 2) u s of that,
s = sum |fl(1 / n) x_k| = S / n (1 + u) at the most.  Together (2 n + 3) u s to first order; (2 n + 4)
u s is asked.

Against Core.score(whiten=W): chi2 there is within (3 n + 8) u sum s_i^2 of the exact sum of squares
(its header).  Here y_i is within (n + 2) u s_i and |y_i| <= s_i, so y_i^2 is within 2 (n + 2) u s_i^2
(to first order), the float64 square rounds once and numpy's n - 1 additions of non-negative terms
add (n - 1) u: (3 n + 4) u sum s_i^2, and one more for the second-order terms.
"""
import importlib.util
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
TILE = int(re.search(r"^#define HXP_TILE (\d+)", _HDR, re.M).group(1))
MT = int(re.search(r"^#define HXP_MT (\d+)", _HDR, re.M).group(1))
MAX_OUT = int(re.search(r"^#define HXP_MAX_OUT (\d+)", _HDR, re.M).group(1))
MAX_YEARS = int(re.search(r"^#define HXP_MAX_YEARS (\d+)", _HDR, re.M).group(1))
_launch = _HDR[_HDR.index("hipError_t hx_launch_project("):]
FLAVOURS = [int(a) for a in re.findall(r"HXP_CASE\((\d+)\);", _launch)]   # NT
assert FLAVOURS == list(range(1, MAX_OUT // TILE + 1)) and len(FLAVOURS) * MT <= 16


def _edges(values, lo, hi):
    return sorted({v + d for v in values for d in (-1, 0, 1) if lo <= v + d <= hi})


# the issue's sizes (its n are 0, 1 or 3 mod 4: 2, 6, 18, 66 and 1022 add the remainder 2), and the
# -1 / 0 / +1 edges of every flavour's outputs and of a wavefront's members
NS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 18, 63, 64, 65, 66, 255, 256, 257, 1022, 1023, 1024]
MS = sorted(set((1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)) | set(_edges([nt * TILE for nt in FLAVOURS], 1, MAX_OUT)))
MEMBERS = sorted(set((1, 15, 16, 17, 63, 64, 65, 1023, 1025, 2051)) | set(_edges([MT * TILE], 1, 4096)))
assert NS[-1] == MAX_YEARS and MS[-1] == MAX_OUT


def _pairs():
    """(n, m) cycled through NS and MS until every n, every m and every (flavour, n mod 4) has occurred."""
    need = {(nt, r) for nt in FLAVOURS for r in range(4)}
    out, seen = [], set()
    i = 0
    while i < max(len(NS), len(MS)) or seen != need:
        n, m = NS[i % len(NS)], MS[i % len(MS)]
        out.append((n, m))
        seen.add(((m + TILE - 1) // TILE, n % 4))
        i += 1
        assert i < 400
    assert {n for n, _ in out} == set(NS) and {m for _, m in out} == set(MS)
    # ... and the corners the cycle does not pair: the longest loops with the most accumulators
    return out + [(NS[-1], MS[-1]), (NS[-2], MS[-2]), (NS[-3], 3 * TILE + 1), (257, MS[-1]), (NS[-1], 1)]


PAIRS = _pairs()
ROWS = 256
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
    member of a 16-tile and a whole 16-tile (all in row 0, which every call reads), and at one member
    in a row that only the reference period reads."""
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


def _integer_reference(x, rows, center, Bint, base_rows):
    """int64 throughout, in quarters: -> float64 [m, members], NaN where the member has a NaN in a row read."""
    X = x[rows]
    bad = np.isnan(X).any(axis=0)
    r4 = 4 * (np.nan_to_num(X).astype(np.int64) - center.astype(np.int64)[:, None])
    if base_rows is not None:
        B = x[base_rows[0]:base_rows[1] + 1]
        assert B.shape[0] == 4
        bad |= np.isnan(B).any(axis=0)
        r4 = r4 - np.nan_to_num(B).astype(np.int64).sum(axis=0)[None, :]
    y4 = Bint @ r4
    assert int(np.abs(r4).max()) <= 2040 and int(np.abs(y4).max()) < 2 ** 23
    out = y4.astype(np.float64) / 4.0
    out[:, bad] = np.nan
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
    rng = np.random.default_rng(2000 + nm)
    nans = 0
    for i, (n, m) in enumerate(PAIRS):
        rows = rng.integers(0, ROWS, n)          # with repetition: n may exceed the rows written
        rows[rng.integers(0, n)] = 0             # (every call reads the row that holds the NaNs)
        order = ("ascending", "descending", "shuffled")[i % 3]
        if order == "ascending":
            rows = np.sort(rows)
        elif order == "descending":
            rows = np.sort(rows)[::-1].copy()
        elif n >= 3:
            rows[1] = rows[2]                    # (a repeated year, side by side, whatever else repeats)
            rows[0] = 0
        Bint = rng.integers(-3, 4, (m, n)).astype(np.int64)
        if m > 1:
            Bint[m // 2, :] = 0                  # the all-zero row
        if n > 1:
            Bint[:, int(np.argmax(rows == 0))] = 0   # the all-zero column: where the NaNs are read
        center = rng.integers(0, 256, n).astype(np.float64)
        base = (None, BASE)[(i // 3) & 1]
        got = core.project(V1, Y0 + rows, Bint.astype(np.float64), center=center, baseline=base)
        ref = _integer_reference(x, rows, center, Bint, None if base is None else (ROWS - 4, ROWS - 1))
        assert got.shape == (m, nm) and np.array_equal(got, ref, equal_nan=True), \
            (nm, n, m, order, base, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5],
             got[:2, :4], ref[:2, :4])
        nans += int(np.isnan(ref).sum())
    # center=None is - 0.0, and a one-dimensional basis gives one row
    rows = np.arange(ROWS)[::-1].copy()
    b = rng.integers(-3, 4, ROWS).astype(np.float64)
    got = core.project(V1, Y0 + rows, b)
    assert got.shape == (nm,)
    assert np.array_equal(got, _integer_reference(x, rows, np.zeros(ROWS), b.astype(np.int64)[None, :], None)[0], equal_nan=True)
    if nm > 2:
        assert nans > 0
    print("members = %d: %d calls, n up to %d, m up to %d, %d NaN results" % (nm, len(PAIRS) + 1, NS[-1], MS[-1], nans))
    core.shutdown()


# ---- the longdouble checker ----------------------------------------------------------------------------

def checker(x, y0, years, basis, center=None, baseline=None):
    """x[year - y0, member] -> (ref, s), both longdouble [m, members]."""
    years = np.asarray(years)
    X = x[years - y0]
    ce = np.zeros(len(years)) if center is None else np.asarray(center, dtype=np.float64)
    if baseline is not None:
        s = np.zeros(x.shape[1])
        for y in range(baseline[0], baseline[1] + 1):
            s = s + x[y - y0]
        base = s / float(baseline[1] - baseline[0] + 1)
        r = (X - base[None, :]) - ce[:, None]
    else:
        r = X - ce[:, None]
    Bl = np.atleast_2d(np.asarray(basis, dtype=np.float64)).astype(LD)
    rl = r.astype(LD)
    return Bl @ rl, np.abs(Bl) @ np.abs(rl)


def check_against(got, ref, s, n, what):
    got = np.atleast_2d(got)
    err = np.abs(got.astype(LD) - ref)
    bound = (n + 2) * LD(U) * s
    assert got.shape == ref.shape and np.isfinite(got).all() and (s > 0).all(), what
    worst = float(np.max(err / bound))
    print("%s: worst error / bound %.3g" % (what, worst))
    assert (err <= bound).all(), (what, worst, np.argwhere(err > bound)[:5])
    _worst["ratio"] = max(_worst["ratio"], worst)


# ---- 2., 3. and 6.: real trajectories ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def real(hip_lib):
    core = _core(777, hip_lib)
    core.run(2105)
    data = {v: core.fetchvars(v, (1745, 2105)) for v in (V1, V2, "slr")}
    yield core, data
    core.shutdown()


def _years(n, rng):
    """165: the instrumental period; more than the 361 years recorded: drawn with repetition."""
    return np.arange(1850, 2015) if n == 165 else rng.integers(1745, 2106, n)


@pytest.mark.parametrize("var,baseline", [(V1, (1850, 1900)), (V2, None)])
def test_real_trajectories(real, var, baseline):
    core, data = real
    x = data[var]
    rng = np.random.default_rng(11)
    for n in (165, 556):
        years = _years(n, rng)
        center = x[years - 1745].mean(axis=1) - (0.0 if baseline is None else x[105:156].mean())
        for m in (3, 16, 64):
            B = rng.normal(size=(m, n))
            got = core.project(var, years, B, center=center, baseline=baseline)
            ref, s = checker(x, 1745, years, B, center, baseline)
            check_against(got, ref, s, n, (var, n, m))
            assert np.array_equal(got, core.project(var, years, B, center=center, baseline=baseline))
        got = core.project(var, years, B[1], baseline=baseline)          # no centre, one row
        ref, s = checker(x, 1745, years, B[1], None, baseline)
        check_against(got, ref, s, n, (var, n, "no centre"))


def test_an_output_does_not_depend_on_the_other_rows(real):
    """Every D element of the matrix instruction is its own chain over k: a row's result is the same
    bits alone, in other company, at another position, in another tile and in another flavour."""
    core, data = real
    rng = np.random.default_rng(12)
    years = np.arange(1850, 2015)
    n = len(years)
    B = rng.normal(size=(64, n))
    center = data[V1][years - 1745].mean(axis=1)
    kw = dict(center=center, baseline=(1850, 1900))
    full = core.project(V1, years, B, **kw)
    ref, s = checker(data[V1], 1745, years, B, center, (1850, 1900))
    check_against(full, ref, s, n, "64 rows")
    for name, pick in (("row 0 alone", [0]), ("rows 5 and 40", [5, 40]), ("reversed", list(range(63, -1, -1))),
                       ("the first 17", list(range(17)))):
        part = core.project(V1, years, B[pick], **kw)
        assert part.shape == (len(pick), 777)
        assert np.array_equal(part, full[pick]), (name, np.argwhere(part != full[pick])[:5])
    assert np.array_equal(core.project(V1, years, B[7], **kw), full[7])


def test_sources_held_derived_and_slr(real):
    core, data = real
    years = np.arange(1900, 2001)
    n = len(years)
    rng = np.random.default_rng(13)
    B = rng.normal(size=(5, n))
    core.hold("pj_held", V1)
    core.derive("pj_anom", "anomaly", V1, years=(1850, 1900))
    try:
        anom = core.fetchvars("pj_anom", (1745, 2105))
        for var, x, baseline in (("pj_held", data[V1], (1850, 1900)), ("pj_anom", anom, None), ("slr", data["slr"], (1900, 1920))):
            assert np.isfinite(x[years - 1745]).all(), var
            center = x[years - 1745, 11] + 0.25            # (a member's own trajectory, shifted: no r is 0)
            got = core.project(var, years, B, center=center, baseline=baseline)
            ref, s = checker(x, 1745, years, B, center, baseline)
            check_against(got, ref, s, n, (var, n))
        assert np.array_equal(core.project("pj_held", years, B), core.project(V1, years, B))
    finally:
        core.drop_series("pj_held")
        core.drop_series("pj_anom")


@pytest.mark.parametrize("var", [V1, V2])
def test_a_row_of_one_nth_against_the_metric_mean(real, var):
    core, data = real
    y0, y1 = 1961, 1990
    years = np.arange(y0, y1 + 1)
    n = len(years)
    b = np.full(n, 1.0 / n)
    got = core.project(var, years, b)
    ref, s = checker(data[var], 1745, years, b)
    check_against(got, ref, s, n, (var, "1 / n"))
    mean = core.metrics(var, [hector_amd.Metric("mean", (y0, y1))])[0]
    gap = np.abs(got.astype(LD) - mean.astype(LD))
    print("%s: project(1 / n) against Metric mean: worst gap / bound %.3g" % (var, float(np.max(gap / ((2 * n + 4) * LD(U) * s[0])))))
    assert (gap <= (2 * n + 4) * LD(U) * s[0]).all()


def test_the_squares_of_a_triangular_basis_against_the_whitened_score(real):
    core, data = real
    years = np.arange(1941, 2001)
    n = len(years)
    assert n == 60
    C = 0.01 * 0.6 ** np.abs(years[:, None] - years[None, :])
    W = hector_amd.whiten(C)[0]
    rng = np.random.default_rng(14)
    obs = data[V1][years - 1745, 5] - data[V1][105:156, 5].mean() + rng.normal(size=n) * 0.1
    y = core.project(V1, years, np.tril(W), center=obs, baseline=(1850, 1900))
    ref, s = checker(data[V1], 1745, years, np.tril(W), obs, (1850, 1900))
    check_against(y, ref, s, n, "tril(W)")
    chi2 = core.score(V1, years, obs, baseline=(1850, 1900), whiten=W)
    mine = (y ** 2).sum(0)
    s2 = (s * s).sum(axis=0)
    gap = np.abs(mine.astype(LD) - chi2.astype(LD))
    bound = ((3 * n + 8) + (3 * n + 4) + 1) * LD(U) * s2
    print("sum of project(tril(W))^2 against score(whiten=W): worst gap / bound %.3g" % float(np.max(gap / bound)))
    assert (gap <= bound).all()


def test_comoments_scores_is_the_explicit_call(real):
    core, data = real
    co = core.comoments(V1, (1980, 2020))
    sc = co.scores(core, V1, 3)
    pat = co.pca(3)[2]
    explicit = core.project(V1, co.years_a, pat, center=co.mean_a)
    assert sc.shape == (3, 777) and np.array_equal(sc, explicit)
    ref, s = checker(data[V1], 1745, co.years_a, pat, co.mean_a)
    check_against(sc, ref, s, len(co.years_a), "PC scores")
    asym = core.comoments(V1, (1980, 2020), V2, (1980, 2020))
    with pytest.raises(E, match="needs a symmetric result"):
        asym.scores(core, V1, 3)


# ---- 4. one member, any company --------------------------------------------------------------------------

def test_a_members_projection_does_not_depend_on_its_company(hip_lib):
    """Written rows (the same doubles in every core by construction): sorting on and off, and the
    ensemble cut to its first 100 members."""
    nm, rows = 1029, 70
    rng = np.random.default_rng(4)
    x = rng.normal(size=(rows, nm)) * 3.0 + 280.0
    x[5, 40] = np.nan                                   # a NaN member among the first 100, and one beyond
    x[6, 500] = np.nan
    years = Y0 + rng.permutation(rows)[:66]
    n = len(years)
    center = rng.normal(size=n) + 280.0
    B = rng.normal(size=(19, n))
    B[:, [np.argmax(years == Y0 + 5), np.argmax(years == Y0 + 6)]] = 0.0     # (0 * NaN carries them)
    assert (years == Y0 + 5).any() and (years == Y0 + 6).any()
    S, q10 = ensemble.ecs_q10(nm)
    res = {}
    kw = dict(center=center, baseline=(Y0 + 60, Y0 + 69))
    for name, members, sorting in (("sorted", nm, True), ("unsorted", nm, False), ("cut", 100, True), ("cut unsorted", 100, False)):
        core = _core(members, hip_lib, sorting=sorting, params=(S[:members], q10[:members]))
        core.run(Y0 + rows - 1)
        for r in range(rows):
            _write_row(core, V1, Y0 + r, x[r, :members], pad_value=(np.nan, -1e300)[r & 1])
        assert np.array_equal(core.fetchvars(V1, (Y0, Y0 + rows - 1)), x[:, :members], equal_nan=True)
        a = core.project(V1, years, B, **kw)
        assert np.array_equal(a, core.project(V1, years, B, **kw), equal_nan=True)
        res[name] = a
        if name == "sorted":
            print("lanes permuted by the sorting: %s" % (not np.array_equal(core.lane_of_member(), np.arange(nm))))
            ref, s = checker(np.nan_to_num(x, nan=280.0), Y0, years, B, center, (Y0 + 60, Y0 + 69))
            ok = ~np.isnan(a).any(axis=0)
            check_against(a[:, ok], ref[:, ok], s[:, ok], n, ("written rows", n))
        core.shutdown()
    bad = np.isnan(res["sorted"])
    assert bad[:, [40, 500]].all() and bad.sum() == 2 * 19
    assert np.array_equal(res["sorted"], res["unsorted"], equal_nan=True)
    assert np.array_equal(res["cut"], res["sorted"][:, :100], equal_nan=True)
    assert np.array_equal(res["cut unsorted"], res["sorted"][:, :100], equal_nan=True)


# ---- 5. shards ---------------------------------------------------------------------------------------

def test_shards_on_one_device_give_the_same_bits(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    nm = 1029
    years = np.arange(1760, 1900)
    n = len(years)
    rng = np.random.default_rng(15)
    B = rng.normal(size=(33, n))
    res = []
    for shards in (1, 2, 3):
        core = _core(nm, hip_lib, pair_limit=0, devices=[0] * shards)
        core.run(1900)
        x = core.fetchvars(V1, (1745, 1900))
        if not res:
            center = x[years - 1745, 3]
        a = core.project(V1, years, B, center=center, baseline=(1745, 1760))
        assert a.shape == (33, nm) and np.array_equal(a, core.project(V1, years, B, center=center, baseline=(1745, 1760)))
        ref, s = checker(x, 1745, years, B, center, (1745, 1760))
        ok = (s > 0).all(axis=0)                         # (the member the centre was taken of: r = 0 where no baseline shifts it)
        check_against(a[:, ok], ref[:, ok], s[:, ok], n, ("shards", shards))
        res.append((x, a))
        core.shutdown()
    for x, a in res[1:]:
        assert np.array_equal(x, res[0][0])             # (the same trajectories, as tests/test_gpu_quantiles.py holds)
        assert np.array_equal(a, res[0][1])


def test_the_ensemble_smoother_example_runs(hip_lib, capsys):
    spec = importlib.util.spec_from_file_location(
        "example_ensemble_smoother", os.path.join(ROOT, "examples", "ensemble_smoother.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 320
    sd_prior, sd_post, theta, new = mod.main(n, lib_path=hip_lib)
    out = capsys.readouterr().out
    assert out.count("correlation of its score with S") == 3 and "after one step" in out
    assert theta.shape == new.shape == (3, n) and np.isfinite(new).all() and not np.array_equal(theta, new)
    for (_, lo, hi, _), row in zip(mod.PRIOR, new):
        assert (row >= lo).all() and (row <= hi).all()
    assert np.isfinite(sd_prior) and np.isfinite(sd_post) and sd_prior > 0 and sd_post > 0


def test_zz_report():
    print("hx_member_project: worst error / bound over this module %.3g" % _worst["ratio"])
    assert 0.0 < _worst["ratio"] <= 1.0
