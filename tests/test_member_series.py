"""Per-member input series (hx_setvar_dated_members) on every kernel flavour, against the oracle.

All ten series that have a row in kDatedInputs (ensemble_core.cpp) set per member: the five emission series at
once on every flavour of the run kernels, the five constraints with members that hold different
ones (or none), values at the ends of the scenario, and the workflows that move a member's series
to another lane or another year.  S is drawn unsorted, so with member sorting on the lane order is
a real permutation of the member order: upload_member_series() has to apply member_of_lane_, the
lag of one year of the four carbon series and the padding lanes' copy of the last member, and the
kernels have to read row mseries[k][iy * npad + lane] behind the ms_mask bit of series k.

Each checked member runs on the oracle, reading a scenario pack that carries that member's series
(conftest.edited_pack, chained); the tolerances are the project's (tests/test_member_constraints.py,
tests/test_emulation_parity.py).  The series do not enter the spinup, so no member is left out.

This file: the helpers and the host-build tier (tests/emul, 70 members: two wavefronts, six real
lanes in the second).  tests/test_gpu_member_series.py: the same on the device with 130 members."""
import numpy as np
import pytest

import hector_amd
from conftest import SCENARIO, edited_pack
from test_tracking import FRAC_TOL

Y0, END = 1745, 2300
WAVE = 64
REL_CO2, ABS_T, ABS_CH4 = 2e-8, 2e-8, 1e-6
TRACK_DATE = 1900
OUTS = ["CO2_concentration", "global_tas", "RF_tot", "CH4_concentration", "timesteps", "NBP"]
BITWISE = OUTS   # what a core in another lane order must reproduce bit for bit

# name: (section, unit, low, high) -- every member its own value in every year of EM_YEARS,
# independent from year to year (a row read from the wrong year shows up in the result)
EMISSIONS = {
    "ffi_emissions": ("simpleNbox", "Pg C/yr", 2.0, 12.0),
    "daccs_uptake": ("simpleNbox", "Pg C/yr", 0.0, 2.0),
    "luc_emissions": ("simpleNbox", "Pg C/yr", 0.0, 2.0),
    "luc_uptake": ("simpleNbox", "Pg C/yr", 0.0, 1.0),
    "CH4_emissions": ("CH4", "Tg CH4", 100.0, 500.0),
}
CONSTRAINTS = {
    "CO2_constrain": ("simpleNbox", "ppmv CO2"),
    "NBP_constrain": ("simpleNbox", "Pg C/yr"),
    "tas_constrain": ("temperature", "degC"),
    "RF_tot_constrain": ("forcing", "W/m2"),
    "CH4_constrain": ("CH4", "ppbv CH4"),
}
SECTION = {k: v[0] for k, v in list(EMISSIONS.items()) + list(CONSTRAINTS.items())}
UNIT = {k: v[1] for k, v in list(EMISSIONS.items()) + list(CONSTRAINTS.items())}
POINTS = ("tas_constrain", "RF_tot_constrain")   # given as points, interpolated per member
EM_YEARS = np.arange(2030, 2101)

# kernel flavours: biome count, two-wavefront threshold, NBP constraint per member, tracking; what
# run() must report.  The pair kernel hands a core with member series to the run kernel
# (tests/test_gpu_pair_kernel.py): its limit is 0 everywhere.
FLAVOURS = {
    "run": dict(B=1, w2=0, kernel="run", variant=-1),
    "run-nbp": dict(B=1, w2=0, kernel="run", variant=1, nbp=True),
    "run2": dict(B=1, w2=1, kernel="run2", variant=-1),
    "run2-nbp": dict(B=1, w2=1, kernel="run2", variant=1, nbp=True),
    "b2": dict(B=2, w2=0, kernel="run", variant=-1),
    "b4": dict(B=4, w2=0, kernel="run", variant=-1),
    "b6": dict(B=6, w2=0, kernel="run", variant=-1),
    "b9": dict(B=9, w2=0, kernel="run", variant=-1),
    "b4-nbp": dict(B=4, w2=0, kernel="run", variant=1, nbp=True),
    "b9-nbp": dict(B=9, w2=0, kernel="run", variant=1, nbp=True),
    "trk": dict(B=1, w2=0, kernel="run", variant=2, track=True),
    "trk-b2": dict(B=2, w2=0, kernel="run", variant=2, track=True),
}
ALL_FLAVOURS = list(FLAVOURS)
N_HOST = 70


# ---------------------------------------------------------------------------------------------
# inputs (functions of the ensemble size alone: fixed seeds)

def member_S(n):
    """Unsorted: with member sorting on the lane order is a permutation of the member order."""
    return np.random.default_rng(20261019).uniform(2.0, 5.0, n)


def emission_series(n):
    """[(name, years, values[year, member])]: all five emission series, 2030-2100."""
    rng = np.random.default_rng(77)
    return [(name, EM_YEARS, rng.uniform(lo, hi, (EM_YEARS.size, n)))
            for name, (_, _, lo, hi) in EMISSIONS.items()]


def nbp_series(n):
    """An NBP constraint held by every third member, 2040-2080 (inside the emission years)."""
    yrs = np.arange(2040, 2081)
    rng = np.random.default_rng(78)
    v = np.full((yrs.size, n), np.nan)
    v[:, ::3] = rng.uniform(-1.0, 2.0, (yrs.size, v[:, ::3].shape[1]))
    return [("NBP_constrain", yrs, v)]


def constraint_series(n):
    """Members that hold different constraints, by member % 7: 0 none; 1 CO2 in a window; 2 NBP;
    3 tas points; 4 RF_tot points; 5 CO2 and CH4; 6 NBP and tas points.  NaN outside the windows
    and for the other members.  The NBP windows begin in different years (1950 + member % 5): the
    kernel's read of the previous row (nbp_lo) meets NaN -> value edges inside a wavefront.  The
    points lie at two to four of five dates, other ones for every member."""
    rng = np.random.default_rng(79)
    kind = np.arange(n) % 7
    f = rng.uniform(0.8, 1.2, n)
    nan = np.nan
    y = np.arange(1950, 2051)
    co2 = np.full((y.size, n), nan)
    for i in np.flatnonzero((kind == 1) | (kind == 5)):
        co2[:, i] = 311.0 + 1.96 * f[i] * (y - 1950) + rng.uniform(0.0, 0.5, y.size)
    y4 = np.arange(1960, 2041)
    ch4 = np.full((y4.size, n), nan)
    for i in np.flatnonzero(kind == 5):
        ch4[:, i] = 1200.0 + 10.0 * f[i] * (y4 - 1960) + rng.uniform(0.0, 5.0, y4.size)
    yn = np.arange(1950, 2001)
    nbp = np.full((yn.size, n), nan)
    for i in np.flatnonzero((kind == 2) | (kind == 6)):
        m = yn >= 1950 + i % 5
        nbp[m, i] = 0.5 * f[i] + rng.uniform(-0.3, 0.3, m.sum())
    out = [("CO2_constrain", y, co2), ("CH4_constrain", y4, ch4), ("NBP_constrain", yn, nbp)]
    for name, kinds, dates, v0, slope in (("tas_constrain", (3, 6), [1960, 1990, 2020, 2050, 2080], 0.3, 0.018),
                                          ("RF_tot_constrain", (4,), [1950, 1980, 2010, 2040, 2070], 0.5, 0.04)):
        dates = np.array(dates)
        pts = np.full((dates.size, n), nan)
        for i in np.flatnonzero(np.isin(kind, kinds)):
            at = np.sort(rng.choice(dates.size, rng.integers(2, 5), replace=False))
            pts[at, i] = v0 + slope * f[i] * (dates[at] - dates[0]) + rng.uniform(-0.05, 0.05, at.size)
        out.append((name, dates, pts))
    return out


def edge_series(n):
    """Values at the ends of the scenario.  ffi_emissions (lag 1): the startDate value is consumed
    in the first year, the endDate value never; CH4_emissions (lag 0)."""
    rng = np.random.default_rng(80)
    yf = np.array([Y0, Y0 + 1, END - 1, END])
    ffi = np.vstack([rng.uniform(0.0, 1.0, (2, n)), rng.uniform(0.0, 5.0, (2, n))])
    yc = np.array([Y0 + 1, END - 1, END])
    ch4 = np.vstack([rng.uniform(20.0, 80.0, (1, n)), rng.uniform(100.0, 400.0, (2, n))])
    return [("ffi_emissions", yf, ffi), ("CH4_emissions", yc, ch4)]


# ---------------------------------------------------------------------------------------------
# the core side

def make_core(lib, fl, n, kw, sorting=True, series=()):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, **kw)
    assert c.backend == ("host-emulation" if kw.get("allow_emulation") else "hip"), c.backend
    if not sorting:
        c.set_member_sorting(False)
    if fl["B"] > 1:
        c.split_biome(["b%d" % b for b in range(fl["B"])])
    c.set_pair_kernel_limit(0).set_two_wave_from(fl["w2"])
    if fl.get("track"):
        c.setvar("trackingDate", [TRACK_DATE])
    c.setvar("S", member_S(n), "degC")
    c.set_outputs(OUTS)
    set_series(c, series)
    return c


def set_series(c, series):
    for name, years, vals in series:
        c.setvar_dated_members(name, years, vals, UNIT[name])


def assert_flavour(c, fl):
    assert (c.last_run_kernel(), c.last_run_variant()) == (fl["kernel"], fl["variant"]), \
        (c.last_run_kernel(), c.last_run_variant(), fl)
    assert len(c.biomes()) == fl["B"]


def outputs(c, run_to=END):
    return {v: c.fetchvars(v, (Y0, run_to)).copy() for v in BITWISE}


def assert_same_bits(a, b, where):
    for v in a:
        assert np.array_equal(a[v], b[v]), (where, v, np.nanmax(np.abs(a[v] - b[v])))


def assert_series_come_back(c, series, where=""):
    """fetchvars of a member series returns what was set, in member order (the interpolated
    constraints: at the members' own points, and nothing for a member without points)."""
    for name, years, vals in series:
        back = c.fetchvars(name, (years.min(), years.max()))[years - years.min()]
        if name in POINTS:
            ok = ~np.isnan(vals)
            assert np.array_equal(back[ok], vals[ok]), (where, name)
            none = ~ok.any(axis=0)
            assert np.isnan(c.fetchvars(name, (Y0 + 1, END))[:, none]).all(), (where, name)
        else:
            assert np.array_equal(back, vals, equal_nan=True), (where, name)


def checked_members(c, n, every):
    """The members to compare with the oracle: all of them, or at least twelve that sit in every
    wavefront -- first lane, other lanes, and the last two real lanes of the ragged one.
    Asserts that the lane order is a real permutation and that the choice covers the wavefronts."""
    lanes = c.lane_of_member()
    assert sorted(lanes) == list(range(n))
    assert not np.array_equal(lanes, np.arange(n)), "lane order is the member order"
    member_at = np.argsort(lanes)
    if every:
        members = list(range(n))
    else:
        want = [w * WAVE + k for w in range((n + WAVE - 1) // WAVE) for k in (0, 1, 17, 33, 63)]
        want = sorted({l for l in want if l < n} | {n - 2, n - 1})
        want += [l for l in range(5, n, 7) if l not in want][:max(0, 12 - len(want))]
        members = [int(member_at[l]) for l in want]
    assert len(members) >= 12
    got = lanes[members]
    waves = (n + WAVE - 1) // WAVE
    assert {int(l) // WAVE for l in got} == set(range(waves)), got
    for w in range(waves):
        assert any(l // WAVE == w and l % WAVE != 0 for l in got), (w, got)
    assert {n - 2, n - 1} <= set(int(l) for l in got)   # (the ragged wavefront's last two)
    return members


# ---------------------------------------------------------------------------------------------
# the reference side

def dense(name, years, vals):
    """What the oracle's pack holds for one member's series: the member's own values; points
    interpolated linearly between the member's first and last one; RF_tot_constrain flat before
    its first date (the reference's Ftot_constrain tseries extrapolates there:
    forcing_component.cpp:498 tests only the last date).  -> (years, values) or None."""
    ok = ~np.isnan(vals)
    if not ok.any():
        return None
    yy, vv = years[ok], vals[ok]
    if name in POINTS:
        full = np.arange(yy[0], yy[-1] + 1)
        vv = np.interp(full, yy, vv)
        yy = full
    if name == "RF_tot_constrain":
        vv = np.concatenate([np.full(yy[0] - Y0, vv[0]), vv])
        yy = np.arange(Y0, yy[-1] + 1)
    return yy, vv


def member_pack(path, series, i, scalars=None, base=None):
    """A scenario pack with member i's column of every series (edited_pack, chained)."""
    cur = base
    for name, years, vals in series:
        d = dense(name, years, vals[:, i])
        if d is not None:
            cur = edited_pack(path, SECTION[name], name, d[0], d[1], base=cur)
    if scalars:
        cur = edited_pack(path, None, None, [], [], base=cur, scalars=scalars)
    return cur or SCENARIO


_ORACLE = {}


def oracle_member(oracle, tmp_path, key, series, i, S, B, run_to=END, scalars=None, track=False):
    """Member i on the oracle, reading its own pack -> the oracle's result; once per `key`."""
    key = (key, i, B, run_to, track)
    if key not in _ORACLE:
        o = type(oracle)(member_pack(tmp_path / "m.hxs", series, i, scalars))
        p = o.default_params()
        if B > 1:
            p = o.split_equal(p, B)
        p.nbiome = B
        p.S = S
        r, err, _ = o.run(p, run_to)
        k = run_to - Y0 + 1
        res = {v: r[v][:k].copy() for v in ("CO2_concentration", "global_tas", "RF_tot", "CH4_concentration",
                                            "timesteps")}
        res["err"] = err
        if track:
            ov, of, _, terr = o.run_tracking(p, TRACK_DATE, run_to)
            k0 = TRACK_DATE - Y0
            res["maps"] = (ov[k0:k].copy(), of[k0:k].copy(), terr)
        o.lib.hxo_scenario_free(o.sc)
        _ORACLE[key] = res
    return _ORACLE[key]


WORST = {}   # what: largest CO2 (relative), global_tas (K), RF_tot (W/m2), CH4 (ppbv) deviation seen


def check_vs_oracle(oracle, tmp_path, c, members, key, series, B, run_to=END, what=None, scalars=None,
                    from_year=Y0):
    """Members of core c against the oracle, none left out: CO2 2e-8 relative; global_tas and
    RF_tot 2e-8 absolute; CH4 1e-6 ppbv; the stash schedule identical; no status flag."""
    n = c.n_members
    S = member_S(n)
    assert (c.status() == 0).all(), np.flatnonzero(c.status())
    got = {v: c.fetchvars(v, (Y0, run_to)) for v in ("CO2_concentration", "global_tas", "RF_tot",
                                                    "CH4_concentration", "timesteps")}
    j = from_year - Y0
    worst = np.zeros(4)
    fails = []
    for i in members:
        r = oracle_member(oracle, tmp_path, (key, n), series, i, S[i], B, run_to, scalars)
        assert r["err"] == 0, (what, i, r["err"])
        ref = r["CO2_concentration"]
        dev = np.array([(np.abs(got["CO2_concentration"][j:, i] - ref[j:]) / ref[j:]).max(),
                        np.abs(got["global_tas"][j:, i] - r["global_tas"][j:]).max(),
                        np.abs(got["RF_tot"][j:, i] - r["RF_tot"][j:]).max(),
                        np.abs(got["CH4_concentration"][j:, i] - r["CH4_concentration"][j:]).max()])
        worst = np.maximum(worst, dev)
        same_steps = np.array_equal(got["timesteps"][max(j, 1):, i], r["timesteps"][max(j, 1):])
        if not (dev[0] < REL_CO2 and dev[1] < ABS_T and dev[2] < ABS_T and dev[3] < ABS_CH4 and same_steps):
            fails.append((i, dev.tolist(), same_steps))
    WORST[what or key] = worst
    print("member series vs oracle [%s] %d members: CO2 %.2e rel, global_tas %.2e K, RF_tot %.2e, CH4 %.2e ppbv"
          % (what or key, len(members), worst[0], worst[1], worst[2], worst[3]))
    assert not fails, (what or key, fails[:8])


def check_maps_vs_oracle(oracle, tmp_path, c, i, key, series, B):
    """Member i's origin maps against the oracle's, at the tolerances of
    tests/test_gpu_one_factor.py::check_maps_vs_oracle."""
    n = c.n_members
    r = oracle_member(oracle, tmp_path, (key, n), series, i, member_S(n)[i], B, END, track=True)
    ov, of, err = r["maps"]
    assert err == 0, i
    gv, gf = c.tracking_data(i, (TRACK_DATE, END))
    assert np.abs(gv - ov).max() < 1e-10 * np.abs(ov).max(), i
    assert np.abs(gf - of).max() < FRAC_TOL, (i, np.abs(gf - of).max())
    assert np.abs(gf.sum(axis=2) - 1.0).max() < 1e-12, i


# ---------------------------------------------------------------------------------------------
# the checks, for the host build and the device alike (kw: how the core is made)

def flavour_series(fl, n):
    return emission_series(n) + (nbp_series(n) if fl.get("nbp") else [])


def check_flavour(lib, oracle, tmp_path, flavour, n, kw):
    """All five emission series at once (and the NBP constraint of the -nbp flavours)."""
    fl = FLAVOURS[flavour]
    series = flavour_series(fl, n)
    c = make_core(lib, fl, n, kw, series=series)
    c.run(END)
    assert_flavour(c, fl)
    members = checked_members(c, n, every=fl["B"] == 1)
    assert_series_come_back(c, series, flavour)
    key = "em+nbp" if fl.get("nbp") else "em"
    check_vs_oracle(oracle, tmp_path, c, members, key, series, fl["B"], what=flavour)
    if fl.get("track"):
        for i in members[1], members[-1]:   # (not lane 0; in the ragged wavefront)
            check_maps_vs_oracle(oracle, tmp_path, c, i, key, series, fl["B"])
    first = outputs(c)
    # the same bits in member order
    d = make_core(lib, fl, n, kw, sorting=False, series=series)
    d.run(END)
    assert_flavour(d, fl)
    assert np.array_equal(d.lane_of_member(), np.arange(n))
    assert_same_bits(outputs(d), first, (flavour, "unsorted"))
    if fl.get("track"):
        for i in members[1], members[-1]:
            a, b = c.tracking_data(i, (TRACK_DATE, END)), d.tracking_data(i, (TRACK_DATE, END))
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (flavour, i)
        # the constraint residual is an untracked source: refused, per member as for the core
        co2 = np.full((1, n), np.nan); co2[0, n // 2] = 400.0
        c.setvar_dated_members("CO2_constrain", [2000], co2, "ppmv CO2")
        with pytest.raises(hector_amd.HectorAmdError, match="carbon tracking together with a CO2 or NBP constraint"):
            c.run(END)
    c.shutdown(); d.shutdown()


def check_constraints(lib, oracle, tmp_path, flavour, n, kw):
    """The five constraints, other ones for every member; the expected variant is the one with the
    NBP machinery."""
    fl = dict(FLAVOURS[flavour], variant=1)
    series = constraint_series(n)
    c = make_core(lib, fl, n, kw, series=series)
    c.run(END)
    assert_flavour(c, fl)
    members = checked_members(c, n, every=fl["B"] == 1)
    members += [k for k in range(7) if k not in {i % 7 for i in members}]   # (every combination)
    assert_series_come_back(c, series, flavour)
    check_vs_oracle(oracle, tmp_path, c, members, "cons", series, fl["B"], what="constraints-" + flavour)
    # the constrained members follow their constraints
    _, years, co2 = series[0]
    got = c.fetchvars("CO2_concentration", (years.min(), years.max()))
    assert np.allclose(got[~np.isnan(co2)], co2[~np.isnan(co2)], rtol=1.5e-8)
    first = outputs(c)
    d = make_core(lib, fl, n, kw, sorting=False, series=series)
    d.run(END)
    assert_flavour(d, fl)
    assert_same_bits(outputs(d), first, (flavour, "constraints", "unsorted"))
    c.shutdown(); d.shutdown()


def check_edges(lib, oracle, tmp_path, flavour, n, kw):
    """Values at startDate, startDate+1, endDate-1 and endDate; every member against the oracle."""
    fl = FLAVOURS[flavour]
    series = edge_series(n)
    c = make_core(lib, fl, n, kw, series=series)
    c.run(END)
    assert_flavour(c, fl)
    members = checked_members(c, n, every=True)
    assert_series_come_back(c, series, flavour)
    check_vs_oracle(oracle, tmp_path, c, members, "edge", series, 1, what="edges-" + flavour)
    # the values matter where they are consumed: the first year's and the last year's CO2 and the
    # last year's CH4 differ between members (S alone moves none of them in year one)
    co2 = c.fetchvars("CO2_concentration", (Y0, END))
    assert np.ptp(co2[1]) > 0.1 and np.ptp(c.fetchvars("CH4_concentration", (END, END))[0]) > 1.0
    d = make_core(lib, fl, n, kw, sorting=False, series=series)
    d.run(END)
    assert_flavour(d, fl)
    assert_same_bits(outputs(d), outputs(c), (flavour, "edges", "unsorted"))
    c.shutdown(); d.shutdown()


def check_segments(lib, oracle, tmp_path, n, kw):
    """Workflow 1: run in segments with the series set beforehand; the one-go run's bits."""
    fl = FLAVOURS["run"]
    series = emission_series(n)
    c = make_core(lib, fl, n, kw, series=series)
    c.run(END)
    whole = outputs(c)
    d = make_core(lib, fl, n, kw, series=series)
    for y in (1750, 1751, 1800, 1983, 2100, 2300):
        d.run(y)
        assert_flavour(d, fl)
    assert_same_bits(outputs(d), whole, "segments")
    check_vs_oracle(oracle, tmp_path, d, checked_members(d, n, True), "em", series, 1, what="segments")
    c.shutdown(); d.shutdown()


def check_history_rerun(lib, oracle, tmp_path, n, kw):
    """Workflow 2: a plain run to 2150, then the series for 2000-2100, then run(2150): the core
    goes back to 1999 by itself.  The years before 2000 keep their bits; the whole trajectory
    against the oracle (the plain kernel before 2000, the extended one after: both within the
    tolerance); and the bits of a core in member order that went through the same sequence of
    kernels (tests/test_emulation_parity.py, test_per_member_emissions_vs_oracle says why the
    sequence must be the same)."""
    fl = FLAVOURS["run"]
    yrs = np.arange(2000, 2101)
    rng = np.random.default_rng(81)
    series = [(name, yrs, rng.uniform(lo, hi, (yrs.size, n))) for name, (_, _, lo, hi) in EMISSIONS.items()]
    res = []
    for sorting in (True, False):
        c = make_core(lib, fl, n, kw, sorting=sorting)
        c.enable_history(True)
        c.run(2150)
        assert (c.last_run_kernel(), c.last_run_variant()) == ("run", 0)
        before = outputs(c, 2150)
        set_series(c, series)
        c.run(2150)
        assert_flavour(c, fl)
        assert c.current_date == 2150
        after = outputs(c, 2150)
        for v in BITWISE:
            assert np.array_equal(after[v][:2000 - Y0], before[v][:2000 - Y0]), v
        assert not np.array_equal(after["CO2_concentration"][2001 - Y0:], before["CO2_concentration"][2001 - Y0:])
        res.append(after)
        if sorting:
            check_vs_oracle(oracle, tmp_path, c, checked_members(c, n, True), "hist", series, 1, 2150,
                            what="history-rerun")
            assert_series_come_back(c, series, "history")
        c.shutdown()
    assert_same_bits(res[0], res[1], "history, sorted against member order")


def check_shared_after_members(lib, oracle, tmp_path, n, kw):
    """Workflow 3: a shared setvar_dated() after the member series exist replaces those years in
    every member's row."""
    fl = FLAVOURS["run"]
    series = emission_series(n)
    c = make_core(lib, fl, n, kw, series=series)
    c.run(2060)
    yrs = np.arange(2050, 2061)
    shared = np.linspace(3.0, 9.0, yrs.size)
    c.setvar_dated("ffi_emissions", yrs, shared, "Pg C/yr")
    c.run(END)
    assert_flavour(c, fl)
    ffi = series[0][2].copy()
    ffi[yrs - EM_YEARS[0]] = shared[:, None]
    merged = [("ffi_emissions", EM_YEARS, ffi)] + series[1:]
    assert_series_come_back(c, merged, "shared after members")
    check_vs_oracle(oracle, tmp_path, c, checked_members(c, n, True), "em+shared", merged, 1,
                    what="shared-after-members")
    c.shutdown()


def check_lane_moves(lib, oracle, tmp_path, n, kw):
    """Workflow 4: the lane order by measured cost, adopted at reset(startDate) after a complete
    run (HECTOR_AMD_CALIBRATE_ALWAYS=1 is the caller's): the series move with their members."""
    fl = FLAVOURS["run"]
    series = emission_series(n) + constraint_series(n)[3:4]   # (and one densified constraint: tas)
    c = make_core(lib, fl, n, kw, series=series)
    c.run(END)
    assert_flavour(c, fl)
    assert not c.lanes_calibrated()
    lane0 = c.lane_of_member().copy()
    first = outputs(c)
    check_vs_oracle(oracle, tmp_path, c, checked_members(c, n, True), "em+tas", series, 1, what="lane-moves")
    c.reset(Y0)
    assert c.lanes_calibrated()
    lane1 = c.lane_of_member().copy()
    assert not np.array_equal(lane0, lane1)
    c.run(END)
    assert_flavour(c, fl)
    assert_same_bits(outputs(c), first, "after the lanes moved")
    assert (c.status() == 0).all()
    assert_series_come_back(c, series, "after the lanes moved")
    c.shutdown()


def check_with_gas_params(lib, oracle, tmp_path, n, kw):
    """Workflow 5: per-member TN2O0 and one halocarbon lifetime (the device gas kernel's HXM_N2O /
    HXM_RF_OTHER rows, uploaded by another path into the same table) next to per-member
    ffi_emissions; twelve members against the oracle, packs as tests/test_member_gas_params.py."""
    fl = FLAVOURS["run"]
    series = emission_series(n)[:1]
    rng = np.random.default_rng(82)
    c = make_core(lib, fl, n, kw, series=series)
    tn = 132.0 * rng.uniform(0.8, 1.2, n)
    tau = c.getvar("tau_CF4")[0] * rng.uniform(0.7, 1.3, n)
    c.setvar("TN2O0", tn, "Years").setvar("tau_CF4", tau, "Years")
    c.run(END)
    assert_flavour(c, fl)
    S = member_S(n)
    assert (c.status() == 0).all()
    members = checked_members(c, n, every=False)
    got = {v: c.fetchvars(v, (Y0, END)) for v in ("CO2_concentration", "global_tas", "RF_tot", "timesteps")}
    n2o = c.fetchvars("N2O_concentration", (Y0, END))
    for i in members:
        sc = {("N2O", "TN2O0"): tn[i], ("CF4_halocarbon", "tau"): tau[i]}
        o = type(oracle)(member_pack(tmp_path / "g.hxs", series, i, scalars=sc))
        p = o.default_params(); p.S = S[i]
        r, err, _ = o.run(p, END)
        o.lib.hxo_scenario_free(o.sc)
        assert err == 0
        ref = r["CO2_concentration"]
        assert (np.abs(got["CO2_concentration"][:, i] - ref) / ref).max() < REL_CO2, i
        assert np.abs(got["global_tas"][:, i] - r["global_tas"]).max() < ABS_T, i
        assert np.abs(got["RF_tot"][:, i] - r["RF_tot"]).max() < ABS_T, i
        assert (np.abs(n2o[:, i] - r["N2O_concentration"]) / r["N2O_concentration"]).max() < 1e-12, i
        assert np.array_equal(got["timesteps"][1:, i], r["timesteps"][1:]), i
    assert np.ptp(n2o[-1]) > 5.0
    c.shutdown()


# ---------------------------------------------------------------------------------------------
# the host-build tier

HOST = dict(allow_emulation=True)


@pytest.mark.parametrize("flavour", ALL_FLAVOURS)
def test_five_emission_series_per_member(emul_lib, oracle, tmp_path, flavour):
    check_flavour(emul_lib, oracle, tmp_path, flavour, N_HOST, HOST)


@pytest.mark.parametrize("name", ["daccs_uptake", "luc_emissions", "luc_uptake"])
def test_one_carbon_series_alone_per_member(emul_lib, oracle, tmp_path, name):
    """The three series no test had set per member, each alone (its ms_mask bit the only one)."""
    n = N_HOST
    fl = FLAVOURS["run"]
    series = [s for s in emission_series(n) if s[0] == name]
    c = make_core(emul_lib, fl, n, HOST, series=series)
    c.run(END)
    assert_flavour(c, fl)
    assert_series_come_back(c, series, name)
    check_vs_oracle(oracle, tmp_path, c, checked_members(c, n, True), "alone-" + name, series, 1,
                    what="alone-" + name)
    c.shutdown()


@pytest.mark.parametrize("flavour", ["run", "run2", "b4"])
def test_member_constraints_differ(emul_lib, oracle, tmp_path, flavour):
    check_constraints(emul_lib, oracle, tmp_path, flavour, N_HOST, HOST)


@pytest.mark.parametrize("flavour", ["run", "run2"])
def test_values_at_the_scenario_ends(emul_lib, oracle, tmp_path, flavour):
    check_edges(emul_lib, oracle, tmp_path, flavour, N_HOST, HOST)


def test_segments(emul_lib, oracle, tmp_path):
    check_segments(emul_lib, oracle, tmp_path, N_HOST, HOST)


def test_series_set_after_a_run_with_history(emul_lib, oracle, tmp_path):
    check_history_rerun(emul_lib, oracle, tmp_path, N_HOST, HOST)


def test_shared_value_after_member_series(emul_lib, oracle, tmp_path):
    check_shared_after_members(emul_lib, oracle, tmp_path, N_HOST, HOST)


def test_series_follow_their_members_when_lanes_move(emul_lib, oracle, tmp_path, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_CALIBRATE_ALWAYS", "1")
    check_lane_moves(emul_lib, oracle, tmp_path, N_HOST, HOST)


def test_member_series_next_to_member_gas_params(emul_lib, oracle, tmp_path):
    check_with_gas_params(emul_lib, oracle, tmp_path, N_HOST, HOST)


def test_the_series_discriminate(oracle, tmp_path):
    """With the oracle alone: a neighbour's series in place of a member's own, or the member's own
    shifted by one year, moves its CO2 by more than 1000 times the tolerance it is held to -- a
    kernel that read the wrong member's row or the wrong year could not pass."""
    n = N_HOST
    series = emission_series(n)
    S = member_S(n)
    i, j = 10, 11
    own = oracle_member(oracle, tmp_path, ("em", n), series, i, S[i], 1)
    assert own["err"] == 0
    swapped = [(name, years, vals[:, [j] * n]) for name, years, vals in series]
    shifted = [(name, years + 1, vals) for name, years, vals in series]
    for what, other in (("swap", swapped), ("shift", shifted)):
        r = oracle_member(oracle, tmp_path, ("em-" + what, n), other, i, S[i], 1)
        assert r["err"] == 0
        moved = (np.abs(r["CO2_concentration"] - own["CO2_concentration"]) / own["CO2_concentration"]).max()
        print("CO2 moved by %.2e (%s)" % (moved, what))
        assert moved > 1000 * REL_CO2, (what, moved)
