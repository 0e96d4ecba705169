"""Per-member input series given as a mix of shared year-vectors (hx_setvar_dated_mix).

The yardstick is the dense path, which tests/test_member_series.py holds to the oracle: a core
given a mix must equal, BIT FOR BIT, a core given setvar_dated_members() of the numpy restatement
of the definition in include/hector_amd.h,

    s = coeff[0][m] * basis[0][i];  for k = 1 .. K-1:  s = s + (coeff[k][m] * basis[k][i])

every product rounded before it is added, in ascending k (numpy's float64 multiply and add are
IEEE operations, nothing is fused).  No tolerance is involved anywhere in this file.

S is unsorted (test_member_series.member_S), so the lane order is a real permutation of the member
order: the mix kernel has to take a lane's coefficients through member_of_lane, give the padding
lanes the last member's, and write row (year - startDate + lag) of the table.

This file: the helpers and the host-build tier (tests/emul, 70 members: two wavefronts, six real
lanes in the second).  tests/test_gpu_member_mix.py: the same on the device with 130 members."""
import ctypes

import numpy as np
import pytest

import hector_amd
from test_member_series import (BITWISE, EM_YEARS, END, FLAVOURS, UNIT, Y0, assert_flavour, make_core,
                                set_series)

N_HOST = 70
HOST = dict(allow_emulation=True)
Error = hector_amd.HectorAmdError

# name: (low, high of the large positive term's basis; amplitude of the small terms' basis).  The
# large term's coefficient lies in 0.7..1.3, the small ones in -1..1: with up to seven small terms
# every resulting emission stays positive.
MIX_VARS = {
    "ffi_emissions": (4.0, 10.0, 0.3),
    "daccs_uptake": (0.5, 2.0, 0.03),
    "luc_emissions": (0.5, 2.0, 0.03),
    "luc_uptake": (0.3, 1.0, 0.02),
    "CH4_emissions": (150.0, 450.0, 10.0),
}


# ---------------------------------------------------------------------------------------------
# inputs (functions of the ensemble size alone: fixed seeds) and the definition

def restate(basis, coeff, descending=False):
    """The definition, literally -> values[year, member].  descending: the same products added in
    the opposite order (what the order test must be able to tell apart)."""
    basis, coeff = np.atleast_2d(basis), np.atleast_2d(coeff)
    ks = range(basis.shape[0])
    s = None
    for k in (reversed(ks) if descending else ks):
        p = coeff[k][None, :] * basis[k][:, None]
        s = p if s is None else s + p
    return s


def one_mix(rng, name, years, n, K):
    lo, hi, small = MIX_VARS[name]
    basis = np.vstack([rng.uniform(lo, hi, (1, years.size)), rng.uniform(-small, small, (K - 1, years.size))])
    coeff = np.vstack([rng.uniform(0.7, 1.3, (1, n)), rng.uniform(-1.0, 1.0, (K - 1, n))])
    assert restate(basis, coeff).min() > 0.0
    return (name, years, basis, coeff)


def standard_mixes(n, seed=91, K=3):
    """[(name, years, basis[K, year], coeff[K, member])]: all five variables, 2030-2100; basis
    values independent from year to year (a row written to the wrong year shows), coefficients
    independent per member."""
    rng = np.random.default_rng(seed)
    return [one_mix(rng, name, EM_YEARS, n, K) for name in MIX_VARS]


def order_mix(n):
    """ffi_emissions, K = 8.  The seed was chosen on the CPU such that adding the products in
    descending k gives other bits somewhere (check_order asserts it)."""
    return [one_mix(np.random.default_rng(92), "ffi_emissions", EM_YEARS, n, 8)]


def edge_mixes(n):
    """K = 1, a year list with gaps that holds both ends of the scenario: ffi_emissions (lag 1:
    the startDate value is consumed in the first year, the endDate value never, it has no row in
    the table) and CH4_emissions (lag 0).  Magnitudes as test_member_series.edge_series."""
    rng = np.random.default_rng(93)
    years = np.array([END, Y0, 2000, Y0 + 1, 2100, END - 1])   # (not in order either)
    late = years > 1900
    ffi = np.where(late, rng.uniform(1.0, 5.0, years.size), rng.uniform(0.1, 1.0, years.size))
    ch4 = np.where(late, rng.uniform(100.0, 400.0, years.size), rng.uniform(20.0, 80.0, years.size))
    return [("ffi_emissions", years, ffi[None, :], rng.uniform(0.5, 1.5, (1, n))),
            ("CH4_emissions", years, ch4[None, :], rng.uniform(0.5, 1.5, (1, n)))]


def as_dense(mixes):
    """The series setvar_dated_members() takes for the same values."""
    return [(name, years, restate(basis, coeff)) for name, years, basis, coeff in mixes]


def set_mixes(c, mixes):
    for name, years, basis, coeff in mixes:
        assert c.setvar_dated_mix(name, years, basis, coeff, UNIT[name]) is c


# ---------------------------------------------------------------------------------------------
# a finished core as plain data; references are computed once and shared, never changed

def result(c, fl=None, run_to=END):
    if fl is not None:
        assert_flavour(c, fl)
    r = {v: c.fetchvars(v, (Y0, run_to)).copy() for v in BITWISE}
    r["status"] = c.status().copy()
    for name in MIX_VARS:
        r["in:" + name] = c.fetchvars(name, (Y0, END)).copy()
    for a in r.values():
        a.setflags(write=False)
    return r


def assert_equal_results(a, b, where):
    assert set(a) == set(b)
    for v in a:
        assert a[v].shape == b[v].shape, (where, v)
        assert np.array_equal(a[v], b[v], equal_nan=True), \
            (where, v, np.argwhere(~((a[v] == b[v]) | (np.isnan(a[v]) & np.isnan(b[v]))))[:4])


_REF = {}


def reference(lib, flavour, n, kw, what, mixes, how):
    """A fresh core given `mixes` as mixes (how = "mix") or as the dense restatement ("dense"),
    run to END -> result(); once per (lib, flavour, n, what, how)."""
    key = (lib, flavour, n, what, how)
    if key not in _REF:
        fl = FLAVOURS[flavour]
        c = make_core(lib, fl, n, kw)
        if how == "mix":
            set_mixes(c, mixes)
        else:
            set_series(c, as_dense(mixes))
        c.run(END)
        assert not np.array_equal(c.lane_of_member(), np.arange(n)), "lane order is the member order"
        _REF[key] = result(c, fl)
        c.shutdown()
    return _REF[key]


# ---------------------------------------------------------------------------------------------
# the checks, for the host build and the device alike (kw: how the core is made)

def check_equality(lib, flavour, n, kw):
    """All five variables at once, K = 3, 2030-2100: outputs, status and the fetched inputs over
    the whole scenario equal the dense core's."""
    mixes = standard_mixes(n)
    got = reference(lib, flavour, n, kw, "std", mixes, "mix")
    want = reference(lib, flavour, n, kw, "std", mixes, "dense")
    assert (want["status"] == 0).all()
    assert_equal_results(got, want, flavour)
    for name, years, basis, coeff in mixes:   # (and the inputs are the definition's bits)
        assert np.array_equal(got["in:" + name][years - Y0], restate(basis, coeff)), name


def check_order(lib, n, kw):
    """K = 8 on ffi_emissions: the ascending-k sum, not the descending one."""
    mixes = order_mix(n)
    _, years, basis, coeff = mixes[0]
    up, down = restate(basis, coeff), restate(basis, coeff, descending=True)
    assert (up != down).any(), "this seed cannot see an order change: choose another"
    assert np.allclose(up, down, rtol=1e-14, atol=0.0)
    got = reference(lib, "run", n, kw, "k8", mixes, "mix")
    back = got["in:ffi_emissions"][years - Y0]
    assert np.array_equal(back, up) and not np.array_equal(back, down)
    # the device table holds the same bits: the run equals the run on the dense restatement
    assert_equal_results(got, reference(lib, "run", n, kw, "k8", mixes, "dense"), "K = 8")


def check_edges(lib, n, kw):
    """K = 1, both ends of the scenario, lag 1 and lag 0, against the dense core as in
    test_member_series.check_edges."""
    mixes = edge_mixes(n)
    got = reference(lib, "run", n, kw, "edge", mixes, "mix")
    want = reference(lib, "run", n, kw, "edge", mixes, "dense")
    assert (want["status"] == 0).all()
    assert_equal_results(got, want, "edges")
    for name, years, basis, coeff in mixes:
        assert np.array_equal(got["in:" + name][years - Y0], restate(basis, coeff)), name
    # the values matter where they are consumed (S alone moves neither in year one)
    assert np.ptp(got["CO2_concentration"][1]) > 0.01 and np.ptp(got["CH4_concentration"][-1]) > 1.0


def check_history(lib, n, kw):
    """A plain run to 2150 with the state history, then a mix from 2050, then run(2150): the core
    goes back to 2049 by itself, like the dense core that does the same
    (test_member_series.check_history_rerun)."""
    fl = FLAVOURS["run"]
    yrs = np.arange(2050, 2101)
    rng = np.random.default_rng(94)
    mixes = [one_mix(rng, name, yrs, n, 3) for name in MIX_VARS]
    res = []
    for how in ("mix", "dense"):
        c = make_core(lib, fl, n, kw)
        c.enable_history(True)
        c.run(2150)
        assert (c.last_run_kernel(), c.last_run_variant()) == ("run", 0)
        before = result(c, run_to=2150)
        if how == "mix":
            set_mixes(c, mixes)
        else:
            set_series(c, as_dense(mixes))
        c.run(2150)
        assert c.current_date == 2150
        after = result(c, fl, run_to=2150)
        for v in BITWISE:
            assert np.array_equal(after[v][:2050 - Y0], before[v][:2050 - Y0]), v
        assert not np.array_equal(after["CO2_concentration"][2051 - Y0:], before["CO2_concentration"][2051 - Y0:])
        res.append(after)
        c.shutdown()
    assert_equal_results(res[0], res[1], "history")


# ---------------------------------------------------------------------------------------------
# the host-build tier

@pytest.mark.parametrize("flavour", ["run", "b4"])
def test_mix_equals_the_dense_path(emul_lib, flavour):
    check_equality(emul_lib, flavour, N_HOST, HOST)


def test_products_are_added_in_ascending_k(emul_lib):
    check_order(emul_lib, N_HOST, HOST)


def test_one_vector_at_the_scenario_ends(emul_lib):
    check_edges(emul_lib, N_HOST, HOST)


def test_mix_set_after_a_run_with_history(emul_lib):
    check_history(emul_lib, N_HOST, HOST)


TO = 2100   # the overlay and error tests run this far: every covered year lies before it


def run_result(c, fl=None):
    c.run(TO)
    return result(c, fl, run_to=TO)


def test_mix_overlays_a_dense_table(emul_lib):
    """A mix over 2050-2070 on top of setvar_dated_members() over 2030-2100: the other years keep
    the dense values; a shared edit in an uncovered year goes into every member's row."""
    n, fl = N_HOST, FLAVOURS["run"]
    rng = np.random.default_rng(95)
    under = rng.uniform(2.0, 12.0, (EM_YEARS.size, n))
    name, yrs, basis, coeff = one_mix(rng, "ffi_emissions", np.arange(2050, 2071), n, 2)
    c = make_core(emul_lib, fl, n, HOST, series=[(name, EM_YEARS, under)])
    c.setvar_dated_mix(name, yrs, basis, coeff, UNIT[name])
    merged = under.copy()
    merged[yrs - EM_YEARS[0]] = restate(basis, coeff)
    d = make_core(emul_lib, fl, n, HOST, series=[(name, EM_YEARS, merged)])
    assert_equal_results(run_result(c, fl), run_result(d, fl), "mix over dense")
    assert np.array_equal(c.fetchvars(name, (2030, 2049)), under[:20])
    for x in (c, d):
        x.setvar_dated(name, [2040, 2041], [7.25, 7.5], UNIT[name])
    got = run_result(c, fl)
    assert_equal_results(got, run_result(d, fl), "shared edit under a mix over dense")
    assert (got["in:" + name][2040 - Y0] == 7.25).all()
    c.clear_mix(name)   # the dense table is whole again
    e = make_core(emul_lib, fl, n, HOST, series=[(name, EM_YEARS, under)])
    e.setvar_dated(name, [2040, 2041], [7.25, 7.5], UNIT[name])
    assert_equal_results(run_result(c, fl), run_result(e, fl), "mix removed from a dense table")
    c.shutdown(); d.shutdown(); e.shutdown()


def test_mix_overlays_the_scenario_and_is_replaced_and_removed(emul_lib):
    """No dense table: the uncovered years keep the scenario's values; a replacing mix with fewer
    years restores the rest; clear_mix restores everything -- the bits (and the kernel) of a core
    that never had a mix."""
    n, fl = N_HOST, FLAVOURS["run"]
    plain_fl = dict(fl, variant=0)
    rng = np.random.default_rng(96)
    name = "ffi_emissions"
    wide = one_mix(rng, name, EM_YEARS, n, 3)
    narrow = one_mix(rng, name, np.arange(2050, 2071), n, 2)
    p = make_core(emul_lib, fl, n, HOST)
    plain = run_result(p, plain_fl)
    scenario = plain["in:" + name]
    assert np.ptp(scenario, axis=1).max() == 0.0
    c = make_core(emul_lib, fl, n, HOST)
    set_mixes(c, [wide])
    first = run_result(c, fl)
    out = np.ones(END - Y0 + 1, bool)
    out[EM_YEARS - Y0] = False
    assert np.array_equal(first["in:" + name][out], scenario[out])
    assert not np.array_equal(first["CO2_concentration"], plain["CO2_concentration"])
    # replaced by a mix with fewer years
    set_mixes(c, [narrow])
    d = make_core(emul_lib, fl, n, HOST)
    set_mixes(d, [narrow])
    second = run_result(c, fl)
    assert_equal_results(second, run_result(d, fl), "replaced")
    out[:] = True
    out[narrow[1] - Y0] = False
    assert np.array_equal(second["in:" + name][out], scenario[out])
    # removed (and removing what is not there is no error)
    assert c.clear_mix(name) is c
    c.clear_mix(name).clear_mix("luc_uptake")
    assert_equal_results(run_result(c, plain_fl), plain, "removed")
    c.shutdown(); d.shutdown(); p.shutdown()


def test_shared_and_dense_edits_next_to_a_mix(emul_lib):
    """setvar_dated in an uncovered year shows in the next run (no dense table: the rows under the
    mix are rebuilt from the shared series); in a covered year it and setvar_dated_members are
    refused, name their function, say what to do and change nothing."""
    n, fl = N_HOST, FLAVOURS["run"]
    name = "ffi_emissions"
    mix = one_mix(np.random.default_rng(97), name, np.arange(2040, 2081), n, 3)
    c = make_core(emul_lib, fl, n, HOST)
    set_mixes(c, [mix])
    before = run_result(c, fl)
    c.setvar_dated(name, [2020, 2021], [11.0, 12.0], UNIT[name])
    d = make_core(emul_lib, fl, n, HOST, series=as_dense([mix]))
    d.setvar_dated(name, [2020, 2021], [11.0, 12.0], UNIT[name])
    edited = run_result(c, fl)
    assert_equal_results(edited, run_result(d, fl), "shared edit in an uncovered year")
    assert (edited["in:" + name][2020 - Y0] == 11.0).all()
    assert not np.array_equal(edited["CO2_concentration"][2022 - Y0], before["CO2_concentration"][2022 - Y0])
    with pytest.raises(Error, match=r"hx_setvar_dated: .*remove the mix first"):
        c.setvar_dated(name, [2039, 2040], [1.0, 1.0], UNIT[name])
    with pytest.raises(Error, match=r"hx_setvar_dated_members: .*remove the mix first"):
        c.setvar_dated_members(name, [2080, 2090], np.ones((2, n)), UNIT[name])
    assert np.array_equal(c.fetchvars(name, (Y0, END)), edited["in:" + name])
    c.reset(Y0)
    assert_equal_results(run_result(c, fl), edited, "after the refused edits")
    # a per-member edit in an uncovered year makes the dense table beneath the mix
    vals = np.random.default_rng(98).uniform(2.0, 12.0, (2, n))
    for x in (c, d):
        x.setvar_dated_members(name, [2085, 2090], vals, UNIT[name])
    assert_equal_results(run_result(c, fl), run_result(d, fl), "dense edit in an uncovered year")
    c.shutdown(); d.shutdown()


def raw_mix(c, cap, years, nyears, basis, nbasis, coeff, units=None):
    """hx_setvar_dated_mix as a C caller sees it -> (return code, message)."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    y = None if years is None else np.ascontiguousarray(years, dtype=np.int32)
    b = None if basis is None else np.ascontiguousarray(basis, dtype=np.float64)
    w = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.float64)
    rc = c._lib.hx_setvar_dated_mix(c._h, cap.encode(), None if y is None else y.ctypes.data_as(ip), nyears,
                                    None if b is None else b.ctypes.data_as(dp), nbasis,
                                    None if w is None else w.ctypes.data_as(dp),
                                    units.encode() if units else None)
    return rc, c._lib.hx_last_error().decode()


def test_refused_calls_name_the_function_and_change_nothing(emul_lib):
    n, fl = N_HOST, FLAVOURS["run"]
    name = "ffi_emissions"
    mix = one_mix(np.random.default_rng(99), name, np.arange(2040, 2081), n, 3)
    c = make_core(emul_lib, fl, n, HOST)
    set_mixes(c, [mix])
    before = run_result(c, fl)
    yrs = np.array([2050, 2051])
    b, w = np.ones((2, 2)), np.ones((2, n))
    nan_b, inf_w = b.copy(), w.copy()
    nan_b[1, 0] = np.nan
    inf_w[1, n - 1] = np.inf
    bad = [
        ("CO2_constrain", yrs, 2, b, 2, w, None, "ffi_emissions, daccs_uptake, luc_emissions, luc_uptake, CH4_emissions"),
        ("tas_constrain", yrs, 2, b, 2, w, None, "CH4_emissions"),
        ("S", yrs, 2, b, 2, w, None, "not supported"),
        (name, yrs, 2, b, 2, w, "Tg CH4", "Units"),
        (name, yrs, 2, np.ones((9, 2)), 9, np.ones((9, n)), None, "nbasis"),
        (name, yrs, 2, b, -1, w, None, "nbasis"),
        (name, yrs, 0, b, 2, w, None, "nyears"),
        (name, [Y0 - 1, 2051], 2, b, 2, w, None, "startDate"),
        (name, [2050, END + 1], 2, b, 2, w, None, "startDate"),
        (name, [2050, 2050], 2, b, 2, w, None, "twice"),
        (name, yrs, 2, nan_b, 2, w, None, "finite"),
        (name, yrs, 2, b, 2, inf_w, None, "finite"),
        (name, None, 2, b, 2, w, None, "null"),
        (name, yrs, 2, None, 2, w, None, "null"),
        (name, yrs, 2, b, 2, None, None, "null"),
    ]
    for cap, years, ny, basis, nb, coeff, units, word in bad:
        rc, msg = raw_mix(c, cap, years, ny, basis, nb, coeff, units)
        assert rc != 0 and msg.startswith("hx_setvar_dated_mix: ") and word in msg, (cap, word, rc, msg)
        assert np.array_equal(c.fetchvars(name, (Y0, END)), before["in:" + name]), word
    # the Python layer: shapes, before anything reaches the library
    for basis, coeff in ((np.ones((2, 3)), w), (b, np.ones((2, n - 1))), (b, np.ones((1, n))), (np.ones(2), w)):
        with pytest.raises(Error, match="setvar_dated_mix: "):
            c.setvar_dated_mix(name, yrs, basis, coeff)
    with pytest.raises(Error, match="hx_setvar_dated_mix: .*nbasis"):
        c.setvar_dated_mix(name, yrs, np.ones((9, 2)), np.ones((9, n)))
    with pytest.raises(Error, match="hx_setvar_dated_mix: "):
        c.clear_mix("CO2_constrain")
    # nothing was dirtied and nothing changed: the results stand, and a new run repeats them
    assert_equal_results(result(c, fl, run_to=TO), before, "after the refused calls")
    c.reset(Y0)
    assert_equal_results(run_result(c, fl), before, "a run after the refused calls")
    # K = 1 as two 1-D arrays is the one-row mix
    one = one_mix(np.random.default_rng(100), name, yrs, n, 1)
    c.setvar_dated_mix(name, yrs, one[2][0], one[3][0], UNIT[name])
    assert np.array_equal(c.fetchvars(name, (2050, 2051)), restate(one[2], one[3]))
    c.shutdown()
