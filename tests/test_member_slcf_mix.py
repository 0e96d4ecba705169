"""Mixes of the short-lived climate forcer inputs -- the aerosol emissions SO2, BC, OC, NH3 and the
ozone / OH precursors NOX, CO, NMVOC (hx_enable_slcf_mixes, then hx_setvar_dated_mix) -- and the
shipped SSPs as members of ONE core (hx_setvar_scenario_mix / Core.setvar_scenarios).

The host keeps the recipes; hx_slcf_mix_kernel evaluates them ahead of the year loop and writes the
seven rows of finished terms (three OH-lifetime terms, three ozone terms, the aerosol forcing for
aero_scalar = 1) that the extended run kernels take where they take the shared table's columns.  The
yardstick is the oracle reading a scenario pack that carries the member's own series -- for the
scenario test the shipped pack itself -- at the project's tolerances: deviation / max(1, max|ref|) <
outputs_matrix.TOL for every row of ORACLE_ROWS, CH4 1e-6 ppbv, the stash schedule identical.

S is unsorted (test_member_series.member_S), so the lane order is a real permutation of the member
order.  This file: the helpers and the host-build tier (tests/emul, 70 members: two wavefronts, six
real lanes in the second).  tests/test_gpu_member_slcf_mix.py: the same on the device, 130 members."""
import os

import numpy as np
import pytest

import hector_amd
import outputs_matrix as om
import test_member_gas_mix as gm
from conftest import SCENARIO, edited_pack
from test_member_mix import assert_equal_results, restate
from test_member_series import BITWISE, END, FLAVOURS, Y0, assert_flavour, checked_members, make_core, member_S

N_HOST = 70
HOST = dict(allow_emulation=True)
Error = hector_amd.HectorAmdError
TOL = om.TOL
DATA = gm.DATA
AEROSOLS = ["SO2_emissions", "BC_emissions", "OC_emissions", "NH3_emissions"]
PRECURSORS = ["NOX_emissions", "CO_emissions", "NMVOC_emissions"]
NAMES = AEROSOLS + PRECURSORS
UNIT = {"SO2_emissions": "Gg S", "BC_emissions": "Tg", "OC_emissions": "Tg", "NH3_emissions": "Tg",
        "NOX_emissions": "Tg N", "CO_emissions": "Tg CO", "NMVOC_emissions": "Tg NMVOC"}
SECTIONS = {"SO2_emissions": ["so2"], "BC_emissions": ["bc"], "OC_emissions": ["oc"], "NH3_emissions": ["nh3"],
            "NOX_emissions": ["OH", "ozone"], "CO_emissions": ["OH", "ozone"], "NMVOC_emissions": ["OH", "ozone"]}
OWN_DIAGNOSTIC = {"SO2_emissions": "RF_SO2", "BC_emissions": "RF_BC", "OC_emissions": "RF_OC",
                  "NH3_emissions": "RF_NH3", "NOX_emissions": "TAU_OH", "CO_emissions": "O3_concentration",
                  "NMVOC_emissions": "O3_concentration"}
# what the core records, what fetchvars answers besides, and what the oracle is asked for
RECORDED = BITWISE + ["O3_concentration", "TAU_OH", "RF_O3_trop", "N2O_concentration", "RF_N2O"]
HOST_DIAG = ["RF_BC", "RF_OC", "RF_SO2", "RF_NH3", "RF_aci"]
ORACLE_ROWS = ["CO2_concentration", "global_tas", "RF_tot", "RF_BC", "RF_OC", "RF_SO2", "RF_NH3", "RF_aci",
               "RF_O3_trop", "O3_concentration", "TAU_OH", "RF_N2O", "RF_halocarbons"]
MIX_YEARS = np.arange(2030, 2101)
SCENARIOS = gm.SCENARIOS
SHIPPED = [os.path.join(DATA, s + ".hxs") for s in SCENARIOS]


# ---------------------------------------------------------------------------------------------
# the core side

def slcf_core(lib, fl, n, kw, sorting=True, params=None, switch=True):
    c = make_core(lib, fl, n, kw, sorting=sorting)
    c.set_outputs(RECORDED)
    if params:
        om.set_members(c, params, fl["B"])
    if switch:
        assert c.enable_slcf_mixes() is c
    return c


def result(c, kernel=None, run_to=END, inputs=NAMES):
    """Everything a core answers: recorded rows, the aerosol forcings, status, the inputs."""
    if kernel is not None:
        assert (c.last_run_kernel(), c.last_run_variant()) == kernel, (c.last_run_kernel(), c.last_run_variant())
    r = {v: c.fetchvars(v, (Y0, run_to)).copy() for v in RECORDED + HOST_DIAG}
    r["status"] = c.status().copy()
    for name in inputs:
        r["in:" + name] = c.fetchvars(name, (Y0, END)).copy()
    for a in r.values():
        a.setflags(write=False)
    return r


def kernel_of(fl):
    return (fl["kernel"], fl["variant"])


def set_mixes(c, mixes):
    for name, years, basis, coeff in mixes:
        assert c.setvar_dated_mix(name, years, basis, coeff, UNIT[name]) is c


def fetched(c, run_to=END):
    """What is held to the oracle, [year, member] (RF_halocarbons as the sum of the gases' forcings
    in the order the forcing component adds them up)."""
    got = {v: c.fetchvars(v, (Y0, run_to)) for v in ORACLE_ROWS[:-1] + ["CH4_concentration", "timesteps"]}
    got["RF_halocarbons"] = sum(c.fetchvars("RF_" + h, (Y0, run_to)) for h in sorted(c.halocarbons()))
    return got


# ---------------------------------------------------------------------------------------------
# the reference side

_ORACLE = {}


def oracle_run(pack, key, params, i, B, run_to=END):
    """Member i with its parameters on the oracle reading `pack`; once per key."""
    import oracle_binding
    if key not in _ORACLE:
        o = oracle_binding.Oracle(pack)
        r, err, _ = o.run(om.oracle_member(o, params, i, B), run_to)
        k = run_to - Y0 + 1
        res = {v: r[v][:k].copy() for v in ORACLE_ROWS + ["CH4_concentration", "timesteps"]}
        res["err"] = err
        o.lib.hxo_scenario_free(o.sc)
        _ORACLE[key] = res
    return _ORACLE[key]


def assert_member_vs_oracle(got, i, r, what):
    """The project's tolerances; prints every figure before it asserts."""
    assert r["err"] == 0, (what, i, r["err"])
    # (O3_concentration from startDate + 1, as outputs_matrix.oracle_row compares every row: the ozone
    # component has not run at startDate, where the reference reports its preindustrial value and the
    # core records nothing)
    first = {"O3_concentration": 1}
    fig = {v: np.abs(got[v][first.get(v, 0):, i] - r[v][first.get(v, 0):]).max() / max(1.0, np.abs(r[v]).max())
           for v in ORACLE_ROWS}
    fig["CH4 ppbv"] = np.abs(got["CH4_concentration"][:, i] - r["CH4_concentration"]).max()
    print("slcf mix vs oracle [%s] member %d: %s" % (what, i, ", ".join("%s %.2e" % kv for kv in fig.items())))
    for v in ORACLE_ROWS:
        assert fig[v] < TOL, (what, i, v, fig[v])
    assert fig["CH4 ppbv"] < 1e-6, (what, i, fig["CH4 ppbv"])
    assert np.array_equal(got["timesteps"][1:, i], r["timesteps"][1:]), (what, i)


def own_series(name):
    return gm.pack_series(SCENARIO)[(SECTIONS[name][0], name)]


def member_pack(path, mixes, i):
    """ssp245 with member i's value of every mix, in BOTH sections of a precursor."""
    cur = None
    for name, years, basis, coeff in mixes:
        for sec in SECTIONS[name]:
            cur = edited_pack(path, sec, name, years, restate(basis, coeff)[:, i], base=cur)
    return cur


# ---------------------------------------------------------------------------------------------
# 1. the shipped SSPs as members

def check_ssp_members(lib, flavour, n, kw):
    """ssp126 / ssp245 / ssp585 / ssp119 straight from hector_amd/data in one core on ssp245 through
    integer labels; every checked member against the oracle reading ITS scenario's shipped pack."""
    fl = FLAVOURS[flavour]
    params, labels = gm.member_params(n), gm.scenario_labels(n)
    c = slcf_core(lib, fl, n, kw, params=params)
    nseries = c.setvar_scenarios(SHIPPED, labels)
    ssp245 = gm.pack_series(SCENARIO)
    packs = [gm.pack_series(p) for p in SHIPPED]
    differing = {k[1] for p in packs for k, v in p.items() if not np.array_equal(v, ssp245[k])}
    assert nseries == len(differing) and set(NAMES) <= differing, (nseries, sorted(differing))
    c.run(END)
    assert_flavour(c, fl)
    assert (c.status() == 0).all(), np.flatnonzero(c.status())
    # one-hot coefficients: a member's inputs are its scenario's own bits
    for sec, name in (("so2", "SO2_emissions"), ("OH", "NOX_emissions")):
        back = c.fetchvars(name, (Y0, END))
        for g, p in enumerate(packs):
            assert np.array_equal(back[:, labels == g], np.repeat(p[(sec, name)][:, None], (labels == g).sum(), 1)), (name, g)
    got = fetched(c)
    for i in checked_members(c, n, every=False):
        g = int(labels[i])
        r = oracle_run(SHIPPED[g], ("ssp", n, fl["B"], i), params, i, fl["B"])
        assert_member_vs_oracle(got, i, r, "%s %s" % (flavour, SCENARIOS[g]))
    # not vacuous: the four groups differ in what only the new names carry (RF_SO2 per unit of the
    # member's aero_scalar; the ozone burden, which the members' carbon-cycle parameters barely reach)
    at = 2100 - Y0
    so2 = [np.median(got["RF_SO2"][at, labels == g] / params["aero_scalar"][labels == g]) for g in range(len(SCENARIOS))]
    o3 = [np.median(got["O3_concentration"][at, labels == g]) for g in range(len(SCENARIOS))]
    for vals in (so2, o3):
        assert np.diff(sorted(vals)).min() > 1000 * TOL, vals
    c.shutdown()


# ---------------------------------------------------------------------------------------------
# 2. each name alone

def one_mix(rng, name, years, n, K):
    """Leading vector: the scenario's series times an independent factor 0.5..1.5 per year (a row
    written to the wrong year shows); the others +-5 % of it; coefficients 0.7..1.3 and +-1.  Every
    resulting value stays positive."""
    own = own_series(name)
    level = np.where(own[years - Y0] > 0, own[years - Y0], 0.02 * own.max())
    lead = level * rng.uniform(0.5, 1.5, years.size)
    basis = np.vstack([lead[None, :]] + [lead[None, :] * rng.uniform(-0.05, 0.05, (1, years.size)) for _ in range(K - 1)])
    coeff = np.vstack([rng.uniform(0.7, 1.3, (1, n)), rng.uniform(-1.0, 1.0, (K - 1, n))])
    assert restate(basis, coeff).min() > 0.0, name
    return (name, years, basis, coeff)


def check_mixes_vs_oracle(lib, tmp_path, flavour, n, kw, mixes, what, moved=()):
    fl = FLAVOURS[flavour]
    params = {"S": member_S(n)}
    c = slcf_core(lib, fl, n, kw)
    set_mixes(c, mixes)
    c.run(END)
    assert_flavour(c, fl)
    assert (c.status() == 0).all()
    for name, years, basis, coeff in mixes:   # the inputs are the definition's bits
        assert np.array_equal(c.fetchvars(name, (Y0, END))[years - Y0], restate(basis, coeff)), name
    got = fetched(c)
    for i in gm.spread_members(c, n):
        r = oracle_run(member_pack(tmp_path / "m.hxs", mixes, i), (what, n, i), params, i, fl["B"])
        assert_member_vs_oracle(got, i, r, what)
    for name in moved:   # the name moved its own diagnostic
        d = c.fetchvars(OWN_DIAGNOSTIC[name], (2100, 2100))[0]
        assert np.ptp(d) > 1000 * TOL, (name, np.ptp(d))
    c.shutdown()


def check_one_name(lib, tmp_path, name, n, kw):
    mix = one_mix(np.random.default_rng(NAMES.index(name) + 400), name, MIX_YEARS, n, 3)
    check_mixes_vs_oracle(lib, tmp_path, "run", n, kw, [mix], "alone:" + name, moved=[name])


# ---------------------------------------------------------------------------------------------
# 3. edges

def edge_mixes(n):
    """K = 1, a year list with gaps, out of order, that holds startDate, startDate + 1, endDate - 1 and
    endDate: NOX (the OH term's row 0 is the member's own), SO2 and BC (the forcing base year)."""
    rng = np.random.default_rng(410)
    years = np.array([END, Y0, 2000, Y0 + 1, 2100, END - 1])
    out = []
    for name in ("NOX_emissions", "SO2_emissions", "BC_emissions"):
        own = own_series(name)
        level = np.where(own[years - Y0] > 0, own[years - Y0], 0.02 * own.max())
        out.append((name, years, (level * rng.uniform(0.5, 1.5, years.size))[None, :], rng.uniform(0.5, 1.5, (1, n))))
    return out


# ---------------------------------------------------------------------------------------------
# 4. order of operations: identity mixes change no bit

ALL_YEARS = np.arange(Y0, END + 1)


def identity(name, n):
    return (name, ALL_YEARS, own_series(name)[None, :].copy(), np.ones((1, n)))


def check_identity_mixes(lib, flavour, n, kw):
    """A: the identity mix of ffi_emissions, so that the extended kernel runs.  B: identity mixes of all
    seven names besides.  The rows hold the table's terms and the year loop adds them in the table's
    order: every recorded output has the same bits."""
    fl = FLAVOURS[flavour]
    ffi = gm.pack_series(SCENARIO)[("simpleNbox", "ffi_emissions")]
    res = []
    for with_slcf in (False, True):
        c = slcf_core(lib, fl, n, kw)
        c.setvar_dated_mix("ffi_emissions", ALL_YEARS, ffi[None, :], np.ones((1, n)), "Pg C/yr")
        if with_slcf:
            set_mixes(c, [identity(name, n) for name in NAMES])
        c.run(END)
        res.append(result(c, kernel_of(fl), inputs=()))
        c.shutdown()
    assert (res[0]["status"] == 0).all()
    assert_equal_results(res[1], res[0], "identity mixes, " + flavour)


# ---------------------------------------------------------------------------------------------
# 5. invariances, bit for bit

def standard_mixes(n, seed=420):
    rng = np.random.default_rng(seed)
    return [one_mix(rng, name, MIX_YEARS, n, 3) for name in NAMES]


_REF = {}


def straight_run(lib, n, kw):
    """A fresh core with all seven names mixed, run to END in one go; once per (lib, n)."""
    if (lib, n) not in _REF:
        fl = FLAVOURS["run"]
        c = slcf_core(lib, fl, n, kw)
        set_mixes(c, standard_mixes(n))
        c.run(END)
        _REF[(lib, n)] = result(c, kernel_of(fl))
        assert (_REF[(lib, n)]["status"] == 0).all()
        c.shutdown()
    return _REF[(lib, n)]


def check_invariances(lib, n, kw):
    fl = FLAVOURS["run"]
    ext = kernel_of(fl)
    mixes = standard_mixes(n)
    ref = straight_run(lib, n, kw)
    # sorting off: the member order is the lane order
    c = slcf_core(lib, fl, n, kw, sorting=False)
    set_mixes(c, mixes)
    c.run(END)
    assert np.array_equal(c.lane_of_member(), np.arange(n))
    assert_equal_results(result(c, ext), ref, "sorting off")
    # ... after a reset
    c.reset(Y0)
    c.run(END)
    assert_equal_results(result(c, ext), ref, "after reset")
    c.shutdown()
    # in segments, with the state history; then new coefficients and the old ones again
    c = slcf_core(lib, fl, n, kw)
    c.enable_history(True)
    set_mixes(c, mixes)
    for y in om.SEGMENTS:
        c.run(y)
    assert_equal_results(result(c, ext), ref, "segments with history")
    other = [(nm, y, b, w * np.random.default_rng(421).uniform(0.97, 1.03, w.shape)) for nm, y, b, w in mixes]
    set_mixes(c, other)
    c.run(END)
    changed = result(c, ext)
    for v in RECORDED + HOST_DIAG:   # the core went back to 2029 by itself
        assert np.array_equal(changed[v][:2030 - Y0], ref[v][:2030 - Y0]), v
    for v in ("RF_SO2", "RF_aci", "O3_concentration", "TAU_OH", "global_tas"):
        assert not np.array_equal(changed[v], ref[v]), v
    set_mixes(c, mixes)
    c.run(END)
    assert_equal_results(result(c, ext), ref, "coefficients replaced and put back")
    # clear_mix of every name: the results, and the kernel, of a core that never had one -- and of
    # one that never heard of the switch
    for name in NAMES:
        assert c.clear_mix(name) is c
    c.run(END)
    cleared = result(c)
    k_cleared = (c.last_run_kernel(), c.last_run_variant())
    c.shutdown()
    for switch in (True, False):
        p = slcf_core(lib, fl, n, kw, switch=switch)
        p.enable_history(True)
        p.run(END)
        assert (p.last_run_kernel(), p.last_run_variant()) == k_cleared != ext
        assert_equal_results(result(p), cleared, "mixes removed / switch %s, no mix" % switch)
        p.shutdown()


# ---------------------------------------------------------------------------------------------
# 6. refusals change nothing

def oh_ozone_differ(path):
    """ssp245 whose ozone.NOX_emissions differs from its OH.NOX_emissions in 2050."""
    v = gm.pack_series(SCENARIO)[("ozone", "NOX_emissions")][2050 - Y0]
    return edited_pack(path, "ozone", "NOX_emissions", [2050], [v * 1.5])


def check_refusals(lib, tmp_path, n, kw):
    fl = FLAVOURS["run"]
    yrs = np.array([2050, 2051])
    c = slcf_core(lib, fl, n, kw, switch=False)
    # switch off: today's message, today's list
    with pytest.raises(Error, match=r"hx_setvar_dated_mix: a mix is not supported for SO2_emissions \(ffi_emissions, "
                                    r"daccs_uptake, luc_emissions, luc_uptake, CH4_emissions, N2O_emissions, RF_albedo "
                                    r"and the <gas>_emissions of the scenario's halocarbons are\)"):
        c.setvar_dated_mix("SO2_emissions", yrs, np.ones((2, 2)), np.ones((2, n)))
    today = gm.OLD_NAMES + ["N2O_emissions", "RF_albedo"] + [h + "_emissions" for h in c.halocarbons()]
    assert c.mix_capabilities() == today
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*so2\.SO2_emissions"):
        c.setvar_scenarios(SHIPPED, gm.scenario_labels(n))
    c.enable_slcf_mixes()
    assert c.mix_capabilities() == today + NAMES
    mixes = standard_mixes(n)
    set_mixes(c, mixes)
    c.run(2100)
    before = result(c, kernel_of(fl), run_to=2100)

    def unchanged(what):
        for name in NAMES:
            assert np.array_equal(c.fetchvars(name, (Y0, END)), before["in:" + name]), (what, name)

    with pytest.raises(Error, match="hx_setvar_dated_mix: Units"):
        c.setvar_dated_mix("SO2_emissions", yrs, np.ones((2, 2)), np.ones((2, n)), "Tg")
    with pytest.raises(Error, match="hx_setvar_dated_mix: .*twice"):
        c.setvar_dated_mix("NOX_emissions", [2050, 2050], np.ones((2, 2)), np.ones((2, n)))
    bad = np.ones((2, n))
    bad[1, n - 1] = np.inf
    with pytest.raises(Error, match="hx_setvar_dated_mix: a coefficient is not finite"):
        c.setvar_dated_mix("BC_emissions", yrs, np.ones((2, 2)), bad)
    for name in ("SV", "RF_misc", "CH4N", "N2O_natural_emissions"):
        with pytest.raises(Error, match=r"hx_setvar_dated_mix: a mix is not supported for .*NMVOC_emissions are\)"):
            c.setvar_dated_mix(name, yrs, np.ones((2, 2)), np.ones((2, n)))
    for name in ("SO2_emissions", "NOX_emissions"):   # the dense verb still refuses the names
        with pytest.raises(Error, match="per-member dated input not supported for " + name):
            c.setvar_dated_members(name, yrs, np.ones((2, n)))
    for name in NAMES:   # a shared edit in a covered year
        with pytest.raises(Error, match=r"hx_setvar_dated: .*remove the mix first"):
            c.setvar_dated(name, [2029, 2030], [1.0, 1.0], UNIT[name])
    with pytest.raises(Error, match=r"hx_enable_slcf_mixes: .*SO2_emissions.* has a mix"):
        c.enable_slcf_mixes(False)
    lab = gm.scenario_labels(n)
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: scalar rho_bc of section forcing .*picontrol"):
        c.setvar_scenarios([os.path.join(DATA, "picontrol.hxs"), SCENARIO], lab % 2)
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*NOX_emissions of section OH differs from .*"
                                    r"OH\.NOX_emissions, ozone\.NOX_emissions"):
        c.setvar_scenarios([oh_ozone_differ(tmp_path / "two.hxs"), SCENARIO], lab % 2)
    for sec, key, val in (("so2", "SV", -1.0), ("CH4", "CH4N", 300.0)):   # these stay unmixable
        other = edited_pack(tmp_path / "other.hxs", sec, key, [2050], [val])
        with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*cannot be a mix.*%s\.%s" % (sec, key)):
            c.setvar_scenarios([other, SCENARIO], lab % 2)
    unchanged("refused calls")
    assert_equal_results(result(c, kernel_of(fl), run_to=2100), before, "after the refused calls")
    c.reset(Y0)
    c.run(2100)
    assert_equal_results(result(c, kernel_of(fl), run_to=2100), before, "a run after the refused calls")
    # a shared edit in an uncovered year is taken, next to the mix
    c.setvar_dated("SO2_emissions", [2020, 2021], [50000.0, 51000.0], UNIT["SO2_emissions"])
    c.setvar_dated("NOX_emissions", [2020], [40.0], UNIT["NOX_emissions"])
    c.run(2100)
    after = result(c, kernel_of(fl), run_to=2100)
    assert (after["in:SO2_emissions"][2020 - Y0] == 50000.0).all() and (after["in:NOX_emissions"][2020 - Y0] == 40.0).all()
    for name in ("SO2_emissions", "NOX_emissions"):
        assert np.array_equal(after["in:" + name][MIX_YEARS - Y0], before["in:" + name][MIX_YEARS - Y0])
    for v in ("RF_SO2", "O3_concentration", "TAU_OH"):
        assert not np.array_equal(after[v][2020 - Y0], before[v][2020 - Y0]), v
        assert np.array_equal(after[v][:2020 - Y0], before[v][:2020 - Y0]), v
    c.shutdown()


# ---------------------------------------------------------------------------------------------
# the host-build tier

@pytest.mark.parametrize("flavour", ["run", "b4"])
def test_shipped_ssps_are_members_of_one_core(emul_lib, oracle, flavour):
    check_ssp_members(emul_lib, flavour, N_HOST, HOST)


@pytest.mark.parametrize("name", NAMES)
def test_each_name_alone_vs_oracle(emul_lib, oracle, tmp_path, name):
    check_one_name(emul_lib, tmp_path, name, N_HOST, HOST)


def test_one_vector_at_the_scenario_ends_vs_oracle(emul_lib, oracle, tmp_path):
    check_mixes_vs_oracle(emul_lib, tmp_path, "run", N_HOST, HOST, edge_mixes(N_HOST), "edges")


@pytest.mark.parametrize("flavour", ["run", "run2", "b4"])
def test_identity_mixes_change_no_bit(emul_lib, flavour):
    check_identity_mixes(emul_lib, flavour, N_HOST, HOST)


def test_results_do_not_depend_on_how_the_core_got_there(emul_lib):
    check_invariances(emul_lib, N_HOST, HOST)


def test_refused_calls_change_nothing(emul_lib, tmp_path):
    check_refusals(emul_lib, tmp_path, N_HOST, HOST)
