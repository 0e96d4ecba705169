"""Mixes of the inputs the gas pre-pass reads -- N2O_emissions, RF_albedo and the <gas>_emissions of
the scenario's halocarbons (hx_setvar_dated_mix) -- and whole scenarios as members of one core
(hx_setvar_scenario_mix / Core.setvar_scenarios).

These names never have a table of emissions: the host keeps the recipe, and hx_gas_mix_kernel
evaluates it where the N2O and halocarbon recurrences read the value, ahead of the year loop, and
writes the two rows the extended run kernels take (N2O; halocarbon + albedo + misc forcing).  The
yardstick is the oracle reading a scenario pack that carries the member's own series
(conftest.edited_pack), at the project's tolerances: deviation / max(1, max|ref|) < 2e-8 for every
row (outputs_matrix.TOL), N2O_concentration 1e-12 relative (tests/test_member_gas_params.py), CH4
1e-6 ppbv, the stash schedule identical.

The aerosol and ozone / OH precursor emissions are NOT mixable, so the shipped SSPs are refused
against each other (they differ in so2.SO2_emissions among others).  The scenarios of the acceptance
test are therefore the shipped ssp126 / ssp245 / ssp585 / ssp119 reduced to what a core on ssp245
can hold per member: ssp245 with every mixable series of the other scenario.

S is unsorted (test_member_series.member_S), so the lane order is a real permutation of the member
order.  This file: the helpers and the host-build tier (tests/emul, 70 members: two wavefronts, six
real lanes in the second).  tests/test_gpu_member_gas_mix.py: the same on the device, 130 members."""
import os

import numpy as np
import pytest

import hector_amd
import outputs_matrix as om
from conftest import SCENARIO, edited_pack
from test_member_mix import assert_equal_results, restate
from test_member_series import (BITWISE, END, FLAVOURS, WAVE, Y0, assert_flavour, checked_members, make_core,
                                member_S)

N_HOST = 70
HOST = dict(allow_emulation=True)
Error = hector_amd.HectorAmdError
TOL = om.TOL
DATA = os.path.dirname(SCENARIO)
OLD_NAMES = ["ffi_emissions", "daccs_uptake", "luc_emissions", "luc_uptake", "CH4_emissions"]
WITH_EMISSIONS, WITHOUT_EMISSIONS = "HFC134a", "CH3CCl3"   # SSP emissions after 2030: some / none
NEW_NAMES = ["N2O_emissions", "RF_albedo", WITH_EMISSIONS + "_emissions", WITHOUT_EMISSIONS + "_emissions"]
UNIT = {"N2O_emissions": "Tg N", "RF_albedo": "W/m2", WITH_EMISSIONS + "_emissions": "Gg",
        WITHOUT_EMISSIONS + "_emissions": "Gg"}
SECTION = {"N2O_emissions": "N2O", "RF_albedo": "simpleNbox",
           WITH_EMISSIONS + "_emissions": WITH_EMISSIONS + "_halocarbon",
           WITHOUT_EMISSIONS + "_emissions": WITHOUT_EMISSIONS + "_halocarbon"}
# what the core records, what fetchvars answers besides, and what the oracle is asked for
RECORDED = BITWISE + ["N2O_concentration", "RF_N2O"]
HOST_DIAG = ["RF_albedo", "RF_" + WITH_EMISSIONS, WITH_EMISSIONS + "_concentration",
             "RF_" + WITHOUT_EMISSIONS, WITHOUT_EMISSIONS + "_concentration"]
ORACLE_ROWS = ["CO2_concentration", "global_tas", "RF_tot", "RF_N2O", "RF_albedo", "RF_halocarbons"]
MIX_YEARS = np.arange(2030, 2101)
BASE_YEAR = 1750   # [forcing] baseyear of the shipped scenarios


# ---------------------------------------------------------------------------------------------
# scenario packs as data

def pack_series(path):
    """{(section, key): values[ns]} of a scenario pack."""
    out = {}
    with open(path) as f:
        for line in f:
            p = line.split()
            if len(p) > 5 and p[0] == "series":
                out[(p[1], p[2])] = np.array([float(x) for x in p[5:5 + int(p[4])]])
    return out


def halocarbons():
    return [sec[:-len("_halocarbon")] for sec, _ in pack_series(SCENARIO) if sec.endswith("_halocarbon")]


def mixable():
    """Every name the mix verb takes for a core on the shipped scenario."""
    return OLD_NAMES + ["N2O_emissions", "RF_albedo"] + [h + "_emissions" for h in halocarbons()]


def reduced_scenario(path, donor):
    """ssp245 with every MIXABLE series of the shipped scenario `donor` (the donor's own text, so
    its own bits) -> path.  What a member of a core on ssp245 can hold of that scenario."""
    take = set(mixable())
    theirs = {}
    with open(os.path.join(DATA, donor + ".hxs")) as f:
        for line in f:
            p = line.split(None, 3)
            if len(p) > 3 and p[0] == "series" and p[2] in take:
                theirs[(p[1], p[2])] = line
    out = []
    with open(SCENARIO) as f:
        for line in f:
            p = line.split(None, 3)
            if len(p) > 3 and p[0] == "series" and (p[1], p[2]) in theirs:
                line = theirs[(p[1], p[2])]
            out.append(line)
    with open(path, "w") as f:
        f.writelines(out)
    return str(path)


# ---------------------------------------------------------------------------------------------
# the core side

def gas_core(lib, fl, n, kw, sorting=True, params=None):
    c = make_core(lib, fl, n, kw, sorting=sorting)
    c.set_outputs(RECORDED)
    if params:
        om.set_members(c, params, fl["B"])
    return c


def member_params(n):
    """S unsorted, and aero_scalar, q10_rh, beta from outputs_matrix.RANGES, drawn together."""
    rng = np.random.default_rng(20261020)
    v = {k: rng.uniform(*om.RANGES[k], n) for k in ("aero_scalar", "q10_rh", "beta")}
    v["S"] = member_S(n)
    return v


def result(c, fl=None, run_to=END, inputs=NEW_NAMES):
    if fl is not None:
        assert_flavour(c, fl)
    r = {v: c.fetchvars(v, (Y0, run_to)).copy() for v in RECORDED + HOST_DIAG}
    r["status"] = c.status().copy()
    for name in inputs:
        r["in:" + name] = c.fetchvars(name, (Y0, END)).copy()
    for a in r.values():
        a.setflags(write=False)
    return r


def spread_members(c, n, count=8):
    """`count` members that sit in every wavefront, the ragged one's last lane among them."""
    lanes = c.lane_of_member()
    assert not np.array_equal(lanes, np.arange(n)), "lane order is the member order"
    member_at = np.argsort(lanes)
    waves = (n + WAVE - 1) // WAVE
    want = sorted({w * WAVE + k for w in range(waves) for k in (0, 1, 33) if w * WAVE + k < n} | {n - 1})
    want += [l for l in range(7, n, 11) if l not in want][:max(0, count - len(want))]
    got = [int(member_at[l]) for l in want]
    assert len(got) >= count
    assert {int(lanes[i]) // WAVE for i in got} == set(range(waves))
    return got


_ORACLE = {}


def oracle_run(pack, key, params, i, B, run_to=END):
    """Member i with its parameters on the oracle reading `pack`; once per key."""
    import oracle_binding
    if key not in _ORACLE:
        o = oracle_binding.Oracle(pack)
        p = om.oracle_member(o, params, i, B)
        r, err, _ = o.run(p, run_to)
        k = run_to - Y0 + 1
        res = {v: r[v][:k].copy() for v in ORACLE_ROWS + ["CH4_concentration", "N2O_concentration", "timesteps"]}
        res["err"] = err
        o.lib.hxo_scenario_free(o.sc)
        _ORACLE[key] = res
    return _ORACLE[key]


def fetched(c, run_to=END):
    """What is held to the oracle, [year, member]: the rows of ORACLE_ROWS (RF_halocarbons as the sum
    of the gases' forcings in the order the forcing component adds them up), CH4, N2O, timesteps."""
    got = {v: c.fetchvars(v, (Y0, run_to)) for v in ORACLE_ROWS[:-1] + ["CH4_concentration", "N2O_concentration",
                                                                       "timesteps"]}
    got["RF_halocarbons"] = sum(c.fetchvars("RF_" + h, (Y0, run_to)) for h in sorted(c.halocarbons()))
    return got


def assert_member_vs_oracle(got, i, r, what):
    """The project's tolerances; prints every figure before it asserts."""
    assert r["err"] == 0, (what, i, r["err"])
    fig = {}
    for v in ORACLE_ROWS:
        # RF_albedo names the INPUT series as well, and fetchvars answers with that: the same as the
        # forcing from its base year on (the input is 0 there), where the reference reports 0 before
        j = BASE_YEAR - Y0 if v == "RF_albedo" else 0
        fig[v] = np.abs(got[v][j:, i] - r[v][j:]).max() / max(1.0, np.abs(r[v]).max())
    fig["N2O rel"] = (np.abs(got["N2O_concentration"][:, i] - r["N2O_concentration"]) / r["N2O_concentration"]).max()
    fig["CH4 ppbv"] = np.abs(got["CH4_concentration"][:, i] - r["CH4_concentration"]).max()
    print("gas mix vs oracle [%s] member %d: %s" % (what, i, ", ".join("%s %.2e" % kv for kv in fig.items())))
    for v in ORACLE_ROWS:
        assert fig[v] < TOL, (what, i, v, fig[v])
    assert fig["N2O rel"] < 1e-12, (what, i, fig["N2O rel"])
    assert fig["CH4 ppbv"] < 1e-6, (what, i, fig["CH4 ppbv"])
    assert np.array_equal(got["timesteps"][1:, i], r["timesteps"][1:]), (what, i)


# ---------------------------------------------------------------------------------------------
# 1. scenario membership equals the scenario

SCENARIOS = ["ssp126", "ssp245", "ssp585", "ssp119"]


def scenario_labels(n):
    return np.random.default_rng(5).permutation(np.arange(n) % len(SCENARIOS)).astype(np.int64)


_REDUCED = {}


def reduced_scenarios(tmp):
    if "paths" not in _REDUCED:
        _REDUCED["paths"] = [reduced_scenario(os.path.join(str(tmp), s + "_reduced.hxs"), s) for s in SCENARIOS]
    return _REDUCED["paths"]


def check_scenario_members(lib, oracle_dir, flavour, n, kw):
    """Four scenarios in one core on ssp245 through integer labels; every checked member against the
    oracle reading ITS scenario's pack with its parameters."""
    fl = FLAVOURS[flavour]
    paths = reduced_scenarios(oracle_dir)
    params, labels = member_params(n), scenario_labels(n)
    c = gas_core(lib, fl, n, kw, params=params)
    nseries = c.setvar_scenarios(paths, labels)
    ssp245 = pack_series(SCENARIO)
    differing = {k[1] for p in paths for k, v in pack_series(p).items() if not np.array_equal(v, ssp245[k])}
    assert nseries == len(differing) and differing <= set(mixable()) and "N2O_emissions" in differing
    c.run(END)
    assert_flavour(c, fl)
    assert (c.status() == 0).all(), np.flatnonzero(c.status())
    # one-hot coefficients: a member's inputs are its scenario's own bits
    for name in ("N2O_emissions", "RF_albedo", WITH_EMISSIONS + "_emissions", "ffi_emissions"):
        back = c.fetchvars(name, (Y0, END))
        for g, p in enumerate(paths):
            want = [v for k, v in pack_series(p).items() if k[1] == name][0]
            assert np.array_equal(back[:, labels == g], np.repeat(want[:, None], (labels == g).sum(), 1)), (name, g)
    got = fetched(c)
    for i in checked_members(c, n, every=False):
        g = int(labels[i])
        r = oracle_run(paths[g], ("scen", n, fl["B"], i), params, i, fl["B"])
        assert_member_vs_oracle(got, i, r, "%s %s" % (flavour, SCENARIOS[g]))
    # not vacuous: the four groups differ in what only the new names carry
    at = 2100 - Y0
    halo = [got["RF_halocarbons"][at, labels == g] for g in range(len(SCENARIOS))]
    n2o = [got["N2O_concentration"][at, labels == g] for g in range(len(SCENARIOS))]
    for rows in (halo, n2o):
        assert all(np.ptp(x) == 0.0 for x in rows)   # (no parameter reaches these rows)
        vals = sorted(x[0] for x in rows)
        assert np.diff(vals).min() > 1000 * TOL, vals
    c.shutdown()


# ---------------------------------------------------------------------------------------------
# 2. each name alone

def level_of(name, years):
    """The scenario's own series in `years`; for the gas whose SSP emissions are zero there, 2 % of
    its own historical peak instead (the mix is then its only source)."""
    own = pack_series(SCENARIO)[(SECTION[name], name)]
    v = own[years - Y0]
    return v if np.abs(v).min() > 0 else np.where(v != 0, v, 0.02 * own.max())


def one_mix(rng, name, years, n, K):
    """Leading vector: the scenario's series times an independent factor 0.5..1.5 per year (a row
    written to the wrong year shows); the others +-5 % of it; coefficients 0.7..1.3 and +-1.  Every
    resulting value keeps the sign of the scenario's (emissions positive, RF_albedo negative)."""
    lead = level_of(name, years) * rng.uniform(0.5, 1.5, years.size)
    basis = np.vstack([lead[None, :]] + [lead[None, :] * rng.uniform(-0.05, 0.05, (1, years.size)) for _ in range(K - 1)])
    coeff = np.vstack([rng.uniform(0.7, 1.3, (1, n)), rng.uniform(-1.0, 1.0, (K - 1, n))])
    sign = -1.0 if name == "RF_albedo" else 1.0
    assert (sign * restate(basis, coeff)).min() > 0.0, name
    return (name, years, basis, coeff)


def set_mixes(c, mixes):
    for name, years, basis, coeff in mixes:
        assert c.setvar_dated_mix(name, years, basis, coeff, UNIT[name]) is c


def member_pack(path, mixes, i):
    cur = None
    for name, years, basis, coeff in mixes:
        cur = edited_pack(path, SECTION[name], name, years, restate(basis, coeff)[:, i], base=cur)
    return cur


OWN_DIAGNOSTIC = {"N2O_emissions": "RF_N2O", "RF_albedo": "RF_albedo",
                  WITH_EMISSIONS + "_emissions": "RF_" + WITH_EMISSIONS,
                  WITHOUT_EMISSIONS + "_emissions": "RF_" + WITHOUT_EMISSIONS}


def check_mixes_vs_oracle(lib, tmp_path, flavour, n, kw, mixes, what, moved=()):
    fl = FLAVOURS[flavour]
    params = {"S": member_S(n)}
    c = gas_core(lib, fl, n, kw)
    set_mixes(c, mixes)
    c.run(END)
    assert_flavour(c, fl)
    assert (c.status() == 0).all()
    for name, years, basis, coeff in mixes:   # the inputs are the definition's bits
        assert np.array_equal(c.fetchvars(name, (Y0, END))[years - Y0], restate(basis, coeff)), name
    got = fetched(c)
    for i in spread_members(c, n):
        r = oracle_run(member_pack(tmp_path / "m.hxs", mixes, i), (what, n, i), params, i, fl["B"])
        assert_member_vs_oracle(got, i, r, what)
    for name in moved:   # the name moved its own diagnostic
        d = c.fetchvars(OWN_DIAGNOSTIC[name], (2100, 2100))[0]
        assert np.ptp(d) > 1000 * TOL, (name, np.ptp(d))
    res = result(c, fl)
    c.shutdown()
    return res


def check_one_name(lib, tmp_path, name, n, kw):
    mix = one_mix(np.random.default_rng(NEW_NAMES.index(name) + 300), name, MIX_YEARS, n, 3)
    check_mixes_vs_oracle(lib, tmp_path, "run", n, kw, [mix], "alone:" + name, moved=[name])


# ---------------------------------------------------------------------------------------------
# 3. edges

def edge_mixes(n):
    """K = 1, a year list with gaps, out of order, that holds startDate and endDate: N2O_emissions,
    RF_albedo (the pre-pass's row 0 is per member) and one halocarbon."""
    rng = np.random.default_rng(310)
    years = np.array([END, Y0, 2000, Y0 + 1, 2100, END - 1])
    out = []
    for name, early, late in (("N2O_emissions", 0.06, 6.0), ("RF_albedo", -0.01, -0.2),
                              (WITH_EMISSIONS + "_emissions", 0.5, 150.0)):
        basis = np.where(years > 1900, late, early) * rng.uniform(0.5, 1.5, years.size)
        out.append((name, years, basis[None, :], rng.uniform(0.5, 1.5, (1, n))))
    return out


# ---------------------------------------------------------------------------------------------
# 4. invariances, bit for bit

def standard_mixes(n, seed=320):
    rng = np.random.default_rng(seed)
    return [one_mix(rng, name, MIX_YEARS, n, 3) for name in NEW_NAMES]


_REF = {}


def straight_run(lib, n, kw):
    """A fresh core with all four new names mixed, run to END in one go; once per (lib, n)."""
    if (lib, n) not in _REF:
        fl = FLAVOURS["run"]
        c = gas_core(lib, fl, n, kw)
        set_mixes(c, standard_mixes(n))
        c.run(END)
        _REF[(lib, n)] = result(c, fl)
        assert (_REF[(lib, n)]["status"] == 0).all()
        c.shutdown()
    return _REF[(lib, n)]


def check_invariances(lib, n, kw):
    fl = FLAVOURS["run"]
    mixes = standard_mixes(n)
    ref = straight_run(lib, n, kw)
    # sorting off: the member order is the lane order
    c = gas_core(lib, fl, n, kw, sorting=False)
    set_mixes(c, mixes)
    c.run(END)
    assert np.array_equal(c.lane_of_member(), np.arange(n))
    assert_equal_results(result(c, fl), ref, "sorting off")
    # ... after a reset
    c.reset(Y0)
    c.run(END)
    assert_equal_results(result(c, fl), ref, "after reset")
    c.shutdown()
    # in segments, with the state history; then new coefficients and the old ones again
    c = gas_core(lib, fl, n, kw)
    c.enable_history(True)
    set_mixes(c, mixes)
    for y in om.SEGMENTS:
        c.run(y)
    assert_equal_results(result(c, fl), ref, "segments with history")
    other = [(nm, y, b, w * np.random.default_rng(321).uniform(0.97, 1.03, w.shape)) for nm, y, b, w in mixes]
    set_mixes(c, other)
    c.run(END)
    changed = result(c, fl)
    for v in RECORDED:   # the core went back to 2029 by itself
        assert np.array_equal(changed[v][:2030 - Y0], ref[v][:2030 - Y0]), v
    assert not np.array_equal(changed["N2O_concentration"], ref["N2O_concentration"])
    assert not np.array_equal(changed["RF_" + WITH_EMISSIONS], ref["RF_" + WITH_EMISSIONS])
    set_mixes(c, mixes)
    c.run(END)
    assert_equal_results(result(c, fl), ref, "coefficients replaced and put back")
    # clear_mix of every new name: the results, and the kernel, of a core that never had one
    for name in NEW_NAMES:
        assert c.clear_mix(name) is c
    c.run(END)
    p = gas_core(lib, fl, n, kw)
    p.enable_history(True)
    p.run(END)
    plain = dict(fl, variant=0)
    assert_equal_results(result(c, plain), result(p, plain), "mixes removed")
    c.shutdown(); p.shutdown()


# ---------------------------------------------------------------------------------------------
# the host-build tier

@pytest.fixture(scope="module")
def scen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("reduced_scenarios")


@pytest.mark.parametrize("flavour", ["run", "b4"])
def test_scenario_members_equal_their_scenarios(emul_lib, oracle, scen_dir, flavour):
    check_scenario_members(emul_lib, scen_dir, flavour, N_HOST, HOST)


@pytest.mark.parametrize("name", NEW_NAMES)
def test_each_name_alone_vs_oracle(emul_lib, oracle, tmp_path, name):
    check_one_name(emul_lib, tmp_path, name, N_HOST, HOST)


def test_one_vector_at_the_scenario_ends_vs_oracle(emul_lib, oracle, tmp_path):
    check_mixes_vs_oracle(emul_lib, tmp_path, "run", N_HOST, HOST, edge_mixes(N_HOST), "edges")


def test_results_do_not_depend_on_how_the_core_got_there(emul_lib):
    check_invariances(emul_lib, N_HOST, HOST)


def test_mix_capabilities_lists_the_names_of_this_core(emul_lib):
    c = hector_amd.Core(SCENARIO, 3, lib_path=emul_lib, **HOST)
    caps = c.mix_capabilities()
    assert caps == OLD_NAMES + ["N2O_emissions", "RF_albedo"] + [h + "_emissions" for h in c.halocarbons()]
    assert sorted(caps) == sorted(mixable()) and len(caps) == 5 + 2 + 26
    for name in caps:   # ... and every one of them is taken (nbasis = 0: nothing to remove, no error)
        assert c.clear_mix(name) is c
    c.shutdown()


def run_to_2100(c):
    c.run(2100)
    return result(c, run_to=2100)


def test_refused_calls_change_nothing(emul_lib, scen_dir, tmp_path):
    n, fl = N_HOST, FLAVOURS["run"]
    c = gas_core(emul_lib, fl, n, HOST)
    mixes = standard_mixes(n)
    set_mixes(c, mixes)
    before = run_to_2100(c)

    def unchanged(what):
        for name in NEW_NAMES:
            assert np.array_equal(c.fetchvars(name, (Y0, END)), before["in:" + name]), (what, name)

    yrs, vals = np.array([2050, 2051]), np.ones((2, n))
    # the dense verb still refuses the names, the old way
    for name in ("N2O_emissions", "RF_albedo", WITH_EMISSIONS + "_emissions", "SO2_emissions", "SV"):
        with pytest.raises(Error, match="per-member dated input not supported for " + name):
            c.setvar_dated_members(name, yrs, vals)
    # the mix verb refuses what no pre-pass or kernel reads per member, and says what it takes
    for name in ("SV", "RF_misc", "CH4N", "N2O_natural_emissions", "SO2_emissions", "NOX_emissions",
                 "CFC999_emissions"):
        with pytest.raises(Error, match=r"hx_setvar_dated_mix: .*ffi_emissions, daccs_uptake, luc_emissions, "
                                        r"luc_uptake, CH4_emissions, N2O_emissions, RF_albedo"):
            c.setvar_dated_mix(name, yrs, np.ones((2, 2)), np.ones((2, n)))
    with pytest.raises(Error, match="hx_setvar_dated_mix: Units"):
        c.setvar_dated_mix("N2O_emissions", yrs, np.ones((2, 2)), np.ones((2, n)), "Gg")
    with pytest.raises(Error, match="hx_setvar_dated_mix: .*twice"):
        c.setvar_dated_mix("RF_albedo", [2050, 2050], np.ones((2, 2)), np.ones((2, n)))
    # a shared edit: refused in a covered year, taken in another
    for name in NEW_NAMES:
        with pytest.raises(Error, match=r"hx_setvar_dated: .*remove the mix first"):
            c.setvar_dated(name, [2029, 2030], [1.0, 1.0], UNIT[name])
    unchanged("refused verbs")
    # whole scenarios
    reduced = reduced_scenarios(scen_dir)
    shipped = [os.path.join(DATA, s + ".hxs") for s in SCENARIOS]
    lab = scenario_labels(n)
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*so2\.SO2_emissions"):
        c.setvar_scenarios(shipped, lab)
    # picontrol: other aerosol efficiencies (scalars, found first), a CO2 constraint, other SV and CH4N
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: scalar rho_bc of section forcing .*picontrol"):
        c.setvar_scenarios([os.path.join(DATA, "picontrol.hxs"), SCENARIO], lab % 2)
    # ... and each kind of series alone: a constraint the core does not hold, another SV, another CH4N
    for sec, key, val, word in (("simpleNbox", "CO2_constrain", 400.0, "missing on one side"),
                                ("so2", "SV", -1.0, "cannot be a mix"), ("CH4", "CH4N", 300.0, "cannot be a mix")):
        other = edited_pack(tmp_path / "other.hxs", sec, key, [2050], [val], base=reduced[0])
        with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*%s\.%s" % (sec, key)) as e:
            c.setvar_scenarios([other, reduced[1]], lab % 2)
        assert word in str(e.value), (key, str(e.value))
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*nscen = 9"):
        c.setvar_scenarios([SCENARIO] * 9, lab)
    with pytest.raises(Error, match="setvar_scenarios: coeff must be"):
        c.setvar_scenarios(reduced, np.ones((3, n)))
    with pytest.raises(Error, match="setvar_scenarios: a label"):
        c.setvar_scenarios(reduced, lab + 1)
    changed = edited_pack(tmp_path / "scalar.hxs", None, None, [], [], base=reduced[0],
                          scalars={("N2O", "TN2O0"): 131.0})
    with pytest.raises(Error, match=r"hx_setvar_scenario_mix: .*TN2O0 of section N2O"):
        c.setvar_scenarios([changed, reduced[1]], lab % 2)
    bad = np.ones((4, n))
    bad[2, n - 1] = np.nan
    with pytest.raises(Error, match="hx_setvar_scenario_mix: .*finite"):
        c.setvar_scenarios(reduced, bad)
    unchanged("refused scenarios")
    # nothing was dirtied: the results stand, and a new run repeats them
    assert_equal_results(result(c, fl, run_to=2100), before, "after the refused calls")
    c.reset(Y0)
    assert_equal_results(run_to_2100(c), before, "a run after the refused calls")
    # a shared edit in an uncovered year shows, next to the mix
    c.setvar_dated("N2O_emissions", [2020, 2021], [9.0, 9.5], UNIT["N2O_emissions"])
    after = run_to_2100(c)
    assert (after["in:N2O_emissions"][2020 - Y0] == 9.0).all()
    assert np.array_equal(after["in:N2O_emissions"][MIX_YEARS - Y0], before["in:N2O_emissions"][MIX_YEARS - Y0])
    assert not np.array_equal(after["N2O_concentration"][2022 - Y0], before["N2O_concentration"][2022 - Y0])
    c.shutdown()
