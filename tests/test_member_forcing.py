"""Forcing efficacies that differ between members (Core.enable_member_forcing): delta_co2, delta_ch4,
delta_n2o enter the year loop of the extended run kernels as three values per lane, rho_bc, rho_oc,
rho_so2, rho_nh3 the aerosol row of the lane-per-member pre-pass (hx_slcf_mix_kernel).  Every
member against the oracle, which reads the member's values as scalars of a scenario of its own;
tolerances as in test_member_gas_params / test_one_factor.check_vs_oracle: CO2 2e-8 relative,
global_tas and RF_tot 2e-8 absolute, identical timesteps; the forcings the host or the diagnostic
kernel derives (RF_BC .. RF_N2O) 1e-10, RF_CO2 2e-8."""
import numpy as np
import pytest

import hector_amd
from conftest import SCENARIO, edited_pack
from test_one_factor import FLAVOURS, HOST_FLAVOURS, OUTS, TRACK_DATE

Y0, RUN_TO = 1745, 2100
UNITS = {"delta_co2": "(unitless)", "delta_ch4": "(unitless)", "delta_n2o": "(unitless)",
         "rho_bc": "W/m2/Tg", "rho_oc": "W/m2/Tg", "rho_so2": "W/m2/Gg", "rho_nh3": "W/m2/Tg"}
NAMES = list(UNITS)
RFS = ["RF_CO2", "RF_CH4", "RF_N2O", "RF_BC", "RF_OC", "RF_SO2", "RF_NH3"]
TOL = {"RF_CO2": 2e-8, "RF_CH4": 1e-10, "RF_N2O": 1e-10, "RF_BC": 1e-10, "RF_OC": 1e-10, "RF_SO2": 1e-10,
       "RF_NH3": 1e-10, "global_tas": 2e-8, "RF_tot": 2e-8}
_BASE = {}


def scenario_values(lib, **kw):
    """The scenario's own seven values, as getvar returns them."""
    if "v" not in _BASE:
        c = hector_amd.Core(SCENARIO, 1, lib_path=lib, **kw)
        _BASE["v"] = {k: float(c.getvar(k)[0]) for k in NAMES}
    return _BASE["v"]


def draws(base, n, seed=20261020, names=NAMES):
    """delta_* in +-0.2, rho_* x 0.5..1.5, S in 2..5; the names not listed stay the scenario's."""
    rng = np.random.default_rng(seed)
    vals = {}
    for k in NAMES:   # (every name draws, listed or not: a member's values do not depend on `names`)
        u = rng.uniform(size=n)
        v = -0.2 + 0.4 * u if k.startswith("delta") else base[k] * (0.5 + u)
        if k in names:
            vals[k] = v
    return vals, 2.0 + 3.0 * rng.uniform(size=n)


def forcing_core(lib, fl, vals, S, run_to=RUN_TO, path=SCENARIO, switch=True, run=True, outs=(), **kw):
    """A core on flavour `fl` with the per-member efficacies `vals` and sensitivities S."""
    c = hector_amd.Core(path, len(S), lib_path=lib, **kw)
    B = fl["B"]
    if B > 1:
        c.split_biome(["b%d" % b for b in range(B)])
    c.set_pair_kernel_limit(fl["pair"]).set_two_wave_from(fl["w2"])
    if fl.get("track"):
        c.setvar("trackingDate", [TRACK_DATE])
    if switch:
        c.enable_member_forcing()
    for k, v in vals.items():
        c.setvar(k, v, UNITS[k])
    c.setvar("S", S, "degC")
    c.set_outputs(OUTS + RFS[:3] + fl.get("outs", []) + list(outs))
    if run:
        c.run(run_to)
    return c


def expect_kernel(c, fl):
    """The flavour's own kernel ran, in an instantiation that carries per-member rows: the
    extended run kernels (with or without the NBP machinery), the tracking kernel, or the
    small-ensemble pair kernel with its constraint code."""
    assert c.last_run_kernel() == fl["kernel"], (c.last_run_kernel(), fl)
    assert c.last_run_variant() in ((2,) if fl.get("track") else (-1, 1)), (c.last_run_variant(), fl)
    assert len(c.biomes()) == fl["B"]


_ORACLE = {}


def oracle_member(tmp_path, member_vals, S, B, run_to=RUN_TO, base=None, tag=""):
    """The oracle on a scenario that holds `member_vals` {name: value} as [forcing] scalars."""
    import oracle_binding
    key = (tuple(sorted((k, float(v)) for k, v in member_vals.items())), float(S), B, run_to, base, tag)
    if key not in _ORACLE:
        path = edited_pack(tmp_path / ("m%d.hxs" % len(_ORACLE)), None, None, [], [], base=base,
                           scalars={("forcing", k): v for k, v in member_vals.items()})
        o = oracle_binding.Oracle(path)
        p = o.default_params()
        if B > 1:
            p = o.split_equal(p, B)
        p.S = S
        p.nbiome = B
        r, err, _ = o.run(p, run_to=run_to)
        assert err == 0
        _ORACLE[key] = r
    return _ORACLE[key]


def check_members_vs_oracle(c, tmp_path, vals, S, B, where, run_to=RUN_TO, members=None, base=None, tag=""):
    nk = run_to - Y0 + 1
    got = {v: c.fetchvars(v, (Y0, run_to)) for v in ["CO2_concentration"] + list(TOL)}
    ts = c.fetchvars("timesteps", (Y0 + 1, run_to))
    assert (c.status() == 0).all(), where
    for i in (range(len(S)) if members is None else members):
        r = oracle_member(tmp_path, {k: v[i] for k, v in vals.items()}, S[i], B, run_to, base, tag)
        ref = r["CO2_concentration"][:nk]
        dev = np.abs(got["CO2_concentration"][:, i] - ref).max() / np.abs(ref).max()
        assert dev < 2e-8, (where, i, "CO2_concentration", dev)
        for v, tol in TOL.items():
            dev = np.abs(got[v][:, i] - r[v][:nk]).max()
            assert dev < tol, (where, i, v, dev)
        assert np.array_equal(ts[:, i], r["timesteps"][1:nk]), (where, i, "timesteps")


def all_outputs(c, fl, run_to=RUN_TO):
    return {v: c.fetchvars(v, (Y0, run_to)) for v in OUTS + RFS + fl.get("outs", [])}


def set_env(monkeypatch, fl):
    for k, v in fl.get("env", {}).items():
        monkeypatch.setenv(k, v)


# ---- the switch ------------------------------------------------------------------------------------
def test_switch_semantics(emul_lib):
    kw = dict(lib_path=emul_lib, allow_emulation=True)
    base = scenario_values(emul_lib, allow_emulation=True)
    c = hector_amd.Core(SCENARIO, 3, **kw)
    for k in NAMES:   # off: the refusal is what it always was
        with pytest.raises(hector_amd.HectorAmdError, match="%s belongs to a member-independent component: one "
                                                            "value for the whole core" % k):
            c.setvar(k, [0.1, 0.2, 0.3])
        assert np.array_equal(c.getvar(k), np.full(3, base[k]))
    assert c.enable_member_forcing() is c
    for j, k in enumerate(NAMES):
        v = np.array([0.01, 0.02, 0.03]) * (j + 1)
        with pytest.raises(hector_amd.HectorAmdError, match="[Uu]nits"):
            c.setvar(k, v, "degC")
        assert np.array_equal(c.getvar(k), np.full(3, base[k]))   # (a refused call changes nothing)
        c.setvar(k, v, UNITS[k])
        assert np.array_equal(c.getvar(k), v)
    with pytest.raises(hector_amd.HectorAmdError, match="member-independent"):
        c.setvar("M0", [700.0, 710.0, 720.0])    # out of scope: core-wide as before
    with pytest.raises(hector_amd.HectorAmdError, match="need 1 or n_members"):
        c.setvar("rho_bc", [0.1, 0.2])
    # on == 0 while a vector exists: refused, naming what differs, and nothing changes
    with pytest.raises(hector_amd.HectorAmdError, match="hx_enable_member_forcing: delta_co2, delta_ch4, "
                                                        "delta_n2o, rho_bc, rho_oc, rho_so2, rho_nh3"):
        c.enable_member_forcing(False)
    assert np.array_equal(c.getvar("rho_nh3"), np.array([0.01, 0.02, 0.03]) * 7)
    # an all-equal vector, or one value, puts a name back on the shared path
    for k in NAMES[:6]:
        c.setvar(k, [base[k]] * 3, UNITS[k])
        assert np.array_equal(c.getvar(k), np.full(3, base[k]))
    with pytest.raises(hector_amd.HectorAmdError, match="hx_enable_member_forcing: rho_nh3 differs"):
        c.enable_member_forcing(False)
    c.setvar("rho_nh3", base["rho_nh3"], UNITS["rho_nh3"])
    c.enable_member_forcing(False)
    with pytest.raises(hector_amd.HectorAmdError, match="member-independent"):
        c.setvar("delta_co2", [0.1, 0.2, 0.3])


def test_delta_out_of_range_in_one_member_is_refused_naming_it(emul_lib):
    c = hector_amd.Core(SCENARIO, 4, lib_path=emul_lib, allow_emulation=True).enable_member_forcing()
    c.setvar("delta_co2", [0.0, 0.5, 1.25, -3.0])
    with pytest.raises(hector_amd.HectorAmdError, match=r"bad delta CO2 value \(member 2\)"):
        c.run(1750)
    c.setvar("delta_co2", [0.0, 0.5, 1.0, -1.0]).setvar("delta_n2o", [0.0, -1.5, 0.0, 0.0])
    with pytest.raises(hector_amd.HectorAmdError, match=r"bad delta N2O value \(member 1\)"):
        c.run(1750)
    c.setvar("delta_n2o", [0.0, -1.0, 0.0, 0.0])
    c.run(1750)
    assert (c.status() == 0).all()


def test_several_shards_split_the_vectors(emul_lib):
    n = 6
    base = scenario_values(emul_lib, allow_emulation=True)
    vals, S = draws(base, n)
    # (members 0..1, the first shard's, share their rho_oc: that shard holds it as one value)
    vals["rho_oc"][:2] = vals["rho_oc"][0]
    fl = FLAVOURS["run"]
    one = forcing_core(emul_lib, fl, vals, S, 1850, allow_emulation=True)
    many = forcing_core(emul_lib, fl, vals, S, 1850, allow_emulation=True, devices=[0, 0, 0])
    for k in NAMES:
        assert np.array_equal(many.getvar(k), vals[k]), k
    for v in OUTS + RFS:
        assert np.array_equal(many.fetchvars(v, (Y0, 1850)), one.fetchvars(v, (Y0, 1850))), v
    with pytest.raises(hector_amd.HectorAmdError, match="hx_enable_member_forcing: delta_co2"):
        many.enable_member_forcing(False)
    assert np.array_equal(many.getvar("rho_so2"), vals["rho_so2"])


# ---- against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", HOST_FLAVOURS)
def test_all_seven_per_member_vs_oracle(emul_lib, tmp_path, monkeypatch, flavour):
    fl = FLAVOURS[flavour]
    set_env(monkeypatch, fl)
    vals, S = draws(scenario_values(emul_lib, allow_emulation=True), 8)
    c = forcing_core(emul_lib, fl, vals, S, allow_emulation=True)
    expect_kernel(c, fl)
    for k in NAMES:
        assert np.array_equal(c.getvar(k), vals[k])
    check_members_vs_oracle(c, tmp_path, vals, S, fl["B"], flavour)


@pytest.mark.parametrize("name", NAMES)
def test_each_name_varied_alone_is_felt(emul_lib, tmp_path, name):
    base = scenario_values(emul_lib, allow_emulation=True)
    vals, _ = draws(base, 4, names=[name])
    S = np.full(4, 3.0)
    c = forcing_core(emul_lib, FLAVOURS["run"], vals, S, allow_emulation=True)
    assert np.ptp(c.fetchvars("RF_tot", (RUN_TO, RUN_TO))[0]) > 0, name
    assert np.ptp(c.fetchvars("global_tas", (RUN_TO, RUN_TO))[0]) > 0, name
    for k in NAMES:
        assert np.array_equal(c.getvar(k), vals[k] if k == name else np.full(4, base[k])), (name, k)
    check_members_vs_oracle(c, tmp_path, vals, S, 1, name)


def own_values_identity(lib, monkeypatch, flavour, n=8, **kw):
    """Members that hold the scenario's own seven values have the bits of a core without
    per-member values that runs the same kernel variant.  The run kernels: the extended
    instantiation for both cores (a diagnostic output and HECTOR_AMD_EXTENDED_CONS, as the `ext`
    flavour).  The pair kernel has two instantiations, without and with the constraint code (which
    carries the per-member rows), and they need not round alike: one scenario-wide CO2 constraint,
    the same in both cores, puts both on the second."""
    fl = dict(FLAVOURS[flavour], outs=["NPP"])
    monkeypatch.setenv("HECTOR_AMD_EXTENDED_CONS", "1")
    pair = fl["kernel"] == "pair"
    base = scenario_values(lib, **kw)
    vals, S = draws(base, n)
    h = n // 2
    for k in NAMES:
        vals[k][:h] = base[k]
    S[:h] = S[h:2 * h]   # (and the perturbed half runs the same sensitivities)
    a = forcing_core(lib, fl, vals, S, run=False, **kw)
    b = forcing_core(lib, fl, {}, S, switch=False, run=False, **kw)
    for c in (a, b):
        if pair:
            c.setvar_dated("CO2_constrain", [1750], [278.0], "ppmv CO2")
        c.run(RUN_TO)
    assert a.last_run_kernel() == b.last_run_kernel() == fl["kernel"]
    assert a.last_run_variant() == b.last_run_variant() == -1
    ga, gb = all_outputs(a, fl), all_outputs(b, fl)
    for v in ga:
        assert np.array_equal(ga[v][:, :h], gb[v][:, :h]), (flavour, v)
    assert not np.array_equal(ga["RF_tot"][:, h:], gb["RF_tot"][:, h:])
    assert np.array_equal(a.status(), b.status())


def test_members_with_the_scenarios_own_values_have_the_bits_of_a_shared_core(emul_lib, monkeypatch):
    own_values_identity(emul_lib, monkeypatch, "run", allow_emulation=True)


@pytest.mark.parametrize("sections", [("CH4", "OH", "ozone"), ("N2O",)], ids=["ch4", "n2o"])
def test_disabled_gas_component_keeps_the_values_and_uses_none(emul_lib, tmp_path, sections):
    """[CH4] or [N2O] enabled=0: the forcing component leaves CO2, CH4 and N2O out (the shared -1);
    per-member delta_* change no bit and getvar still returns them."""
    path = edited_pack(tmp_path / "off.hxs", None, None, [], [], scalars={(s, "enabled"): 0.0 for s in sections})
    base = scenario_values(emul_lib, allow_emulation=True)
    vals, S = draws(base, 4, names=NAMES[:3])
    outs = OUTS
    cores = []
    for v in (vals, {}):
        c = hector_amd.Core(path, 4, lib_path=emul_lib, allow_emulation=True).enable_member_forcing()
        for k, x in v.items():
            c.setvar(k, x, UNITS[k])
        c.setvar("S", S, "degC").set_outputs(outs)
        c.run(RUN_TO)
        cores.append(c)
    a, b = cores
    for k in NAMES[:3]:
        assert np.array_equal(a.getvar(k), vals[k]), k
    assert a.last_run_variant() == b.last_run_variant() == 0   # (no efficacy rows: the plain kernel)
    for v in outs:
        assert np.array_equal(a.fetchvars(v, (Y0, RUN_TO)), b.fetchvars(v, (Y0, RUN_TO))), v


def test_rho_per_member_together_with_an_aerosol_mix(emul_lib, tmp_path):
    n = 6
    base = scenario_values(emul_lib, allow_emulation=True)
    vals, S = draws(base, n, names=NAMES[3:])
    rng = np.random.default_rng(7)
    scale, aero = 0.6 + 0.8 * rng.uniform(size=n), 0.5 + rng.uniform(size=n)
    c = hector_amd.Core(SCENARIO, n, lib_path=emul_lib, allow_emulation=True)
    c.enable_member_forcing().enable_slcf_mixes()
    years = np.arange(Y0, 2301)
    so2 = c.fetchvars("SO2_emissions", (Y0, 2300))[:, 0].copy()
    c.setvar_dated_mix("SO2_emissions", years, so2[None, :], scale[None, :], "Gg S")
    for k, v in vals.items():
        c.setvar(k, v, UNITS[k])
    c.setvar("S", S, "degC").setvar("aero_scalar", aero, "(unitless)")
    c.set_outputs(OUTS + RFS[:3])
    c.run(RUN_TO)
    assert c.last_run_kernel() == "run" and (c.status() == 0).all()
    # RF_SO2 = aero_scalar * rho_so2[m] * E[m], relative to the base year (1746), in the host's order
    E = scale[None, :] * so2[:RUN_TO - Y0 + 1, None]
    term = aero[None, :] * (vals["rho_so2"][None, :] * E)
    want = term - term[1]
    want[0] = 0.0
    assert np.array_equal(c.fetchvars("RF_SO2", (Y0, RUN_TO)), want)
    import oracle_binding
    nk = RUN_TO - Y0 + 1
    got = {v: c.fetchvars(v, (Y0, RUN_TO)) for v in ["CO2_concentration"] + list(TOL)}
    ts = c.fetchvars("timesteps", (Y0 + 1, RUN_TO))
    for i in range(n):
        path = edited_pack(tmp_path / ("mix%d.hxs" % i), "so2", "SO2_emissions", years, scale[i] * so2,
                           scalars={("forcing", k): v[i] for k, v in vals.items()})
        o = oracle_binding.Oracle(path)
        p = o.default_params(); p.S = S[i]; p.aero_scalar = aero[i]
        r, err, _ = o.run(p, run_to=RUN_TO)
        assert err == 0
        ref = r["CO2_concentration"][:nk]
        assert np.abs(got["CO2_concentration"][:, i] - ref).max() / ref.max() < 2e-8, i
        for v, tol in TOL.items():
            assert np.abs(got[v][:, i] - r[v][:nk]).max() < tol, (i, v)
        assert np.array_equal(ts[:, i], r["timesteps"][1:nk]), i


def test_segments_and_reset_are_bitwise_the_one_piece_run(emul_lib):
    fl = FLAVOURS["run"]
    vals, S = draws(scenario_values(emul_lib, allow_emulation=True), 8)
    one = all_outputs(forcing_core(emul_lib, fl, vals, S, allow_emulation=True), fl)
    c = forcing_core(emul_lib, fl, vals, S, run=False, allow_emulation=True)
    c.run(1900)
    c.run(RUN_TO)
    seg = all_outputs(c, fl)
    for v in one:
        assert np.array_equal(seg[v], one[v]), ("segments", v)
    c.reset()
    c.run(RUN_TO)
    again = all_outputs(c, fl)
    for v in one:
        assert np.array_equal(again[v], one[v]), ("reset", v)


def test_back_to_shared_equals_a_fresh_core(emul_lib):
    fl = FLAVOURS["run"]
    base = scenario_values(emul_lib, allow_emulation=True)
    vals, S = draws(base, 8)
    c = forcing_core(emul_lib, fl, vals, S, allow_emulation=True)
    assert c.last_run_variant() in (-1, 1)
    for k in NAMES:
        c.setvar(k, base[k], UNITS[k])
    c.run(RUN_TO)
    assert c.last_run_variant() == 0   # (the HXM_RF_AERO row and the efficacy rows are gone: the plain kernel)
    f = forcing_core(emul_lib, fl, {}, S, switch=False, allow_emulation=True)
    assert f.last_run_variant() == 0
    for v in OUTS + RFS:
        assert np.abs(c.fetchvars(v, (Y0, RUN_TO)) - f.fetchvars(v, (Y0, RUN_TO))).max() < 1e-9, v
