"""Every output and diagnostic against the oracle on every kernel flavour: the shared part of
tests/test_outputs_matrix.py (host build) and tests/test_gpu_outputs_matrix.py (device).

The year-loop kernels are separate instantiations of one source (hx_kernels.hip: one to four
biomes, the unrolled five to eight, the looped ones, the two-wavefront flavour, the extended kernel
with and without the NBP machinery, the plain kernel + diagnostics, carbon tracking, the
small-ensemble pair kernel).  Each records some sixty rows besides CO2 and tas; a row recorded from
the wrong register, a per-biome weight dropped, a diagnostic not cleared at the start of a year
shows in none of the rows the other suites compare.  A case here is (flavour, condition): one core
with every row of a set requested, compared row by row with the oracle given the same members and
the same constraint, checked for identities among its own rows, and replayed in segments, from a
reset and after a parameter change, bit for bit.

The output sets are imported by tools/soak/soak.py too."""
import os
import tempfile

import numpy as np

import hector_amd
from conftest import SCENARIO, edited_pack
from test_diagnostics import DERIVED_VARS, HOST_VARS, KERNEL_VARS, ORACLE_NAME
from test_one_factor import FLAVOURS, TRACK_DATE
from test_random_sweep import check_member

Y0, Y1 = 1745, 2300   # compared: 1746-2300

# ---------------------------------------------------------------------------------- output sets
_MORE = ["veg_c", "detritus_c", "soil_c", "permafrost_c", "thawedp_c", "earth_c", "atmos_co2", "ocean_c",
         "NBP", "ocean_uptake", "RF_tot", "RF_CO2", "land_tas", "sst", "CO2_concentration", "global_tas",
         "timesteps", "solver_steps"]
ALL = KERNEL_VARS + DERIVED_VARS + HOST_VARS + [v for v in _MORE if v not in KERNEL_VARS]
# the eleven rows per biome of the output stream (tests/test_biomes_ini.py); the oracle returns
# them for biomes 0-3
PER_BIOME = ["veg_c", "detritus_c", "soil_c", "permafrost_c", "thawedp_c", "NPP", "RH", "rh_ch4", "f_frozen",
             "detritus_tempfert", "soil_tempfert"]
BIOME_SUMS = ["veg_c", "detritus_c", "soil_c", "permafrost_c", "thawedp_c", "NPP", "RH"]   # global = sum over biomes
# what hx_pair_kernel records itself: the names behind ok[] in EnsembleCore::run (any other row
# requested moves the run to the run kernel, which last_run_kernel() == "pair" then shows)
PAIR = ["sst", "land_tas", "CO2_concentration", "global_tas", "timesteps", "RF_tot", "RF_CO2", "atmos_co2",
        "ocean_c", "ocean_uptake", "HL_pH", "LL_pH", "CH4_concentration", "O3_concentration", "NBP", "veg_c",
        "detritus_c", "soil_c", "permafrost_c", "thawedp_c", "earth_c", "heatflux", "NPP", "RH", "rh_det",
        "rh_soil", "rh_ch4", "f_frozen", "gmst"]
# ... of which a split core sends these to the run kernels
PAIR_NOT_SPLIT = ["NPP", "RH", "rh_det", "rh_soil", "heatflux"]
RF_PARTS = ["RF_CO2", "RF_N2O", "RF_CH4", "RF_H2O_strat", "RF_O3_trop", "RF_BC", "RF_OC", "RF_SO2", "RF_NH3",
            "RF_aci", "RF_vol", "RF_albedo", "RF_misc"]
INTEGER_ROWS = ["timesteps", "solver_steps", "ocean_timesteps"]   # equal, not close


def biome_rows(B, nb=None):
    return ["b%d.%s" % (b, v) for b in range(min(B, 4) if nb is None else nb) for v in PER_BIOME]


def output_set(flavour, which):
    """The rows a case requests: (rows compared with the oracle, rows requested besides)."""
    B = FLAVOURS[flavour]["B"]
    if which == "PAIR":
        return [v for v in PAIR if B == 1 or v not in PAIR_NOT_SPLIT], []
    if B == 1:
        return list(ALL), []
    # the identities need the summed rows of every biome, the oracle knows the first four
    return ALL + biome_rows(B), ["b%d.%s" % (b, v) for b in range(4, B) for v in BIOME_SUMS]


# ---------------------------------------------------------------------------------- tolerances
TOL = 2e-8   # the project's: tests/test_diagnostics.py, tests/test_gpu_parity.py
# Rows allowed more ON THE DEVICE, where each instantiation contracts its own multiply-adds: only the
# air-sea fluxes and NBP (small differences of large pools; tests/test_diagnostics_only_kernel.py:FLUX
# allows them 50 x between two instantiations), only with the oracle's stash schedule (asserted for
# every member compared), at most 4 x the measured worst and never more than 50 x.
# (case id, row) -> factor                       # measured worst, case
WIDER = {
    # none needed.  Measured on an MI355X over all 38 cases: the worst rows of members the oracle pins are
    # ocean_uptake 1.97e-8 (run-diff), HL_ocean_uptake 1.84e-8 (run2-ftot), LL_ocean_uptake 1.56e-8 (run-diff),
    # NBP 1.2e-9 (run2-ftot); the host build has the same members at 1.98e-8 / 1.94e-8 / 1.46e-8, so these
    # are the oracle's conditioning (check_member's noise test takes those past 2e-8), not the contraction
}
FLUX_ROWS = ("HL_ocean_uptake", "LL_ocean_uptake", "ocean_uptake", "NBP")
assert all(v in FLUX_ROWS and 1.0 < f <= 50.0 for (_, v), f in WIDER.items())


def tol(case_id, v, device):
    return TOL * (WIDER.get((case_id, v), 1.0) if device else 1.0)


# ---------------------------------------------------------------------------------- vacuous rows
# Reference rows without any spread over the years and members compared, per condition: a
# comparison of such a row says nothing.  Asserted both ways (assert_spread).
#  RF_misc: no such forcing in SSP2-4.5.  atmos_c_residual: zero unless a CO2 constraint is active
#  (hector_oracle.c, the residual of the constrained atmosphere).
VACUOUS = {
    None: {"RF_misc", "atmos_c_residual"},
    "diff": {"RF_misc", "atmos_c_residual"},
    "co2": {"RF_misc"},
    "tas": {"RF_misc", "atmos_c_residual"},
    "ftot": {"RF_misc", "atmos_c_residual"},
    "ch4": {"RF_misc", "atmos_c_residual"},
    "nbp": {"RF_misc", "atmos_c_residual"},
    "lo": {"RF_misc", "atmos_c_residual"},
}

# ---------------------------------------------------------------------------------- identities
# ocean_uptake = HL_ocean_uptake + LL_ocean_uptake and ocean_c = the four boxes, relative to the
# row's largest value: twice what the oracle's own rows satisfy them to (test_outputs_matrix.py::
# test_oracle_rows_satisfy_the_identities measures and asserts the oracle's half:
#  uptake 2.07e-16, ocean_c 3.83e-16 -- two ulps of 38 000 Pg C)
UPTAKE_SUM_TOL = 2 * 2.1e-16
OCEAN_C_SUM_TOL = 2 * 3.9e-16


# ---------------------------------------------------------------------------------- the ensemble
RANGES = {"S": (2.0, 5.0), "q10_rh": (1.3, 2.6), "beta": (0.3, 0.7), "aero_scalar": (0.5, 1.5),
          "vol_scalar": (0.6, 1.4)}
UNITS = {"S": "degC", "diff": "cm2/s"}
DEFAULT = {"S": 3.0, "q10_rh": 1.2, "beta": 0.65, "aero_scalar": 1.0, "vol_scalar": 1.0, "diff": 1.042}   # the INI's
DIFF_RANGE = (0.8, 2.8)
# (the reference's own mass-balance check, simpleNbox.hpp:37, fails a member that has to meet the NBP
# ramp with little CO2 fertilisation or much warming -- 31 of 128 members of the full ranges, in the
# 2040s; the oracle fails them likewise and the kernels flag them: such members are no parity case)
NBP_RANGES = {"S": (2.0, 3.2), "beta": (0.55, 0.7)}
PER_BIOME_PARAMS = ("q10_rh", "beta")
Q10_STEP, BETA_STEP = 0.05, 0.02          # biome b: + b x this (no two biomes alike)
WF0, WF_STEP = 0.85, 0.08                 # biome b's warming factor
# probe members as tests/test_gpu_one_factor.py places them: the INI default, a low and a high
# member, each twice, never member 0 -- which holds every range's lower end and so sorts to lane 0
PROBES = {"default": (5, 70), "low": (40, 101), "high": (20, 90)}
PROBE_AT = {"low": 0.1, "high": 0.9}


def probes(n):
    """{member: kind} for an ensemble of n; a ragged ensemble's last member is a probe."""
    out = {i: kind for kind, at in PROBES.items() for i in at if i < n}
    if n > 6 and n % 64:
        out[n - 1] = "high"
    if n <= 6:   # host tier
        out = {1: "default", 2: "low", 3: "high"}
    return out


def members(n, cond=None, seed=20261):
    """{parameter: values[n]}: S, q10_rh, beta, aero_scalar and vol_scalar varied together (seeded),
    plus diff or lo_warming_ratio where the condition is about them."""
    rng = np.random.default_rng(seed)
    ranges = dict(RANGES, **({"diff": DIFF_RANGE} if cond == "diff" else NBP_RANGES if cond == "nbp" else {}))
    v = {}
    for k, (lo, hi) in ranges.items():
        x = rng.uniform(lo, hi, n)
        x[0] = lo
        for i, kind in probes(n).items():
            x[i] = DEFAULT[k] if kind == "default" else lo + PROBE_AT[kind] * (hi - lo)
        v[k] = x
    if cond == "lo":
        v["lo_warming_ratio"] = np.where(np.arange(n) % 2, 1.5, 0.0)
    return v


def biome_value(k, x, b):
    return x + b * (Q10_STEP if k == "q10_rh" else BETA_STEP)


def set_members(c, v, B):
    for k, x in v.items():
        if k in PER_BIOME_PARAMS and B > 1:
            for b in range(B):
                c.setvar("b%d.%s" % (b, k), biome_value(k, x, b))
        else:
            c.setvar(k, x, UNITS.get(k))
    if B > 1:
        for b in range(B):
            c.setvar("b%d.warmingfactor" % b, np.full(len(v["S"]), WF0 + WF_STEP * b))


def oracle_member(o, v, i, B):
    p = o.default_params()
    if B > 1:
        p = o.split_equal(p, B)
    p.nbiome = B
    for k, x in v.items():
        if k in PER_BIOME_PARAMS:
            for b in range(B):
                getattr(p, k)[b] = biome_value(k, x[i], b) if B > 1 else x[i]
        else:
            setattr(p, k, x[i])
    if B > 1:
        for b in range(B):
            p.warmingfactor[b] = WF0 + WF_STEP * b
    return p


# ---------------------------------------------------------------------------------- conditions
_TMP = None
_ORACLES = {}
_REFS = {}


def default_run():
    """The default member's unconstrained run by the oracle (what the CO2 and CH4 constraints scale)."""
    return oracle_for(None).run()[0]


def constraint(cond):
    """-> None or (capability, unit, pack section, years, values, years and values for the pack)"""
    if cond == "co2":     # 1.05 x the default member's own trajectory over the historical period
        y = np.arange(1850, 2015)
        x = 1.05 * default_run()["CO2_concentration"][y - Y0]
        return "CO2_constrain", "ppmv CO2", "simpleNbox", y, x, y, x
    if cond == "tas":     # warmer than any member gets by 2000
        y = np.arange(1900, 2001)
        x = np.linspace(0.3, 2.2, y.size)
        return "tas_constrain", "degC", "temperature", y, x, y, x
    if cond == "ftot":    # (used for every date up to its last one, flat before its first:
        y = np.arange(1950, 2051)   # forcing_component.cpp:498-505; the pack spells that out)
        x = np.linspace(0.8, 5.0, y.size)
        return ("RF_tot_constrain", "W/m2", "forcing", y, x, np.arange(Y0, 2051),
                np.concatenate([np.full(1950 - Y0, x[0]), x]))
    if cond == "ch4":     # 1.5 x the default run's concentrations, the preindustrial one included
        y = np.arange(Y0, Y1 + 1)
        x = 1.5 * default_run()["CH4_concentration"]
        return "CH4_constrain", "ppbv CH4", "CH4", y, x, y, x
    if cond == "nbp":
        y = np.arange(1950, 2051)
        x = 0.5 + 0.01 * (y - 1950)
        return "NBP_constrain", "Pg C/yr", "simpleNbox", y, x, y, x
    return None


def oracle_for(cond):
    """The oracle reading the packaged scenario, or a copy that carries the condition's constraint."""
    global _TMP
    key = cond if constraint(cond) is not None else None
    if key not in _ORACLES:
        import oracle_binding
        path = SCENARIO
        if key is not None:
            if _TMP is None:
                _TMP = tempfile.TemporaryDirectory(prefix="outputs_matrix_")
            cap, _, section, _, _, py, px = constraint(cond)
            path = edited_pack(os.path.join(_TMP.name, cond + ".hxs"), section, cap, py, px)
        _ORACLES[key] = oracle_binding.Oracle(path)
    return _ORACLES[key]


def reference(cond, v, i, B):
    """(params, rows, err) of member i by the oracle; cached by (pack, parameters) -- the flavours of
    one biome count share their members, the probes come in pairs."""
    o = oracle_for(cond)
    key = (cond if constraint(cond) is not None else None, B) + tuple(float(v[k][i]) for k in sorted(v))
    if key not in _REFS:
        p = oracle_member(o, v, i, B)
        r, err, _ = o.run(p)
        _REFS[key] = (p, r, err)
    return _REFS[key]


# ---------------------------------------------------------------------------------- cases
def case(flavour, cond=None, which="ALL", kernel=None, variant=None, env=None, n=None):
    fl = FLAVOURS[flavour]
    if variant is None:
        if cond == "nbp":
            variant = 1
        elif fl.get("track"):
            variant = 2
        elif env or cond not in (None, "diff") or fl["B"] > 4:
            variant = -1    # the extended kernel proper
        else:
            variant = -2    # the plain kernel + diagnostics
    cid = "-".join([flavour] + ([cond] if cond else []) + (["cons"] if env else []) + (["n%d" % n] if n else []))
    return dict(id=cid, flavour=flavour, cond=cond, which=which, kernel=kernel or fl["kernel"], variant=variant,
                env=env or {}, n=n)


CONS = {"HECTOR_AMD_EXTENDED_CONS": "1"}
UNCONSTRAINED = [case("run"), case("ext", env=CONS), case("run2"), case("run2", env=CONS),
                 case("pair", which="PAIR"), case("b4pair", which="PAIR"),
                 case("b2"), case("b4"), case("b6"), case("b9"), case("trk")]
# per-member ocean diffusivity: the per-member DOECLIM kernel table, the heat-flux rows
PER_MEMBER_DIFF = [case("run", "diff"), case("run2", "diff"), case("pair", "diff", which="PAIR"), case("b4", "diff")]
CONSTRAINED = ([case(f, "co2", which="PAIR" if f == "pair" else "ALL") for f in ("run", "run2", "pair", "b4")] +
               [case(f, "tas", which="PAIR" if f == "pair" else "ALL") for f in ("run", "run2", "pair", "b2")] +
               [case(f, "ftot") for f in ("run", "run2", "b6")] +
               [case(f, "ch4", which="PAIR" if f == "pair" else "ALL") for f in ("run", "pair", "b2")] +
               [case(f, "nbp") for f in ("run", "run2", "b2")] +
               # what the pair kernel does not serve falls back to the run kernel (EnsembleCore::run)
               [case("pair", "nbp", which="PAIR", kernel="run")])
LO_RATIO = [case("run", "lo"), case("run2", "lo"), case("b4", "lo")]
RAGGED = [case("run", n=65)]
CASES = UNCONSTRAINED + PER_MEMBER_DIFF + CONSTRAINED + LO_RATIO
HOST_CASES = [c for c in CASES if FLAVOURS[c["flavour"]]["kernel"] != "pair"]   # (no pair kernel: no MFMA)
GPU_REPLAY = [case("run"), case("run2"), case("pair", which="PAIR"), case("b4"), case("b9"), case("run2", "co2")]
assert len({c["id"] for c in CASES + RAGGED}) == len(CASES + RAGGED)


def build_core(lib, cs, v, history=False, **kw):
    """A core of case `cs` holding members `v`, its rows requested, not yet run.
    -> (core, rows compared, every row requested)"""
    fl = FLAVOURS[cs["flavour"]]
    B = fl["B"]
    c = hector_amd.Core(SCENARIO, len(v["S"]), lib_path=lib, **kw)
    if B > 1:
        c.split_biome(["b%d" % b for b in range(B)])
    c.set_pair_kernel_limit(fl["pair"]).set_two_wave_from(fl["w2"])
    if fl.get("track"):
        c.setvar("trackingDate", [TRACK_DATE])
    if history:
        c.enable_history(True)
    set_members(c, v, B)
    con = constraint(cs["cond"])
    if con:
        c.setvar_dated(con[0], con[3], con[4], con[1])
    compared, more = output_set(cs["flavour"], cs["which"])
    c.set_outputs(compared + more)
    return c, compared, compared + more


def assert_case_kernel(c, cs):
    assert c.last_run_kernel() == cs["kernel"], (cs["id"], c.last_run_kernel())
    assert c.last_run_variant() == cs["variant"], (cs["id"], c.last_run_variant())
    assert len(c.biomes()) == FLAVOURS[cs["flavour"]]["B"]


def fetch(c, rows, y1=Y1):
    return {v: c.fetchvars(v, (Y0 + 1, y1)) for v in rows}


def assert_lanes(c, n):
    """No probe in lane 0, probes in both wavefronts."""
    lanes = c.lane_of_member()
    ps = probes(n)
    assert all(lanes[i] != 0 for i in ps), lanes[list(ps)]
    assert {int(lanes[i]) // 64 for i in ps} == {0, 1}, lanes[list(ps)]


# ---------------------------------------------------------------------------------- the checks
WORST = {}   # (case id, row) -> worst deviation / max(1, max|ref|): test_zz_report prints it
ILL = []     # (case id, member, row, deviation) that check_member's noise test let pass


def oracle_row(r, v):
    return r[ORACLE_NAME.get(v, v)][1:]


def assert_vs_oracle(c, cs, v, got, compared, who, device):
    """Members `who` of the case's core against the oracle, every compared row; then the vacuous-row
    table both ways.  -> the ill-conditioned members met (check_member's escape)."""
    cid, B = cs["id"], FLAVOURS[cs["flavour"]]["B"]
    st = c.status()
    ill, refs = [], {}
    for i in who:
        p, r, err = reference(cs["cond"], v, i, B)
        assert err == 0 and st[i] == 0, (cid, i, err, st[i])
        refs[i] = r
        dev = {}
        for row in compared:
            ref, x = oracle_row(r, row), got[row][:, i]
            if row in INTEGER_ROWS:   # (the stash schedule first: what the wider flux tolerances rest on)
                assert np.array_equal(x, ref), (cid, row, i)
                continue
            d = np.abs(x - ref).max() / max(1.0, np.abs(ref).max())
            dev[ORACLE_NAME.get(row, row)] = d
        tols = {ORACLE_NAME.get(row, row): tol(cid, row, device) for row in compared}
        check_member(oracle_for(cs["cond"]), p, dev, tols, (cid, i), ill)
        for row, d in dev.items():   # (an ill-conditioned member's rows over the tolerance: reported apart)
            if d < tols[row]:
                WORST[(cid, row)] = max(WORST.get((cid, row), 0.0), d)
            else:
                ILL.append((cid, i, row, d))
    assert_spread(cs, compared, refs)
    return ill


def assert_spread(cs, compared, refs):
    """Every compared reference row varies over the years and members compared, except the rows
    VACUOUS lists for the condition -- and those do not."""
    flat = set()
    for row in compared:
        x = np.stack([oracle_row(r, row) for r in refs.values()])
        if x.max() == x.min():
            flat.add(row)
    listed = VACUOUS[cs["cond"]] & set(compared)
    assert flat == listed, (cs["id"], "rows without spread", sorted(flat), "listed", sorted(listed))


def assert_identities(c, cs, got, requested):
    """Identities among the kernel's own rows (every member)."""
    cid, B = cs["id"], FLAVOURS[cs["flavour"]]["B"]
    if all(v in got for v in RF_PARTS + ["RF_tot"]):
        # the reference's RF_tot is the sum of its parts (forcing_component.cpp:489-492) -- under an
        # RF_tot constraint after its last date only, and then shifted by the base year's difference
        # between the constraint and the parts (forcing_component.cpp:498-505, 515-530)
        total = sum(got[v] for v in RF_PARTS) + sum(c.fetchvars("RF_" + h, (Y0 + 1, Y1)) for h in sorted(c.halocarbons()))
        yr = np.arange(Y0 + 1, Y1 + 1)
        free = yr > 2050 if cs["cond"] == "ftot" else yr > 0
        d = (total - got["RF_tot"])[free]
        assert np.abs(d - (d[0] if cs["cond"] == "ftot" else 0.0)).max() < 1e-12, (cid, "RF_tot")
    if B > 1 and cs["which"] != "PAIR":
        for v in BIOME_SUMS:
            parts = sum(c.fetchvars("b%d.%s" % (b, v), (Y0 + 1, Y1)) for b in range(B))
            assert np.allclose(parts, got[v], rtol=1e-13, atol=0.0), (cid, v, np.abs(parts - got[v]).max())
    if "HL_ocean_uptake" in got:
        s = got["HL_ocean_uptake"] + got["LL_ocean_uptake"]
        assert np.abs(s - got["ocean_uptake"]).max() <= UPTAKE_SUM_TOL * np.abs(got["ocean_uptake"]).max(), (cid, "uptake")
        s = got["HL_ocean_c"] + got["LL_ocean_c"] + got["IO_ocean_c"] + got["DO_ocean_c"]
        assert np.abs(s - got["ocean_c"]).max() <= OCEAN_C_SUM_TOL * np.abs(got["ocean_c"]).max(), \
            (cid, "ocean_c", np.abs(s - got["ocean_c"]).max())
    if cs["cond"] == "nbp":   # NBP is the constraint in its years (tests/test_constraints.py)
        _, _, _, y, x, _, _ = constraint("nbp")
        assert np.abs(got["NBP"][y - Y0 - 1] - x[:, None]).max() < 1e-10, cid
    if cs["cond"] == "lo" and "ocean_tas" in got:
        # temperature_component.cpp:722-739: land and sea follow global tas at the member's ratio
        lo = np.where(np.arange(got["sst"].shape[1]) % 2, 1.5, 0.0)
        on = lo != 0
        assert np.allclose(got["land_tas"][100:, on] / got["ocean_tas"][100:, on], lo[on], rtol=1e-12), cid


def run_case(lib, cs, n, on_device, **kw):
    """One case: the core run in one launch, held to the oracle and to its identities.
    -> (core, members, rows compared, rows requested, what it recorded)"""
    v = members(n, cs["cond"])
    c, compared, requested = build_core(lib, cs, v, **kw)
    c.run(Y1)
    assert_case_kernel(c, cs)
    assert (c.status() == 0).all(), cs["id"]
    got = fetch(c, compared)
    B = FLAVOURS[cs["flavour"]]["B"]
    # one biome: every member; several: the probes (the host tier's few members: all of them)
    who = range(n) if B == 1 or n <= 6 else sorted(probes(n))
    ill = assert_vs_oracle(c, cs, v, got, compared, who, on_device)
    assert_identities(c, cs, got, requested)
    if ill:
        print("ill-conditioned members:", ill)
    return c, v, compared, requested, got


SEGMENTS = (1750, 1751, 1800, 1983, 2100, 2300)


SLR_ROWS = ("slr", "sl_rc", "slr_no_ice", "sl_rc_no_ice")


def assert_same(a, b, rows, y1, what, who=slice(None)):
    for v in rows:
        x, y = a.fetchvars(v, (Y0, y1))[:, who], b.fetchvars(v, (Y0, y1))[:, who]
        if v in SLR_ROWS and y1 < 1980:
            # slr_component.cpp:116-232: no sea level before its reference period 1951-1980 has run
            assert not x.any(), (what, v, y1)
            continue
        assert np.array_equal(x, y, equal_nan=True), (what, v, y1, np.nanmax(np.abs(x - y)))


def replay_case(lib, cs, n, one=None, **kw):
    """A second core with its history kept, run in segments, from two resets and after a parameter
    change: every requested row (the device-derived ones and their caches included) bit for bit the
    one-launch core's -- one instantiation against itself."""
    v = members(n, cs["cond"])
    if one is None:
        one, _, _ = build_core(lib, cs, v, **kw)
        one.run(Y1)
    b, _, rows = build_core(lib, cs, v, history=True, **kw)
    for y in SEGMENTS:
        b.run(y)
        assert_case_kernel(b, cs)
        assert_same(b, one, rows, y, (cs["id"], "segment"))
    for date in (2050, 1746):
        b.reset(date)
        b.run(Y1)
        assert_case_kernel(b, cs)
        assert_same(b, one, rows, Y1, (cs["id"], "reset", date))
    rev = dict(v, S=v["S"][::-1].copy())
    b.setvar("S", rev["S"], "degC")
    b.run(Y1)
    assert_case_kernel(b, cs)
    fresh, _, _ = build_core(lib, cs, rev, **kw)
    fresh.run(Y1)
    # (a member the model fails with its new S -- an NBP constraint it cannot meet -- fails in both
    # cores and in the oracle; what its rows hold past the failure is not defined)
    st = fresh.status()
    assert np.array_equal(b.status(), st), (cs["id"], st, b.status())
    for i in np.nonzero(st)[0]:
        assert reference(cs["cond"], rev, i, FLAVOURS[cs["flavour"]]["B"])[2] != 0, (cs["id"], i, st[i])
    assert (st == 0).sum() >= len(st) - 1
    assert_same(b, fresh, rows, Y1, (cs["id"], "S reversed"), who=st == 0)
    x, y = b.fetchvars("global_tas", (Y0, Y1)), one.fetchvars("global_tas", (Y0, Y1))
    assert not np.array_equal(x, y), (cs["id"], "the parameter change moved nothing")
    return one, b, fresh


def report_lines():
    """Worst deviation per row over the cases run, with the case that holds it."""
    by_row = {}
    for (cid, row), d in WORST.items():
        if d >= by_row.get(row, (-1.0, ""))[0]:
            by_row[row] = (d, cid)
    return (["%-22s %.2e  %s" % (row, d, cid) for row, (d, cid) in sorted(by_row.items(), key=lambda kv: -kv[1][0])] +
            ["ill-conditioned (oracle's own answer moves under rounding noise): %s member %d %s %.2e" % x for x in ILL])
