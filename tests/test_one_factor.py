"""One parameter varied alone, on every kernel flavour of the host build (tests/emul).

The year-loop kernels read a parameter row from the uniform table (member 0's value, scalar loads)
when every member shares it, else from the member's own row: EnsembleCore::buffers() turns
row_uniform_ into per-group flags (uni_k, uni_avc, uni_wf, uni_bio, uni_landk, ker_per_member), and
the spinup column of kParams decides whether one prototype spins up for every lane.  A row read
under a flag that does not cover it, or a spinup column that is wrong, hands every member lane 0's
value silently -- and only in the mixed case: one group varying while the others stay uniform.

The host build has no FMA contraction, so the two reads must agree bit for bit: member k of an
ensemble in which only this parameter varies equals member 0 of an ensemble in which every member
holds member k's value.  A few members are checked against the oracle besides.
(tests/test_gpu_one_factor.py: the same matrix on the device, against the oracle.)"""
import numpy as np
import pytest

import hector_amd
from conftest import SCENARIO
from test_random_sweep import check_member

# capability: (low, high, unit, per_biome, spinup) -- low/high after test_random_sweep.RANGES, the
# rows it lacks added.  `spinup`: the spinup sees the parameter (the kParams column; the spinup
# zeroes the emissions and holds co2fert, tempfert and f_frozen at 1, simpleNbox-runtime.cpp:952-1000,
# simpleNbox.cpp:733,802).
PARAMS = {
    "S": (1.5, 6.0, "degC", False, False),
    "diff": (0.6, 3.0, "cm2/s", False, False),
    "qco2": (3.0, 4.5, "W/m2", False, False),
    "aero_scalar": (0.3, 1.7, None, False, False),
    "vol_scalar": (0.5, 1.5, None, False, False),
    "C0": (265.0, 290.0, "ppmv CO2", False, True),
    "tt": (5.5e7, 9e7, "m3/s", False, True),
    "tu": (4e7, 6e7, "m3/s", False, True),
    "twi": (1e7, 1.6e7, "m3/s", False, True),
    "tid": (1.5e8, 2.5e8, "m3/s", False, True),
    "preind_surface_c": (750.0, 1050.0, "Pg C", False, True),
    "preind_interdeep_c": (32000.0, 42000.0, "Pg C", False, True),
    "lo_warming_ratio": (1.2, 1.8, None, False, False),
    "beta": (0.2, 0.9, None, True, False),
    "q10_rh": (1.1, 3.0, None, True, False),
    "warmingfactor": (0.8, 1.6, None, True, False),
    "npp_flux0": (45.0, 64.0, "Pg C/yr", True, True),   # (65.0: a tie in the reference's own alkalinity
                                                        # tuner, its trajectory moves 5e-5 K under 1e-13 noise)
    "veg_c": (400.0, 700.0, "Pg C", True, True),
    "detritus_c": (40.0, 70.0, "Pg C", True, True),
    "soil_c": (700.0, 1100.0, "Pg C", True, True),
    "permafrost_c": (600.0, 1100.0, "Pg C", True, True),
    "f_nppv": (0.3, 0.4, None, True, True),
    "f_nppd": (0.5, 0.6, None, True, True),
    "f_litterd": (0.9, 1.0, None, True, True),
    "rh_ch4_frac": (0.01, 0.04, None, True, False),
    "pf_mu": (1.4, 1.9, "degC", True, False),
    "pf_sigma": (0.8, 1.1, "degC", True, False),
    "fpf_static": (0.6, 0.85, None, True, False),
}
# values at the edges check_parameters() accepts (the other rows of the biome at their defaults:
# f_nppv 0.35 + f_nppd 0.65 = 1), where the oracle runs cleanly
EDGES = {"beta": [0.0], "q10_rh": [1.0], "f_litterd": [1.0], "f_nppv": [0.4], "f_nppd": [0.65],
         "permafrost_c": [0.0], "fpf_static": [0.0, 1.0], "warmingfactor": [1.0]}
ORACLE_SCALARS = {"S", "diff", "qco2", "aero_scalar", "vol_scalar", "C0", "tt", "tu", "twi", "tid",
                  "preind_surface_c", "preind_interdeep_c", "lo_warming_ratio"}
LAND = [k for k, v in PARAMS.items() if v[3]]
TRACK_DATE = 1900

# kernel flavours: biome count, pair-kernel limit, two-wavefront threshold, what run() must report.
# 6 biomes: the unrolled 5-8 family; 9: the looped kernels (hx_looped_from(), hx_kernels.hip).  The
# varying per-biome row sits in the LAST biome (the looped kernels' second 8-column chunk at 9).
FLAVOURS = {
    "run": dict(B=1, pair=0, w2=0, kernel="run"),
    "run2": dict(B=1, pair=0, w2=1, kernel="run2"),
    "pair": dict(B=1, pair=32768, w2=0, kernel="pair"),
    "b2": dict(B=2, pair=0, w2=0, kernel="run"),
    "b4": dict(B=4, pair=0, w2=0, kernel="run"),
    "b4pair": dict(B=4, pair=32768, w2=0, kernel="pair"),
    "b6": dict(B=6, pair=0, w2=0, kernel="run"),
    "b9": dict(B=9, pair=0, w2=0, kernel="run"),
    # the extended kernel (diagnostic outputs; HECTOR_AMD_EXTENDED_CONS: not the plain-plus-
    # diagnostics instantiation) and carbon tracking, on a split core
    "ext": dict(B=2, pair=0, w2=0, kernel="run", variant=-1, outs=["NPP", "RH", "f_frozen"],
                env={"HECTOR_AMD_EXTENDED_CONS": "1"}),
    "trk": dict(B=2, pair=0, w2=0, kernel="run", variant=2, track=True),
}
HOST_FLAVOURS = ["run", "run2", "b2", "b4", "b6", "b9", "ext", "trk"]   # (no pair kernel: no MFMA)
OUTS = ["CO2_concentration", "global_tas", "timesteps", "RF_tot", "ocean_c", "sst", "veg_c", "soil_c",
        "permafrost_c", "NBP"]


def cases(flavours):
    """(flavour, parameter): every parameter on every flavour, the tracking and extended kernels
    for the land parameters."""
    return [(f, k) for f in flavours for k in PARAMS if k in LAND or f not in ("ext", "trk")]


def capability(name, B):
    return "b%d.%s" % (B - 1, name) if PARAMS[name][3] and B > 1 else name


def expected_variant(fl, values, name):
    if "variant" in fl:
        return fl["variant"]
    # a land-ocean warming ratio takes the extended kernel (with or without the NBP machinery)
    return (-1, 1) if name == "lo_warming_ratio" and np.any(np.asarray(values) != 0) else (0,)


def make_core(lib, fl, name, values, run_to, path=SCENARIO, **kw):
    """A core on flavour `fl` in which only `name` differs between members (given in the units
    of the unsplit core: pools and npp_flux0 are scaled by the biome's share, as split_biome does).
    Runs it to `run_to`."""
    n = len(values)
    c = hector_amd.Core(path, n, lib_path=lib, **kw)
    B = fl["B"]
    if B > 1:
        c.split_biome(["b%d" % b for b in range(B)])
    c.set_pair_kernel_limit(fl["pair"]).set_two_wave_from(fl["w2"])
    if fl.get("track"):
        c.setvar("trackingDate", [TRACK_DATE])
    c.setvar(capability(name, B), biome_values(name, values, B), PARAMS[name][2])
    c.set_outputs(OUTS + fl.get("outs", []))
    c.run(run_to)
    return c


def biome_values(name, values, B):
    scale = 1.0 / B if name in ("npp_flux0", "veg_c", "detritus_c", "soil_c", "permafrost_c") else 1.0
    return np.asarray(values, dtype=np.float64) * scale


def expected_kernel(fl, values, name):
    # what the pair kernel does not serve goes to the run kernel (EnsembleCore::run): a land-ocean
    # warming ratio; per-member diffusivity on a split core
    varies = np.any(np.asarray(values) != np.asarray(values)[0])
    if fl["kernel"] == "pair" and ((name == "lo_warming_ratio" and np.any(np.asarray(values) != 0)) or
                                   (name == "diff" and fl["B"] > 1 and varies)):
        return "run"
    return fl["kernel"]


def assert_flavour(c, fl, name, values):
    assert c.last_run_kernel() == expected_kernel(fl, values, name), (c.last_run_kernel(), fl, name)
    v = expected_variant(fl, values, name)
    assert c.last_run_variant() in (v if isinstance(v, tuple) else (v,)), (c.last_run_variant(), fl, name)
    assert len(c.biomes()) == fl["B"]


def host_values(name):
    """Member 0 at the INI default (what the uniform table holds); then low, high and an edge."""
    lo, hi = PARAMS[name][:2]
    return [DEFAULTS[name], lo, hi] + EDGES.get(name, [])[-1:]


DEFAULTS = {"S": 3.0, "diff": 1.042, "qco2": 3.75, "aero_scalar": 1.0, "vol_scalar": 1.0, "C0": 277.15,
            "tt": 7.2e7, "tu": 4.9e7, "twi": 1.25e7, "tid": 2e8, "preind_surface_c": 900.0,
            "preind_interdeep_c": 37100.0, "lo_warming_ratio": 0.0, "beta": 0.65, "q10_rh": 1.2,
            "warmingfactor": 1.0, "npp_flux0": 56.2, "veg_c": 550.0, "detritus_c": 55.0, "soil_c": 917.0,
            "permafrost_c": 865.0, "f_nppv": 0.35, "f_nppd": 0.6, "f_litterd": 0.98,
            "rh_ch4_frac": 0.023, "pf_mu": 1.67, "pf_sigma": 0.986, "fpf_static": 0.74}


def oracle_params(o, name, value, B):
    p = o.default_params()
    if B > 1:
        p = o.split_equal(p, B)
    if name in ORACLE_SCALARS:
        setattr(p, name, value)
    else:
        getattr(p, name)[B - 1] = biome_values(name, [value], B)[0]
    p.nbiome = B
    return p


_ORACLE = {}


def check_vs_oracle(o, c, i, name, value, B, run_to, where, ill):
    """Member i of core c against the oracle: CO2 2e-8 relative, Tgav 2e-8 K, the stash schedule,
    the spinup's step count (the test_random_sweep escape for ill-conditioned members only)."""
    key = (name, float(value), B, run_to)
    if key not in _ORACLE:   # (what the oracle gives depends on the parameter values alone)
        p = oracle_params(o, name, value, B)
        _ORACLE[key] = (p,) + tuple(o.run(p, run_to))
    p, r, err, steps = _ORACLE[key]
    assert err == 0 and c.status()[i] == 0, (where, err, c.status()[i])
    k = run_to - 1745 + 1
    co2 = c.fetchvars("CO2_concentration", (1745, run_to))[:, i]
    tg = c.fetchvars("global_tas", (1745, run_to))[:, i]
    dev = {"CO2_concentration": np.abs(co2 - r["CO2_concentration"][:k]).max() / np.abs(r["CO2_concentration"][:k]).max(),
           "global_tas": np.abs(tg - r["global_tas"][:k]).max()}
    check_member(o, p, dev, {"CO2_concentration": 2e-8, "global_tas": 2e-8}, where, ill)
    assert np.array_equal(c.fetchvars("timesteps", (1746, run_to))[:, i], r["timesteps"][1:k]), where
    assert c.spinup_steps(i) == steps, (where, c.spinup_steps(i), steps)
    return dev


def assert_member_is(c, i, ref, j, outs, run_to, where, track=False):
    """Member i of c bit for bit member j of ref: every recorded output, the spinup, the status."""
    for v in outs:
        a = c.fetchvars(v, (1745, run_to))[:, i]
        b = ref.fetchvars(v, (1745, run_to))[:, j]
        assert np.array_equal(a, b), (where, v, np.abs(a - b).max())
    assert c.spinup_steps(i) == ref.spinup_steps(j), where
    assert c.status()[i] == ref.status()[j], where
    if track:
        va, fa = c.tracking_data(i, (TRACK_DATE, run_to))
        vb, fb = ref.tracking_data(j, (TRACK_DATE, run_to))
        assert np.array_equal(va, vb) and np.array_equal(fa, fb), (where, "tracking")


RUN_TO = 2100   # (host: the warming this century is what moves the permafrost and CH4 rows)
_uniform_cache = {}


def uniform_core(lib, flavour, name, value):
    """Member 0 of an ensemble in which every member holds `value` (the row uniform)."""
    key = (flavour, name, float(value))
    if key not in _uniform_cache:
        _uniform_cache[key] = make_core(lib, FLAVOURS[flavour], name, [value], RUN_TO, allow_emulation=True)
    return _uniform_cache[key]


@pytest.mark.parametrize("flavour,name", cases(HOST_FLAVOURS), ids=["-".join(c) for c in cases(HOST_FLAVOURS)])
def test_one_parameter_varied_alone_is_bitwise_the_uniform_ensemble(emul_lib, oracle, monkeypatch, flavour, name):
    fl = FLAVOURS[flavour]
    for k, v in fl.get("env", {}).items():
        monkeypatch.setenv(k, v)
    vals = host_values(name)
    c = make_core(emul_lib, fl, name, vals, RUN_TO, allow_emulation=True)
    assert_flavour(c, fl, name, vals)
    outs = OUTS + fl.get("outs", [])
    for i, v in enumerate(vals):
        ref = uniform_core(emul_lib, flavour, name, v)
        assert_flavour(ref, fl, name, [v])
        assert_member_is(c, i, ref, 0, outs, RUN_TO, (flavour, name, i, v), track=fl.get("track", False))
    if flavour in ("run", "b4", "b9"):   # a few members against the oracle (one-biome ones: every one)
        ill = []
        for i in (range(len(vals)) if fl["B"] == 1 else (1, 2)):
            check_vs_oracle(oracle, c, i, name, vals[i], fl["B"], RUN_TO, (flavour, name, i), ill)
