"""The cases of test_stash_control_emulation.py, test_gpu_stash_control.py and
tools/make_stash_control_golden.py: the per-lane control of the stash and of the segment loop
around it (stash(), solve_year() in hx_dev_solver.h).

The 96 members of test_gpu_step_control.py (S 1.5-6 x Q10 1.2-4: one full wavefront and a half-
filled one) on the run kernel (`set_pair_kernel_limit(0)`), for SSP2-4.5 and SSP5-8.5, on the plain
kernel ("run"), the two-wave flavour ("run2") and four biomes ("run_b4": an equal split whose biomes
differ in Q10 and warming factor).  Each run is 555 years of 96 members.

Of those three kernels only the plain one-biome one takes the flat form (hx_flat_stash); the plain
two-wave and four-biome kernels keep the nested form.  Five further cases on SSP2-4.5 (EXTRA) put
the flat form of every other family into the same mixed wavefronts, and the flag cases run flat
instantiations with and without the NBP machinery (FLAG_VARIANT).

Not a test module: no test_ prefix."""
import hashlib
import os

import numpy as np

import hector_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = {"ssp245": os.path.join(ROOT, "hector_amd", "data", "ssp245.hxs"),
             "ssp585": os.path.join(ROOT, "hector_amd", "data", "ssp585.hxs")}
KERNELS = ("run", "run2", "run_b4")
# Which instantiation hx_run_kernel<B, HF, KERPM, CON> a case runs (EnsembleCore::run and
# launch_run_b: per-member diffusivity gives <.., true, true, ..>; else a heat-flux output or
# CON = 1 gives <.., true, false, ..>; a diagnostic such as NPP alone gives CON = -2; an NBP
# constraint CON = 1), with 101 for the two-wave flavour.  The first three are the issue's; of
# them only "run" is an instantiation of hx_flat_stash (hx_dev_solver.h) -- the plain two-wave
# and four-biome kernels keep the nested form -- so the further ones, SSP2-4.5 only, each put the
# flat form of another family into the same mixed wavefronts: two-wave, two / three / four biomes,
# the diagnostics kernel.  flat_stash() mirrors the header's list; the tests assert it for them.
VARIANT = {"run": (1, False, False, 0), "run2": (101, False, False, 0), "run_b4": (4, False, False, 0),
           "run2_diff_hf": (101, True, True, 0), "b2_diff": (2, True, True, 0),
           "b3_diff": (3, True, True, 0), "b4_npp": (4, False, False, -2), "b1_npp": (1, False, False, -2)}
EXTRA = ("run2_diff_hf", "b2_diff", "b3_diff", "b4_npp", "b1_npp")
CASES = [(s, k) for s in sorted(SCENARIOS) for k in KERNELS] + [("ssp245", k) for k in EXTRA]


def flat_stash(B, HF, KERPM, CON):
    """hx_flat_stash<B, HF, KERPM, CON>() of hx_dev_solver.h, line by line."""
    if not (CON < 2 and (1 <= B <= 4 or B == 101)):
        return False
    if B == 101:
        if CON in (-2, 1, -1):
            return HF and KERPM
        return HF
    if B == 1:
        return not (not KERPM and CON in (1, -1))
    if B == 2:
        return {-2: HF and KERPM, -1: not HF, 1: False, 0: KERPM}[CON]
    if B == 3:
        return {-1: HF, 0: KERPM}.get(CON, True)
    return {-2: not KERPM, -1: False, 1: HF and not KERPM, 0: False}[CON]


def n_biomes(kernel):
    return {"run_b4": 4, "b2_diff": 2, "b3_diff": 3, "b4_npp": 4}.get(kernel, 1)


def member_diff():
    """per-member ocean diffusivity (cm2/s), scattered over the members"""
    return 0.8 + 1.6 * ((np.arange(N) * 37) % N) / (N - 1.0)


OUTS = ["CO2_concentration", "global_tas", "sst", "land_tas", "timesteps"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "stash_control_parent.npz")
# the years whose values the golden holds as float64 (every output's whole series as a SHA-256)
GOLDEN_YEARS = (1850, 1950, 2000, 2050, 2100, 2150, 2200, 2300)
N = 96
REL_CO2 = 2e-8
ABS_T = 2e-8
BIOMES = ["b1", "b2", "b3", "b4"]


def ensemble96():
    S = np.repeat(np.linspace(1.5, 6.0, 12), 8)
    q10 = np.tile(np.linspace(1.2, 4.0, 8), 12)
    return S, q10


def biome_q10(q10, b):
    return q10 * (0.94 + 0.04 * b)


def biome_wf(b):
    return 0.85 + 0.1 * b


ORDERS = {"natural": np.arange(N), "reversed": np.arange(N)[::-1].copy(),
          "permuted": np.random.default_rng(20261020).permutation(N)}


def run_case(lib, scen, kernel, order=None, **kw):
    """The ensemble with member order[i] in place i -> its outputs back in the ensemble's order:
    {output: [556, 96]} and "status": [96]."""
    S, q10 = ensemble96()
    order = np.arange(N) if order is None else order
    c = hector_amd.Core(SCENARIOS[scen], N, lib_path=lib, **kw)
    assert kw.get("allow_emulation") or c.backend == "hip"
    c.set_pair_kernel_limit(0)
    two_wave = kernel.startswith("run2")
    c.set_two_wave_from(1 if two_wave else 0)
    c.set_member_sorting(False)
    nb = n_biomes(kernel)
    if nb > 1:
        names = BIOMES[:nb]
        c.split_biome(names)
        for b, nm in enumerate(names):
            c.setvar(nm + ".q10_rh", biome_q10(q10, b)[order])
            c.setvar(nm + ".warmingfactor", np.full(N, biome_wf(b)))
    else:
        c.setvar("q10_rh", q10[order], "(unitless)")
    c.setvar("S", S[order], "degC")
    if "diff" in kernel:
        c.setvar("diff", member_diff()[order], "cm2/s")
    c.set_outputs(OUTS + (["heatflux"] if kernel.endswith("_hf") else []) + (["NPP"] if kernel.endswith("_npp") else []))
    c.run(2300)
    assert c.last_run_kernel() == ("run2" if two_wave else "run")
    assert c.last_run_variant() == VARIANT[kernel][3], kernel
    inv = np.argsort(order)
    res = {v: c.fetchvars(v, (1745, 2300))[:, inv].copy() for v in OUTS}
    res["status"] = c.status()[inv].copy()
    c.shutdown()
    return res


def oracle_case(scen, kernel):
    """The oracle's run of every member -> {"CO2_concentration", "global_tas", "timesteps",
    "max_timestep": [556, 96]}.  ("run" and "run2" are the same members.)"""
    import oracle_binding
    orc = oracle_binding.Oracle(SCENARIOS[scen])
    S, q10 = ensemble96()
    keys = ("CO2_concentration", "global_tas", "timesteps", "max_timestep")
    cols = {k: [] for k in keys}
    for i in range(N):
        p = orc.default_params()
        nb = n_biomes(kernel)
        if nb > 1:
            p = orc.split_equal(p, nb)
            for b in range(nb):
                p.q10_rh[b] = biome_q10(q10, b)[i]
                p.warmingfactor[b] = biome_wf(b)
        else:
            p.q10_rh[0] = q10[i]
        p.S = S[i]
        if "diff" in kernel:
            p.diff = member_diff()[i]
        o, err, _ = orc.run(p)
        assert err == 0, (scen, kernel, i)
        for k in keys:
            cols[k].append(o[k].copy())
    return {k: np.array(v).T for k, v in cols.items()}


def check_against_oracle(r, o, what):
    """Every member at the project's tolerances, the stash schedule year by year, clean status."""
    assert (r["status"] == 0).all(), what
    rel = np.abs(r["CO2_concentration"] - o["CO2_concentration"]) / o["CO2_concentration"]
    dt = np.abs(r["global_tas"] - o["global_tas"])
    print("%s, 96 members vs oracle: max rel dCO2 %.3e, max |dTgav| %.3e" % (what, rel.max(), dt.max()))
    assert rel.max() < REL_CO2, what
    assert dt.max() < ABS_T, what
    assert np.array_equal(r["timesteps"][1:], o["timesteps"][1:]), what


def coverage(o):
    """What the oracle's own schedule of one case covers -> set of names.  max_timestep[y] is the
    ocean's max_timestep at the end of year y (ocean_component.cpp:703-733: halved, floor 0.3, when
    the air-sea flux jumps; doubled, cap 1, when the 20-stash timeout runs out, and the timeout
    re-armed while it stays below 1)."""
    ts = o["timesteps"][1:].astype(int)
    mt = o["max_timestep"]
    got = set()
    if (ts == 1).any():
        got.add("one_stash_years")
    if (ts == 2).any():
        got.add("two_stash_years")
    if (ts >= 3).any():
        got.add("three_and_more_stash_years")
    prev, cur = mt[:-1], mt[1:]
    if (cur < prev).any():
        got.add("halves_max_ts")
    up = cur > prev            # a doubling needs the timeout counted down to 0
    if (up & (cur < 1.0)).any():
        got.add("doubles_back_below_one_rearmed")
    if (up & (cur == 1.0)).any():
        got.add("doubles_back_to_exactly_one")
    # one wavefront (members 0-63 in the natural order) mixes lanes of different segment counts
    if (ts[:, :64].min(axis=1) != ts[:, :64].max(axis=1)).any():
        got.add("wavefront_mixes_segment_counts")
    return got


COVERAGE = {"one_stash_years", "two_stash_years", "three_and_more_stash_years", "halves_max_ts",
            "doubles_back_below_one_rearmed", "doubles_back_to_exactly_one",
            "wavefront_mixes_segment_counts"}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def golden_entries(r, prefix):
    """What the golden holds of one run: the outputs at GOLDEN_YEARS (float64), every stash count
    (uint8), the status words, and a SHA-256 of each output's whole [556, 96] float64 series."""
    rows = [y - 1745 for y in GOLDEN_YEARS]
    d = {}
    for v in OUTS:
        if v == "timesteps":
            d[prefix + v] = r[v].astype(np.uint8)
        else:
            d[prefix + v] = r[v][rows].astype(np.float64)
        d[prefix + v + "_sha256"] = np.array(digest(r[v]))
    d[prefix + "status"] = r["status"].astype(np.int64)
    return d


def check_against_golden(r, g, prefix, what):
    want = golden_entries(r, prefix)
    for k, v in want.items():
        assert k in g.files, k
        assert np.array_equal(g[k], v), (what, k)


# ---- the flag paths: members known to raise a status bit in the stash ---------------------------
# HX_ERR_NEGPOOL (4): the runaway member of test_host_logic.py (SSP1-1.9) between two clean ones,
# which stash on for 170 years while it idles with its status set.
# HX_ERR_MASS (1): an NBP constraint drives the warmest members out of mass balance late in the run
# (test_opening_retry_emulation.py's nbp_constrained case: the CON = 1 kernel).
RUNAWAY = {"S": 7.4981, "diff": 0.55557, "aero_scalar": 1.6819, "vol_scalar": 0.33619, "C0": 313.54,
           "tt": 41731000.0, "tu": 47115000.0, "twi": 11610000.0, "tid": 232640000.0,
           "beta": 0.46336, "q10_rh": 3.5869, "warmingfactor": 2.1026, "f_nppv": 0.29871,
           "f_nppd": 0.48862, "f_litterd": 0.93955, "rh_ch4_frac": 0.023349, "pf_mu": 0.88199,
           "pf_sigma": 1.3919, "fpf_static": 0.36564}
FLAG_OUTS = ["CO2_concentration", "global_tas", "timesteps"]


FLAG_CASES = {"negpool": 4, "mass": 1, "runaway_nbp": 1, "mass_diff": 1}
# the instantiations the flag cases run: the runaway member's own diffusivity makes "negpool" a
# per-member-diffusivity launch; "runaway_nbp" adds an NBP constraint (the stash then moves the thawed
# pool AFTER the clamp the flag is tested on); "mass" runs a kernel that keeps the nested form,
# "mass_diff" -- the same members with per-member diffusivity -- one of hx_flat_stash.
FLAG_VARIANT = {"negpool": (1, False, True, 0), "runaway_nbp": (1, True, True, 1),
                "mass": (1, True, False, 1), "mass_diff": (1, True, True, 1)}


def run_flag_case(lib, which, **kw):
    """which: a key of FLAG_CASES -> {output: [556, n]} and "status"."""
    if which in ("negpool", "runaway_nbp"):
        c = hector_amd.Core(os.path.join(ROOT, "hector_amd", "data", "ssp119.hxs"), 3, lib_path=lib, **kw)
        for k, v in RUNAWAY.items():
            base = c.getvar(k)[0]
            c.setvar(k, [base, v, base])
        if which == "runaway_nbp":
            years = np.arange(1950, 2051)
            c.setvar_dated("NBP_constrain", years, 0.5 + 0.01 * (years - 1950))
    else:
        n = 12
        S, q10 = ensemble96()
        idx = np.round(np.linspace(0, N - 1, n)).astype(int)
        c = hector_amd.Core(SCENARIOS["ssp245"], n, lib_path=lib, **kw)
        c.setvar("S", S[idx], "degC").setvar("q10_rh", q10[idx], "(unitless)")
        years = np.arange(1950, 2051)
        c.setvar_dated("NBP_constrain", years, 0.5 + 0.01 * (years - 1950))
        if which == "mass_diff":
            c.setvar("diff", member_diff()[idx], "cm2/s")
    assert kw.get("allow_emulation") or c.backend == "hip"
    c.set_pair_kernel_limit(0)
    c.set_two_wave_from(0)
    c.set_outputs(FLAG_OUTS)
    c.run(2300)
    assert c.last_run_kernel() == "run"
    assert c.last_run_variant() == FLAG_VARIANT[which][3], which
    res = {v: c.fetchvars(v, (1745, 2300)).copy() for v in FLAG_OUTS}
    res["status"] = c.status().copy()
    c.shutdown()
    return res
