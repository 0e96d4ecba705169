"""Carbon tracking (fluxpool origin maps, inst/include/fluxpool.hpp; SimpleNbox::stashCValues
src/simpleNbox-runtime.cpp:289-540; oceanbox.cpp:240-303; CSVFluxPoolVisitor) on the kernel
source compiled for the host, against the oracle's restatement, plus the properties
tests/testthat/test_tracking.R states.  The GPU suite repeats the comparison through HIP."""
import numpy as np
import pytest

import hector_amd
from conftest import SCENARIO

T0, END = 1770, 2100
FRAC_TOL = 1e-8


def tracked_core(lib, n, date=T0, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, **kw)
    c.setvar("trackingDate", [date])
    return c


def check_tracking_vs_oracle(lib, oracle, **kw):
    c = tracked_core(lib, 3, **kw)
    q10 = c.getvar("q10_rh"); q10[1] *= 0.9; q10[2] = 2.6
    S = np.array([3.0, 3.0, 4.5])
    c.setvar("q10_rh", q10).setvar("S", S, "degC")
    POOL_VARS = {"atmos_co2": "atmos_co2", "earth_c": "earth_c", "veg_c": "veg_c",
                 "detritus_c": "detritus_c", "soil_c": "soil_c", "HL": "HL_ocean_c",
                 "LL": "LL_ocean_c", "intermediate": "IO_ocean_c", "deep": "DO_ocean_c"}
    c.set_outputs(["CO2_concentration"] + list(POOL_VARS.values()))
    c.run(END)
    assert (c.status() == 0).all()
    assert c.getvar("trackingDate")[0] == T0
    names = c.tracking_pools()
    assert names == ["atmos_co2", "earth_c", "veg_c", "detritus_c", "soil_c", "permafrost_c",
                     "thawedp_c", "HL", "LL", "intermediate", "deep"]
    for i in range(3):
        p = oracle.default_params(); p.q10_rh[0] = q10[i]; p.S = S[i]
        ov, of, _, err = oracle.run_tracking(p, T0, END)
        assert err == 0
        gv, gf = c.tracking_data(i, (T0, END))
        k0, k1 = T0 - 1745, END - 1745 + 1
        # pools to ~1e-11 relative like every other output; fractions are ratios of sums of
        # fluxes, and in small pools (thawed permafrost, detritus) the 1e-11 differences of the
        # fluxes are amplified: FRAC_TOL absolute on numbers in [0, 1]
        assert np.abs(gv - ov[k0:k1]).max() < 1e-10 * np.abs(ov).max()
        assert np.abs(gf - of[k0:k1]).max() < FRAC_TOL
        # every pool's origins sum to 1 (test_tracking.R:96-101)
        assert np.abs(gf.sum(axis=2) - 1.0).max() < 1e-12
        # first tracked year: mostly itself; the pool values are the model's (test_tracking.R:163-)
        assert gf[0, 1, 1] == 1.0
        # test_tracking.R:164-262 "Pool names are valid": the value tracked for each of the nine
        # pools equals fetchvars(<pool variable>) (the R test allows 1e-3; here every year, exactly)
        # and carries its unit
        for pool, var in POOL_VARS.items():
            assert np.array_equal(gv[:, names.index(pool)], c.fetchvars(var, (T0, END))[:, i]), pool
            assert c.getunits(var) == "Pg C"
    # ... and the source names are the pool names (test_tracking.R:258-262)
    rows = hector_amd.get_tracking_data(c, member=0)
    assert sorted({r[5] for r in rows}) == sorted({r[2] for r in rows}) == sorted(names)
    return c


def test_tracking_vs_oracle(emul_lib, oracle):
    c = check_tracking_vs_oracle(emul_lib, oracle, allow_emulation=True)
    # a changed parameter changes the origins (test_tracking.R:30-50)
    _, f0 = c.tracking_data(0, (T0, END)); _, f1 = c.tracking_data(1, (T0, END))
    assert np.abs(f0 - f1).max() > 1e-4
    rows = hector_amd.get_tracking_data(c, 0)
    years = sorted({r[0] for r in rows})
    assert years == list(range(T0, END + 1))  # test_tracking.R:70-90
    assert {r[1] for r in rows} == {"simpleNbox", "ocean"} and {r[4] for r in rows} == {"Pg C"}


def test_tracking_changes_nothing_else(emul_lib):
    """Tracking only observes: the run itself is the untracked run (to the rounding differences
    between two instantiations of the run kernel)."""
    a = hector_amd.Core(SCENARIO, 2, lib_path=emul_lib, allow_emulation=True)
    b = tracked_core(emul_lib, 2, allow_emulation=True)
    for c in (a, b):
        c.setvar("S", [2.5, 4.0], "degC"); c.run(2100)
    for v in ("CO2_concentration", "global_tas"):
        d = np.abs(a.fetchvars(v, (1745, 2100)) - b.fetchvars(v, (1745, 2100))).max()
        print(v, d)
        assert d < 1e-10


def test_no_tracking_is_empty(emul_lib):
    c = hector_amd.Core(SCENARIO, 1, lib_path=emul_lib, allow_emulation=True)
    c.run(1760)
    assert hector_amd.get_tracking_data(c) == []          # test_tracking.R:12-20
    assert c.getvar("trackingDate")[0] == 9999            # core.cpp:60
    with pytest.raises(hector_amd.HectorAmdError):
        c.tracking_data(0, (1750, 1760))
    # a tracking date that a run can never reach (simpleNbox-runtime.cpp:217: runToDate == tdate)
    c.setvar("trackingDate", [1745]); c.run(1760)
    assert c.getvar("trackingDate")[0] == 1745
    with pytest.raises(hector_amd.HectorAmdError):
        c.tracking_data(0, (1750, 1760))


def test_tracking_with_reset(emul_lib):
    tracking_reset_checks(emul_lib, allow_emulation=True)


def tracking_reset_checks(lib, **kw):
    """test_tracking.R:104-160: reset below the tracking date empties the record, a reset at or
    past it resumes with the maps of that date; a run-reset-run reproduces the straight run."""
    c = tracked_core(lib, 2, date=1760, **kw)
    c.enable_history(True)
    c.setvar("S", [3.0, 4.0], "degC")
    c.run(1800)
    v0, f0 = c.tracking_data(1, (1760, 1800))
    c.reset(1750)
    assert hector_amd.get_tracking_data(c) == []
    assert c.getvar("trackingDate")[0] == 1760
    c.run(1770)
    rows = hector_amd.get_tracking_data(c, 1)
    assert min(r[0] for r in rows) == 1760 and max(r[0] for r in rows) == 1770
    c.reset(1765)                       # >= trackingDate
    c.run(1800)
    v1, f1 = c.tracking_data(1, (1760, 1800))
    assert np.array_equal(v0, v1) and np.array_equal(f0, f1)
    c.reset(1760); c.run(1780); c.run(1800)
    v2, f2 = c.tracking_data(1, (1760, 1800))
    assert np.array_equal(v0, v2) and np.array_equal(f0, f2)
    with pytest.raises(hector_amd.HectorAmdError):
        c.tracking_data(1, (1750, 1800))


def test_tracking_four_biomes(emul_lib, oracle):
    tracking_four_biomes(emul_lib, oracle, allow_emulation=True)


def tracking_four_biomes(lib, oracle, **kw):
    tracking_n_biomes(lib, oracle, 4, **kw)


def tracking_n_biomes(lib, oracle, nb, run_to=2050, **kw):
    """`nb` equal biomes with their own Q10 per member: pools, fractions and which sources are in
    the maps, against the oracle.  5-16 biomes take the looped kernels (run-time pool count), 12
    and more have over 64 pools: two mask words per pool."""
    c = tracked_core(lib, 2, date=1800, **kw)
    names = ["b%d" % (b + 1) for b in range(nb)]
    c.split_biome(names)
    q = [[1.8 + 0.07 * ((5 * b) % 11), 2.6 - 0.05 * ((3 * b) % 13)] for b in range(nb)]
    for b, nm in enumerate(names):
        c.setvar(nm + ".q10_rh", q[b])
    c.run(run_to)
    assert (c.status() == 0).all()
    pools = c.tracking_pools()
    tp = 6 + 5 * nb
    assert len(pools) == tp and pools[2] == "b1.veg_c" and pools[tp - 5] == "b%d.thawedp_c" % nb
    k0, k1 = 1800 - 1745, run_to - 1745 + 1
    for i in range(2):
        p = oracle.split_equal(oracle.default_params(), nb)
        for b in range(nb):
            p.q10_rh[b] = q[b][i]
        ov, of, _, err = oracle.run_tracking(p, 1800, run_to)
        assert err == 0
        gv, gf, held = c.tracking_data(i, (1800, run_to), masks=True)
        assert np.abs(gv - ov[k0:k1]).max() < 1e-10 * np.abs(ov).max()
        assert np.abs(gf - of[k0:k1]).max() < FRAC_TOL
        assert np.abs(gf.sum(axis=2) - 1.0).max() < 1e-12
        # a source outside the map has no share; every pool holds itself; the atmosphere ends up
        # holding every pool that has carbon to give (the highest-numbered ones included)
        assert (gf[~held] == 0.0).all()
        assert held[:, np.arange(tp), np.arange(tp)].all()
        assert held[-1, 0, tp - 4:].all() and held[-1, 0, 2:tp - 4:5].all()
    return c


@pytest.mark.parametrize("nb", [5, 12])
def test_tracking_beyond_four_biomes(emul_lib, oracle, nb):
    """The reference tracks any number of biomes (fluxpool maps are string-keyed); here 5-16 run
    on the looped kernels.  12 biomes = 66 pools: the second mask word."""
    tracking_n_biomes(emul_lib, oracle, nb, run_to=1900, allow_emulation=True)


def test_tracking_refuses_carbon_constraints(emul_lib, tmp_path):
    from conftest import edited_pack
    pack = edited_pack(tmp_path / "c.hxs", "simpleNbox", "CO2_constrain", [1800, 1801], [285.0, 285.2])
    c = hector_amd.Core(str(pack), 1, lib_path=emul_lib, allow_emulation=True)
    c.setvar("trackingDate", [1770])
    with pytest.raises(hector_amd.HectorAmdError, match="constraint"):
        c.run(1850)


# ---------------------------------------------------------------------------------------------
# Every member's maps against the oracle, on an ensemble whose lanes part ways and whose edge
# members empty a pool.  (tests/test_gpu_tracking_maps.py: the same checker on the device, where
# one and two biomes keep their maps on companion wavefronts -- code the host build never runs.)
#
# 70 members: one full wavefront and six lanes.  S, the Q10 and beta are spread widely, so the
# lanes of a wavefront take different numbers of stashes in many years (the companions' partial-
# wavefront protocol, TRKR_ACTIVE); members at fixed indices sit at the values where a pool or a
# flux is exactly zero: permafrost_c = 0 (the permafrost map is "a zero total, shared equally
# among the names of the map", fluxpool.hpp:243-251, every year -- next to lanes with ordinary
# maps), fpf_static = 1 and 0, beta = 0, f_litterd = 1.  Member 0 holds the INI defaults.
EDGE_N = 70
EDGE_PF0 = (7, 30, 58)
EDGE_MEMBERS = (0,) + EDGE_PF0 + (12, 41, 23, 50)   # the host tier's eight
EDGE_SPANS = {"ssp245": (1950, 2100), "ssp534-over": (2000, 2150)}   # tracking date, run to
_oracles, _oracle_runs = {}, {}


def edge_ensemble(diff=False):
    """-> {parameter: values[EDGE_N]}, in the units of the unsplit core."""
    from test_one_factor import DEFAULTS
    rng = np.random.default_rng(2025)
    e = {"S": rng.uniform(1.5, 6.0, EDGE_N), "q10_rh": rng.uniform(1.1, 3.0, EDGE_N),
         "beta": rng.uniform(0.2, 0.9, EDGE_N)}
    for k in ("permafrost_c", "fpf_static", "f_litterd"):
        e[k] = np.full(EDGE_N, DEFAULTS[k])
    if diff:   # (its own stream: the other rows are the same with and without it)
        e["diff"] = np.random.default_rng(2026).uniform(0.8, 2.4, EDGE_N)
    for k in ("S", "q10_rh", "beta"):
        e[k][0] = DEFAULTS[k]
    e["permafrost_c"][list(EDGE_PF0)] = 0.0
    e["fpf_static"][12], e["fpf_static"][41] = 1.0, 0.0
    e["beta"][23] = 0.0
    e["f_litterd"][50] = 1.0
    return e


def scenario_oracle(name):
    """(pack path, its oracle) of a shipped scenario."""
    import os
    import oracle_binding
    from conftest import ROOT
    path = os.path.join(ROOT, "hector_amd", "data", name + ".hxs")
    if name not in _oracles:
        _oracles[name] = oracle_binding.Oracle(path)
    return path, _oracles[name]


def edge_core(lib, path, ens, nb, date, members=None, **kw):
    """The core of `ens` (its `members`, default all): per-biome parameters in the LAST of `nb`
    equal biomes, pools scaled by the biome's share (test_one_factor.make_core)."""
    from test_one_factor import PARAMS, biome_values, capability
    idx = np.arange(EDGE_N) if members is None else np.asarray(members)
    c = hector_amd.Core(path, len(idx), lib_path=lib, **kw)
    if nb > 1:
        c.split_biome(["b%d" % b for b in range(nb)])
    c.set_pair_kernel_limit(0)
    c.setvar("trackingDate", [date])
    for k, v in ens.items():
        c.setvar(capability(k, nb), biome_values(k, v[idx], nb), PARAMS[k][2])
    c.set_outputs(["CO2_concentration", "timesteps"] + [pool_variable(p) for p in c.tracking_pools()])
    return c


def edge_params(o, ens, i, nb):
    from test_one_factor import ORACLE_SCALARS, biome_values
    p = o.default_params()
    if nb > 1:
        p = o.split_equal(p, nb)
    p.nbiome = nb
    for k, v in ens.items():
        if k in ORACLE_SCALARS:
            setattr(p, k, v[i])
        else:
            getattr(p, k)[nb - 1] = biome_values(k, [v[i]], nb)[0]
    return p


def pool_variable(pool):
    return {"HL": "HL_ocean_c", "LL": "LL_ocean_c", "intermediate": "IO_ocean_c", "deep": "DO_ocean_c"}.get(pool, pool)


def oracle_maps(oracle, p, T0, END):
    """(values, fractions, stashes per year) of the tracked span; computed once per member."""
    key = (oracle.sc, bytes(p), T0, END)
    if key not in _oracle_runs:
        k0, k1 = T0 - oracle.start, END - oracle.start + 1
        ov, of, _, err = oracle.run_tracking(p, T0, END)
        assert err == 0
        r, err, _ = oracle.run(p, END)
        assert err == 0
        _oracle_runs[key] = (ov[k0:k1].copy(), of[k0:k1].copy(), r["timesteps"][k0 + 1:k1].copy())
    return _oracle_runs[key]


def check_maps_every_member(core, oracle, params_of_member, T0, END, daccs=False, wavefront=True,
                            min_divergent=1.0 / 3.0, min_counts=3):
    """EVERY member's tracking_data(i, (T0, END), masks=True) of a core that has run to END
    against oracle.run_tracking(params_of_member(i)), at this file's tolerances.  -> the worst
    pool (relative to the largest pool) and fraction deviations.

    First, on the oracle's output alone, that the case exercises what it is there for:
    - wavefront: within lanes 0-63 the stashes per year differ between lanes in at least
      `min_divergent` of the tracked years (the host build runs its lanes one after the other:
      nothing parts there);
    - every permafrost_c = 0 member's permafrost row is equal shares in every tracked year, with
      at least `min_counts` different numbers of sources over the span;
    - daccs: earth_c ends up less than 99 % itself (direct air capture moves atmosphere there)."""
    n = core.n_members
    assert (core.status() == 0).all()
    pools = core.tracking_pools()
    tp = len(pools)
    nb = (tp - 6) // 5
    ref = [oracle_maps(oracle, params_of_member(i), T0, END) for i in range(n)]
    if wavefront:
        lanes = core.lane_of_member()
        ts = np.array([ref[i][2] for i in range(n) if lanes[i] < 64])
        parted = int((ts.max(axis=0) != ts.min(axis=0)).sum())
        print("lanes take different numbers of stashes in %d of %d years; stashes a year %s"
              % (parted, ts.shape[1], sorted(set(ts.ravel().astype(int)))))
        assert parted >= min_divergent * ts.shape[1], (parted, ts.shape[1])
    zero_pf = 0
    for i in range(n):
        p = params_of_member(i)
        for b in range(nb):
            if p.permafrost_c[b] == 0.0:
                row = ref[i][1][:, 2 + 5 * b + 3, :]
                cnt = (row > 0).sum(axis=1)
                assert np.array_equal(row, np.where(row > 0, 1.0 / cnt[:, None], 0.0)), i
                assert len(set(cnt)) >= min_counts, (i, sorted(set(cnt)))
                zero_pf += 1
    if daccs:
        assert max(r[1][-1, 1, 1] for r in ref) < 0.99
    recorded = {pool: core.fetchvars(pool_variable(pool), (T0, END)) for pool in pools}
    worst_v = worst_f = 0.0
    for i in range(n):
        ov, of, _ = ref[i]
        gv, gf, held = core.tracking_data(i, (T0, END), masks=True)
        dv, df = np.abs(gv - ov).max() / np.abs(ov).max(), np.abs(gf - of).max()
        worst_v, worst_f = max(worst_v, dv), max(worst_f, df)
        assert dv < 1e-10, (i, dv)
        assert df < FRAC_TOL, (i, df)
        assert np.abs(gf.sum(axis=2) - 1.0).max() < 1e-12, i
        assert (gf[~held] == 0.0).all(), i
        assert held[:, np.arange(tp), np.arange(tp)].all(), i
        for k, pool in enumerate(pools):
            assert np.array_equal(gv[:, k], recorded[pool][:, i]), (i, pool)
    print("%d members, %d pools (%d with permafrost_c = 0): worst pool deviation %.2e relative, "
          "worst fraction deviation %.2e" % (n, tp, zero_pf, worst_v, worst_f))
    return worst_v, worst_f


HOST_EDGE_CASES = [("ssp245", 1), ("ssp245", 2), ("ssp245", 4), ("ssp245", 13), ("ssp534-over", 1),
                   ("ssp534-over", 2)]


def edge_min_counts(scenario, T0):
    """How many different source counts the oracle's equal-shares permafrost row shows: the names
    arrive with the first non-zero flux of each kind, so a span that starts in 1950 on ssp245
    passes through 4, 9, 10 and 11 names (one biome); by 2000 on ssp534-over every flux runs and
    the row holds every name from the first stash on; 1900-1960 sees two counts."""
    return 3 if (scenario, T0) == ("ssp245", 1950) else 2 if scenario == "ssp245" else 1


@pytest.mark.parametrize("scenario,nb", HOST_EDGE_CASES, ids=["%s-%d" % c for c in HOST_EDGE_CASES])
def test_maps_of_edge_members_vs_oracle(emul_lib, scenario, nb):
    """The inline maps (track_stash) on the host build where a pool or a flux is exactly zero:
    the edge members and the default one, 1-13 biomes (13: 71 pools, the zero pool's bits in the
    second mask word), with and without direct air capture."""
    path, o = scenario_oracle(scenario)
    T0, END = (1900, 1960) if nb == 13 else EDGE_SPANS[scenario]
    ens = edge_ensemble()
    c = edge_core(emul_lib, path, ens, nb, T0, members=EDGE_MEMBERS, allow_emulation=True)
    c.run(END)
    assert c.last_run_kernel() == "run" and c.last_run_variant() == 2
    check_maps_every_member(c, o, lambda i: edge_params(o, ens, EDGE_MEMBERS[i], nb), T0, END,
                            daccs=scenario == "ssp534-over", wavefront=False,
                            min_counts=edge_min_counts(scenario, T0))


TRACK_BOTH_WAYS = """
import sys, numpy as np, hector_amd
from hector_amd import ensemble
out = {}
for nb in (1, 2):
    n = 200
    S, q = ensemble.ecs_q10(n, offset=5)
    c = hector_amd.Core(hector_amd.DEFAULT_SCENARIO, n, device=0)
    if nb > 1:
        c.split_biome(["a", "b"], fveg_c=[0.3, 0.7])
        c.setvar("a.q10_rh", q)
    else:
        c.setvar("q10_rh", q)
    c.setvar("S", S, "degC").setvar("trackingDate", [1800.0])
    c.run(1900)
    c.run(2000)           # resumes past the tracking date: the maps come back from the record
    assert (c.status() == 0).all()
    for i in (0, 63, 64, 199):
        v, f, held = c.tracking_data(i, (1800, 2000), masks=True)
        out["v%d_%d" % (nb, i)] = v; out["f%d_%d" % (nb, i)] = f; out["m%d_%d" % (nb, i)] = held
    c.reset(1850); c.run(1950)   # reset(date) into the tracked span needs the history: refused or redone
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_companion_wavefronts_and_inline_maps_agree_on_gpu(tmp_path):
    """One and two biomes track on companion wavefronts (hx_run_kernel<B,HF,KERPM,3>: the maps in
    the registers of wavefronts that do nothing else), HECTOR_AMD_TRACK_INLINE=1 keeps the maps
    in the record and mixes inside the stash (what 3-16 biomes and big two-biome ensembles do):
    the same pools bit for bit, the same names in every map, fractions to rounding."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    res = {}
    for mode in ("companions", "inline"):
        env = dict(os.environ)
        env.pop("HECTOR_AMD_TRACK_INLINE", None)
        if mode == "inline":
            env["HECTOR_AMD_TRACK_INLINE"] = "1"
        path = str(tmp_path / (mode + ".npz"))
        script = TRACK_BOTH_WAYS.replace("c.reset(1850); c.run(1950)", "pass")
        r = subprocess.run([sys.executable, "-c", script, path], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        res[mode] = np.load(path)
    a, b = res["companions"], res["inline"]
    for k in a.files:
        if k.startswith("v"):
            assert np.array_equal(a[k], b[k]), k
        elif k.startswith("m"):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert np.abs(a[k] - b[k]).max() < 1e-12, k
            assert np.abs(a[k].sum(axis=2) - 1.0).max() < 1e-12
