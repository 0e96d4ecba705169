"""The opening retry of the run kernels and of the pair kernel (a segment's retries decided before
its first step: solve_year in hx_dev_solver.h, pair_open_retry in hx_dev_pair.h) on the MI355X.

96 members -- one full wavefront and a half-filled one -- of test_gpu_step_control.py's ensemble
(S 1.5-6 x Q10 1.2-4, SSP2-4.5, 1745-2300): lanes that take their retries in the same segment as
wave-mates that take none.

 - the fast path against the faithful one (HECTOR_AMD_FAITHFUL_RETRIES=1: the retries inside the
   step loop, discarded steps executed) bit for bit: run kernel, two-wave flavour, pair kernel,
   four biomes, NPP recorded;
 - the fast path's rows at the years of tests/golden/step_control_parent.npz equal that file's
   (recorded two changes of the step loop ago); `solver_steps` is not compared -- recording it
   selects the faithful path, which test_gpu_step_control.py holds to the file;
 - wave-mates do not matter on the fast path: reversed, permuted and cost-sorted lane orders;
 - every member within 2e-8 of the oracle, with the stash schedule equal;
 - a member that must be flagged has the same status word on both paths;
 - the fast path IS taken: under HECTOR_AMD_FAITHFUL_RETRIES=0 `solver_steps` counts fewer steps
   than the faithful launch, and hx_last_run_retries says which path every launch here took.

(CPU twin: test_opening_retry_emulation.py.)"""
import os

import numpy as np
import pytest

import hector_amd
from conftest import ROOT, SCENARIO

pytestmark = pytest.mark.gpu

ENV = "HECTOR_AMD_FAITHFUL_RETRIES"
REL_CO2 = 2e-8
ABS_T = 2e-8
N = 96
OUTS = ["CO2_concentration", "global_tas", "sst", "land_tas", "timesteps"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_control_parent.npz")


def ensemble96():
    S = np.repeat(np.linspace(1.5, 6.0, 12), 8)
    q10 = np.tile(np.linspace(1.2, 4.0, 8), 12)
    return S, q10


def _biomes(c):
    names = ["b1", "b2", "b3", "b4"]
    c.split_biome(names, fveg_c=[0.1, 0.2, 0.3, 0.4], fdetritus_c=[0.4, 0.3, 0.2, 0.1],
                  fsoil_c=[0.25, 0.25, 0.3, 0.2], fpermafrost_c=[0.0, 0.1, 0.3, 0.6],
                  fnpp_flux0=[0.35, 0.3, 0.2, 0.15])
    for b, nm in enumerate(names):
        c.setvar(nm + ".q10_rh", np.linspace(1.2 + 0.2 * b, 2.4 + 0.2 * b, N))
        c.setvar(nm + ".warmingfactor", np.full(N, 1.0 + 0.25 * b))


def _nbp_con(c):
    years = np.arange(1950, 2051)
    c.setvar_dated("NBP_constrain", years, 0.5 + 0.01 * (years - 1950))


def _co2_con(c):
    years = np.arange(1850, 2101)
    c.setvar_dated("CO2_constrain", years, 280.0 + 0.9 * (years - 1850) + 0.004 * (years - 1850) ** 2, "ppmv CO2")


def _run(hip_lib, faithful, kernel="run", order=None, sorting=False, outs=OUTS, biomes=False, setup=None,
         nbp=False):
    """The ensemble with member order[i] in place i -> its outputs back in the ensemble's order.
    faithful: False (the fast path), True (HECTOR_AMD_FAITHFUL_RETRIES=1) or "count" (=0: the fast
    path although `outs` records solver_steps, which then counts the executed steps)."""
    mp = pytest.MonkeyPatch()
    try:
        if faithful == "count":
            mp.setenv(ENV, "0")
        elif faithful:
            mp.setenv(ENV, "1")
        else:
            mp.delenv(ENV, raising=False)
        S, q10 = ensemble96()
        order = np.arange(N) if order is None else order
        c = hector_amd.Core(SCENARIO, N, device=0, lib_path=hip_lib)
        assert c.backend == "hip"
        if kernel != "pair":
            c.set_pair_kernel_limit(0)
        c.set_two_wave_from(1 if kernel == "run2" else 0)
        c.set_member_sorting(sorting)
        c.setvar("S", S[order], "degC")
        if biomes:
            _biomes(c)
        else:
            c.setvar("q10_rh", q10[order], "(unitless)")
        if setup:
            setup(c)
        c.set_outputs(outs)
        c.run(2300)
        assert c.last_run_kernel() == kernel
        # (nbp: the NBP-capable kernels are held to the faithful path whatever is asked for)
        assert c.last_run_retries() == (1 if nbp or faithful is True or (not faithful and "solver_steps" in outs) else 0)
        inv = np.argsort(order)
        res = {v: c.fetchvars(v, (1745, 2300))[:, inv].copy() for v in outs}
        res["status"] = c.status()[inv].copy()
        res["lanes"] = c.lane_of_member().copy()
        c.shutdown()
        return res
    finally:
        mp.undo()


def same(a, b, outs, what):
    for v in list(outs) + ["status"]:
        assert np.array_equal(a[v], b[v], equal_nan=True), (what, v)


ORDERS = {"reversed": np.arange(N)[::-1].copy(),
          "permuted": np.random.default_rng(20261020).permutation(N)}


@pytest.fixture(scope="module")
def fast(hip_lib):
    """The fast path in the natural order, kernel by kernel, once."""
    return {k: _run(hip_lib, False, k) for k in ("run", "run2", "pair")}


@pytest.mark.parametrize("kernel", ["run", "run2", "pair"])
def test_fast_path_equals_faithful_path(hip_lib, fast, kernel):
    f = fast[kernel]
    assert (f["status"] == 0).all()
    assert set(np.unique(f["timesteps"][1:]).astype(int)) >= {1, 2, 4}
    same(f, _run(hip_lib, True, kernel), OUTS, kernel)


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_the_fast_path_is_taken_and_executes_fewer_steps(hip_lib, fast, kernel):
    """If the launch constant were stuck, or read wrongly by the kernel, every comparison of the two
    paths in this file would hold trivially.  With solver_steps recorded, the faithful launch counts
    the reference's steps and the launch under HECTOR_AMD_FAITHFUL_RETRIES=0 the executed ones:
    fewer for every member, never more in any year, the other outputs the same bits.  (The pair
    kernel does not record solver_steps -- such a run goes to the run kernel -- so for it the time
    of the launch is the evidence: profiles/opening_retry_ab.md section 3.)"""
    outs = OUTS + ["solver_steps"]
    ref = _run(hip_lib, False, kernel, outs=outs)         # recording it selects the faithful path
    cnt = _run(hip_lib, "count", kernel, outs=outs)
    same(ref, cnt, OUTS, (kernel, "count"))
    same(fast[kernel], cnt, OUTS, (kernel, "fast"))
    a, b = ref["solver_steps"][1:], cnt["solver_steps"][1:]
    print("%s kernel: steps per member-year faithful %.3f -> executed %.3f" % (kernel, a.mean(), b.mean()))
    assert (b <= a).all() and (b.sum(0) < a.sum(0)).all()
    assert (b >= cnt["timesteps"][1:]).all()


def test_nbp_constrained_runs_stay_on_the_faithful_path(hip_lib):
    """The six-variable solver (an NBP constraint: CON = 1), on the two-wave flavour, whose CON = 1
    kernel has the opening block.  With the block taken, CO2_concentration of this ensemble differed
    from the faithful path's in its last bits on the MI355X (none on the host emulation; the likely
    cause: the kernel holds a fresh stepper's first right-hand side twice, ahead of the step loop and
    inside the retry block, and the two copies need not be contracted alike).  So EnsembleCore::run keeps every
    NBP-capable launch on the faithful path: no mode changes a bit or a step count of such a run."""
    outs = OUTS + ["NBP", "solver_steps"]
    kw = dict(outs=outs, setup=_nbp_con, nbp=True)
    ref = _run(hip_lib, True, "run2", **kw)
    # (the constraint drives the warmest members out of mass balance late in the run: flagged in
    # every mode alike; more than half run clean to 2300)
    assert (ref["status"] == 0).sum() > N // 2 and ref["timesteps"][1:].max() >= 2
    same(ref, _run(hip_lib, "count", "run2", **kw), outs, "NBP constrained, =0")
    f = _run(hip_lib, False, "run2", outs=OUTS + ["NBP"], setup=_nbp_con, nbp=True)
    same(f, ref, OUTS + ["NBP"], "NBP constrained, solver_steps not recorded")


def test_fast_path_equals_faithful_path_co2_constrained(hip_lib):
    """The extended kernel without the NBP machinery (CON = -1): a CO2-constrained run."""
    outs = OUTS + ["NBP"]
    f = _run(hip_lib, False, outs=outs, setup=_co2_con)
    assert (f["status"] == 0).all() and f["timesteps"][1:].max() >= 2
    same(f, _run(hip_lib, True, outs=outs, setup=_co2_con), outs, "CO2 constrained")
    outs_n = outs + ["solver_steps"]
    ref = _run(hip_lib, False, outs=outs_n, setup=_co2_con)
    cnt = _run(hip_lib, "count", outs=outs_n, setup=_co2_con)
    same(f, cnt, outs, "CO2 constrained, count")
    a, b = ref["solver_steps"][1:], cnt["solver_steps"][1:]
    assert (b <= a).all() and (b.sum(0) < a.sum(0)).all()


def test_fast_path_equals_faithful_path_four_biomes(hip_lib):
    outs = OUTS + ["veg_c", "permafrost_c"]
    f = _run(hip_lib, False, outs=outs, biomes=True)
    assert (f["status"] == 0).all() and f["timesteps"][1:].max() >= 2
    same(f, _run(hip_lib, True, outs=outs, biomes=True), outs, "four biomes")


def test_fast_path_equals_faithful_path_npp_recorded(hip_lib):
    outs = OUTS + ["NPP"]      # (the diagnostics instantiation of the run kernel)
    f = _run(hip_lib, False, outs=outs)
    assert (f["status"] == 0).all() and f["timesteps"][1:].max() >= 2
    same(f, _run(hip_lib, True, outs=outs), outs, "NPP recorded")


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_fast_path_rows_equal_the_golden_file(hip_lib, kernel):
    g = np.load(GOLDEN)
    S, q10 = ensemble96()
    assert np.array_equal(g["S"], S) and np.array_equal(g["q10"], q10)
    sfx = "" if kernel == "run" else "_run2"
    rows = [int(y) - 1745 for y in g["years"]]
    r = _run(hip_lib, False, kernel, sorting=True)      # (the file was recorded with the default lane order)
    assert np.array_equal(r["CO2_concentration"][rows], g["co2" + sfx])
    assert np.array_equal(r["global_tas"][rows], g["tgav" + sfx])
    assert np.array_equal(r["timesteps"][1:].sum(0).astype(np.int64), g["timesteps" + sfx])


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_wave_mates_do_not_matter_on_the_fast_path(hip_lib, fast, kernel):
    ref = fast[kernel]
    assert np.array_equal(ref["lanes"], np.arange(N))
    for name, order in ORDERS.items():
        same(ref, _run(hip_lib, False, kernel, order=order), OUTS, (kernel, name))
    s = _run(hip_lib, False, kernel, sorting=True)
    assert not np.array_equal(s["lanes"], np.arange(N))
    same(ref, s, OUTS, (kernel, "sorted"))


@pytest.fixture(scope="module")
def oracle96(oracle):
    S, q10 = ensemble96()
    co2, tg, ts = [], [], []
    for i in range(N):
        p = oracle.default_params(); p.S = S[i]; p.q10_rh[0] = q10[i]
        r, err, _ = oracle.run(p)
        assert err == 0, (i, S[i], q10[i])
        co2.append(r["CO2_concentration"]); tg.append(r["global_tas"]); ts.append(r["timesteps"])
    return np.array(co2).T, np.array(tg).T, np.array(ts).T


@pytest.mark.parametrize("kernel", ["run", "run2", "pair"])
def test_every_member_against_the_oracle(fast, oracle96, kernel):
    oco2, otg, ots = oracle96
    r = fast[kernel]
    rel = np.abs(r["CO2_concentration"] - oco2) / oco2
    dt = np.abs(r["global_tas"] - otg)
    print("%s kernel, fast path, 96 members vs oracle: max rel dCO2 %.3e, max |dTgav| %.3e"
          % (kernel, rel.max(), dt.max()))
    assert rel.max() < REL_CO2
    assert dt.max() < ABS_T
    assert np.array_equal(r["timesteps"][1:], ots[1:])      # the stash schedule, year by year


def test_flagged_member_has_the_same_status_on_both_paths(hip_lib):
    """test_emulation_parity.py::test_model_errors_are_flags_not_crashes' member (its CPU twin on
    both paths: test_opening_retry_emulation.py)."""
    S = np.full(N, 3.0)
    npp = np.full(N, 56.2); npp[[1, 70]] = 1e5
    res = {}
    mp = pytest.MonkeyPatch()
    try:
        for faithful in (False, True):
            if faithful:
                mp.setenv(ENV, "1")
            else:
                mp.delenv(ENV, raising=False)
            c = hector_amd.Core(SCENARIO, N, device=0, lib_path=hip_lib)
            c.set_pair_kernel_limit(0)
            c.set_two_wave_from(0)
            c.setvar("S", S, "degC").setvar("npp_flux0", npp)
            c.set_outputs(["CO2_concentration"])
            c.run(1800)
            assert c.last_run_kernel() == "run"
            res[faithful] = (c.status().copy(), c.fetchvars("CO2_concentration", (1745, 1800)).copy())
            c.shutdown()
    finally:
        mp.undo()
    st, co2 = res[False]
    bad = np.zeros(N, bool); bad[[1, 70]] = True
    assert (st[bad] != 0).all() and (st[~bad] == 0).all()
    assert np.array_equal(res[True][0], st)
    assert np.array_equal(co2[:, ~bad], res[True][1][:, ~bad])
    assert (co2[:, ~bad] == co2[:, [0]]).all() and np.isfinite(co2[:, 0]).all()
