"""The opening retry of the run kernels (solve_year, hx_dev_solver.h: a segment's retries decided
before its first step) under host emulation: the fast path against the faithful one -- the retries
taken inside the step loop, as the reference takes them -- bit for bit.

The faithful path is forced in two ways: by HECTOR_AMD_FAITHFUL_RETRIES=1 in the environment, and
by recording `solver_steps` (the reference's count includes the steps a retry discards, so a
launch that records it must execute them).  HECTOR_AMD_FAITHFUL_RETRIES=0 keeps the fast path even
with `solver_steps` recorded: the output then counts the steps that were executed.

Every comparison is np.array_equal: the two paths do the same arithmetic on the same values, the
fast one only leaves out steps whose results the retry throws away.

(GPU twin: test_gpu_opening_retry.py.)"""
import numpy as np
import pytest

import hector_amd
from hector_amd import ensemble
from conftest import ROOT, SCENARIO

import os

ENV = "HECTOR_AMD_FAITHFUL_RETRIES"
SSP585 = os.path.join(ROOT, "hector_amd", "data", "ssp585.hxs")
OUTS = ["CO2_concentration", "global_tas", "sst", "land_tas", "timesteps"]
N = 96


def ensemble96():
    """test_gpu_step_control.py's members: S 1.5-6 x Q10 1.2-4."""
    S = np.repeat(np.linspace(1.5, 6.0, 12), 8)
    q10 = np.tile(np.linspace(1.2, 4.0, 8), 12)
    return S, q10


def sq(n):
    """n members spread evenly over the 96 (both ends of S and of Q10 included)."""
    S, q10 = ensemble96()
    if n == N:
        return S, q10
    idx = np.round(np.linspace(0, N - 1, n)).astype(int)
    return S[idx], q10[idx]


def fetch(c, outs, y1=2300):
    r = {v: c.fetchvars(v, (1745, y1)).copy() for v in outs}
    r["status"] = c.status().copy()
    return r


def run(lib, monkeypatch, mode, S, q10, outs=OUTS, scenario=SCENARIO, two_wave=False, setup=None, to=2300,
        nbp=False):
    """mode: "fast" | "env" (faithful by environment) | "rec" (faithful by recording solver_steps) |
    "count" (fast with solver_steps recorded: the executed steps)."""
    if mode == "env":
        monkeypatch.setenv(ENV, "1")
    elif mode == "count":
        monkeypatch.setenv(ENV, "0")
    else:
        monkeypatch.delenv(ENV, raising=False)
    rec = list(outs) + (["solver_steps"] if mode in ("rec", "count") else [])
    c = hector_amd.Core(scenario, len(S), lib_path=lib, allow_emulation=True)
    c.set_pair_kernel_limit(0)
    c.set_two_wave_from(1 if two_wave else 0)
    if setup:
        setup(c)
    c.setvar("S", S, "degC")
    if q10 is not None:
        c.setvar("q10_rh", q10, "(unitless)")
    c.set_outputs(rec)
    c.run(to)
    assert c.last_run_kernel() == ("run2" if two_wave else "run")
    # (nbp: the NBP-capable kernels are held to the faithful path whatever the mode, see CASES)
    assert c.last_run_retries() == (0 if mode in ("fast", "count") and not nbp else 1), mode
    r = fetch(c, rec, to)
    c.shutdown()
    monkeypatch.delenv(ENV, raising=False)
    return r


def same(a, b, outs, what):
    for v in list(outs) + ["status"]:
        assert np.array_equal(a[v], b[v], equal_nan=True), (what, v)


@pytest.fixture(scope="module")
def runs96(emul_lib):
    """The 96 members on both flavours and all four modes, once."""
    S, q10 = ensemble96()
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for two_wave in (False, True):
            for mode in ("fast", "env", "rec", "count"):
                out["run2" if two_wave else "run", mode] = run(emul_lib, mp, mode, S, q10, two_wave=two_wave)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_fast_path_equals_faithful_path(runs96, kernel):
    fast = runs96[kernel, "fast"]
    assert (fast["status"] == 0).all()
    for mode in ("env", "rec", "count"):
        same(fast, runs96[kernel, mode], OUTS, (kernel, mode))
    # the ensemble does spend years in reduced-timestep mode: 2 and 4 stashes a year occur
    assert set(np.unique(fast["timesteps"][1:]).astype(int)) >= {1, 2, 4}


@pytest.fixture(scope="module")
def oracle_steps96(oracle):
    """The oracle's solver_steps of all 96 members, once: [year][member]."""
    S, q10 = ensemble96()
    steps = []
    for i in range(N):
        p = oracle.default_params(); p.S = S[i]; p.q10_rh[0] = q10[i]
        o, err, _ = oracle.run(p)
        assert err == 0, i
        steps.append(o["solver_steps"])
    return np.array(steps).T


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_solver_steps_faithful_is_the_oracles_and_fast_is_fewer(runs96, oracle_steps96, kernel):
    rec, cnt = (runs96[kernel, m] for m in ("rec", "count"))
    ref = rec["solver_steps"][1:]
    assert np.array_equal(ref, oracle_steps96[1:])      # every member, every year
    got = cnt["solver_steps"][1:]
    assert (got <= ref).all()
    assert (got.mean(0) < ref.mean(0)).all()
    assert (got >= rec["timesteps"][1:]).all()      # at least one step a segment
    print("%s: steps per member-year faithful %.3f -> executed %.3f; costliest member %.3f -> %.3f"
          % (kernel, ref.mean(), got.mean(), ref.mean(0).max(), got.mean(0).max()))


def _biomes(c):
    names = ["b1", "b2", "b3", "b4"]
    c.split_biome(names, fveg_c=[0.1, 0.2, 0.3, 0.4], fdetritus_c=[0.4, 0.3, 0.2, 0.1],
                  fsoil_c=[0.25, 0.25, 0.3, 0.2], fpermafrost_c=[0.0, 0.1, 0.3, 0.6],
                  fnpp_flux0=[0.35, 0.3, 0.2, 0.15])
    n = c.n_members
    for b, nm in enumerate(names):
        c.setvar(nm + ".q10_rh", np.linspace(1.2 + 0.2 * b, 2.4 + 0.2 * b, n))
        c.setvar(nm + ".warmingfactor", np.full(n, 1.0 + 0.25 * b))


def _co2_con(c):
    years = np.arange(1850, 2101)
    c.setvar_dated("CO2_constrain", years, 280.0 + 0.9 * (years - 1850) + 0.004 * (years - 1850) ** 2, "ppmv CO2")


def _nbp_con(c):
    years = np.arange(1950, 2051)
    c.setvar_dated("NBP_constrain", years, 0.5 + 0.01 * (years - 1950))


def _nbp_con_biomes(c):
    _biomes(c)
    _nbp_con(c)


CASES = {
    # name: (members, q10 set?, outputs, scenario, setup, two-wave flavour)
    "four_unequal_biomes": (N, False, OUTS + ["veg_c", "permafrost_c"], SCENARIO, _biomes, False),
    "npp_rh_recorded": (N, True, OUTS + ["NPP", "RH"], SCENARIO, None, False),
    "co2_constrained": (12, True, OUTS + ["NBP"], SCENARIO, _co2_con, False),
    # The NBP constraint takes the six-variable solver (CON = 1).  The host holds those kernels to
    # the faithful path in every mode (EnsembleCore::run: on the GPU their two copies of a fresh
    # stepper's first right-hand side round differently, so the opening retry is not bit-identical
    # there).  What these cases show: the modes change nothing for such a run, step counts included,
    # on a kernel without the block (one biome), with it (two-wave flavour, four biomes).
    "nbp_constrained_one_wave": (12, True, OUTS + ["NBP"], SCENARIO, _nbp_con, False),
    "nbp_constrained": (12, True, OUTS + ["NBP"], SCENARIO, _nbp_con, True),
    "nbp_constrained_four_biomes": (12, False, OUTS + ["NBP", "veg_c"], SCENARIO, _nbp_con_biomes, False),
    "ssp585": (24, True, OUTS, SSP585, None, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fast_path_equals_faithful_path_on(emul_lib, monkeypatch, case):
    n, with_q10, outs, scenario, setup, two_wave = CASES[case]
    S, q10 = sq(n)
    nbp = case.startswith("nbp_constrained")
    kw = dict(outs=outs, scenario=scenario, setup=setup, two_wave=two_wave, nbp=nbp)
    fast = run(emul_lib, monkeypatch, "fast", S, q10 if with_q10 else None, **kw)
    # (the NBP constraint drives its warmest members out of mass balance late in the run: they are
    # flagged, on both paths alike -- same() compares the status words and the frozen outputs; more
    # than half of the members run clean to 2300)
    assert (fast["status"] == 0).sum() > (n // 2 if case.startswith("nbp_constrained") else n - 1)
    res = {mode: run(emul_lib, monkeypatch, mode, S, q10 if with_q10 else None, **kw)
           for mode in ("env", "rec", "count")}
    for mode, r in res.items():
        same(fast, r, outs, (case, mode))
    # the two paths really are two: this case's kernel has the opening block and its members retry
    # (a kernel left out of hx_open_retry_k would count the same steps on both)
    ref, got = res["rec"]["solver_steps"][1:], res["count"]["solver_steps"][1:]
    if nbp:
        assert np.array_equal(got, ref), case
    else:
        assert (got <= ref).all() and (got.sum(0) < ref.sum(0)).all(), case
    print("%s: steps per member-year faithful %.3f -> executed %.3f" % (case, ref.mean(), got.mean()))


def test_a_run_in_two_segments_equals_one_run(emul_lib, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    S, q10 = sq(24)
    one = run(emul_lib, monkeypatch, "fast", S, q10)
    c = hector_amd.Core(SCENARIO, 24, lib_path=emul_lib, allow_emulation=True)
    c.set_pair_kernel_limit(0)
    c.setvar("S", S, "degC").setvar("q10_rh", q10, "(unitless)")
    c.set_outputs(OUTS)
    c.run(2000)
    c.run(2300)
    same(one, fetch(c, OUTS), OUTS, "two segments")
    c.shutdown()


def test_reset_and_rerun_reproduces_the_output(emul_lib, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    S, q10 = sq(24)
    one = run(emul_lib, monkeypatch, "fast", S, q10)
    c = hector_amd.Core(SCENARIO, 24, lib_path=emul_lib, allow_emulation=True)
    c.set_pair_kernel_limit(0)
    c.setvar("S", S, "degC").setvar("q10_rh", q10, "(unitless)")
    c.enable_history(True)
    c.set_outputs(OUTS)
    c.run(2300)
    same(one, fetch(c, OUTS), OUTS, "with history")
    c.reset(1900)
    assert c.current_date == 1900
    c.run(2300)
    same(one, fetch(c, OUTS), OUTS, "reset to 1900")
    c.shutdown()


def test_runaway_member_has_the_same_status_on_both_paths(emul_lib, monkeypatch):
    """test_emulation_parity.py::test_model_errors_are_flags_not_crashes' member."""
    S = np.array([3.0, 3.0, 3.0]); npp = np.array([56.2, 1e5, 56.2])
    res = {}
    for mode in ("fast", "env", "rec"):
        res[mode] = run(emul_lib, monkeypatch, mode, S, None, outs=["CO2_concentration", "timesteps"],
                        setup=lambda c: c.setvar("npp_flux0", npp), to=1800)
    st = res["fast"]["status"]
    assert st[0] == 0 and st[2] == 0 and st[1] != 0
    for mode in ("env", "rec"):
        assert np.array_equal(res[mode]["status"], st), mode
        for i in (0, 2):
            assert np.array_equal(res[mode]["CO2_concentration"][:, i], res["fast"]["CO2_concentration"][:, i])
