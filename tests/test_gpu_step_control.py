"""The lock-step control around a dopri5 pass of the run kernels (solve_year, hx_dev_solver.h) on
the MI355X, on a wavefront that MIXES what the control has to tell apart.

One fixed ensemble of 96 members -- one full wavefront and a half-filled one, so padding lanes
exist -- with S on a grid from 1.5 to 6.0 and Q10 from 1.2 to 4.0, SSP2-4.5, on the run kernel
(`set_pair_kernel_limit(0)`): members of 3 to 5 passes a year, lanes that finish the year early,
rejecting lanes, members in reduced-timestep mode with retries, side by side.  The host emulation
runs one lane at a time and sees none of that.

 - every member against the oracle (CO2, Tgav at the project's tolerances; the stash schedule
   year by year; clean status words);
 - wave-mates do not matter: the same members in reversed order, in a seeded permutation and in
   the lane order of the parameter key give the same bits member by member -- what a control
   built on wave votes can break and a tolerance cannot see -- on the plain kernel and on the
   two-wave flavour;
 - the same bits as the build before the control was flattened (tests/golden/
   step_control_parent.npz, tools/make_step_control_golden.py).

(The runaway member -- a lane that must be flagged and taken out of the loop -- runs on the GPU's
run kernel in test_gpu_parity.py::test_runaway_member_is_flagged_and_does_not_hang_on_gpu.)"""
import os

import numpy as np
import pytest

import hector_amd
from conftest import ROOT, SCENARIO

pytestmark = pytest.mark.gpu

REL_CO2 = 2e-8
ABS_T = 2e-8
N = 96
OUTS = ["CO2_concentration", "global_tas", "timesteps", "solver_steps"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_control_parent.npz")


def ensemble96():
    S = np.repeat(np.linspace(1.5, 6.0, 12), 8)
    q10 = np.tile(np.linspace(1.2, 4.0, 8), 12)
    return S, q10


def _run(hip_lib, order, two_wave, sorting):
    """The ensemble with member order[i] in place i -> its outputs back in the ensemble's order."""
    S, q10 = ensemble96()
    c = hector_amd.Core(SCENARIO, N, device=0, lib_path=hip_lib)
    assert c.backend == "hip"
    c.set_pair_kernel_limit(0)
    c.set_two_wave_from(1 if two_wave else 0)
    c.set_member_sorting(sorting)
    c.setvar("S", S[order], "degC").setvar("q10_rh", q10[order], "(unitless)")
    c.set_outputs(OUTS)
    c.run(2300)
    assert c.last_run_kernel() == ("run2" if two_wave else "run")
    inv = np.argsort(order)
    res = {v: c.fetchvars(v, (1745, 2300))[:, inv].copy() for v in OUTS}
    res["status"] = c.status()[inv].copy()
    res["lanes"] = c.lane_of_member().copy()
    c.shutdown()
    return res


ORDERS = {"natural": np.arange(N), "reversed": np.arange(N)[::-1].copy(),
          "permuted": np.random.default_rng(20261018).permutation(N)}


@pytest.fixture(scope="module")
def runs(hip_lib):
    """Every arrangement once, shared by the tests below: (flavour, arrangement) -> outputs."""
    out = {}
    for two_wave in (False, True):
        k = "run2" if two_wave else "run"
        for name, order in ORDERS.items():
            out[k, name] = _run(hip_lib, order, two_wave, sorting=False)
        out[k, "sorted"] = _run(hip_lib, ORDERS["natural"], two_wave, sorting=True)
    return out


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


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_every_member_against_the_oracle(runs, oracle96, kernel):
    oco2, otg, ots = oracle96
    r = runs[kernel, "natural"]
    assert (r["status"] == 0).all()
    rel = np.abs(r["CO2_concentration"] - oco2) / oco2
    dt = np.abs(r["global_tas"] - otg)
    print("%s kernel, 96 members vs oracle: max rel dCO2 %.3e, max |dTgav| %.3e" % (kernel, rel.max(), dt.max()))
    assert rel.max() < REL_CO2
    assert dt.max() < ABS_T
    assert np.array_equal(r["timesteps"][1:], ots[1:])      # the stash schedule, year by year
    # the wavefronts do mix what the control tells apart: 1 to 4 stashes a year, 3 and more passes
    assert set(np.unique(ots[1:]).astype(int)) >= {1, 2, 4}
    steps = r["solver_steps"][1:]
    assert steps.min() <= 3 and steps.max() >= 5 and (steps.std(axis=1) > 0).any()


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_wave_mates_do_not_matter(runs, kernel):
    ref = runs[kernel, "natural"]
    assert (ref["status"] == 0).all()
    for name in ("reversed", "permuted", "sorted"):
        r = runs[kernel, name]
        for v in OUTS:
            assert np.array_equal(r[v], ref[v]), (kernel, name, v)
        assert (r["status"] == 0).all()
    # the arrangements are different lanes for the same member
    assert np.array_equal(runs[kernel, "natural"]["lanes"], np.arange(N))
    assert not np.array_equal(runs[kernel, "sorted"]["lanes"], np.arange(N))


def test_two_wave_flavour_takes_the_same_decisions(runs):
    a, b = runs["run", "natural"], runs["run2", "natural"]
    for v in ("timesteps", "solver_steps"):
        assert np.array_equal(a[v], b[v]), v


@pytest.mark.parametrize("kernel", ["run", "run2"])
def test_same_bits_as_the_build_before_the_change(runs, kernel):
    g = np.load(GOLDEN)
    S, q10 = ensemble96()
    assert np.array_equal(g["S"], S) and np.array_equal(g["q10"], q10)
    sfx = "" if kernel == "run" else "_run2"
    rows = [int(y) - 1745 for y in g["years"]]
    assert [int(y) for y in g["years"]] == [1850, 1950, 2000, 2050, 2100, 2150, 2200, 2300]
    r = runs[kernel, "sorted"]      # (the fixture was recorded with the default lane order)
    assert np.array_equal(r["CO2_concentration"][rows], g["co2" + sfx])
    assert np.array_equal(r["global_tas"][rows], g["tgav" + sfx])
    assert np.array_equal(r["solver_steps"][1:].sum(0).astype(np.int64), g["solver_steps" + sfx])
    assert np.array_equal(r["timesteps"][1:].sum(0).astype(np.int64), g["timesteps" + sfx])
