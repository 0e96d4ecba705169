"""The per-lane control of the stash and of the segment loop around it (stash(), solve_year() in
hx_dev_solver.h: decisions as selects on lane masks, hx_flat_stash) under host emulation.

The cases of stash_control_cases.py: the 96 members of test_gpu_step_control.py (S 1.5-6 x Q10
1.2-4) on the run kernel, SSP2-4.5 and SSP5-8.5, plain kernel, two-wave flavour and four biomes;
555 years of 96 members each.
Five further cases on SSP2-4.5 (per-member diffusivity, heat flux or NPP recorded; two-wave, two,
three and four biomes) run instantiations that DO take the flat form -- of the three above only
the plain one-biome kernel does (test_which_cases_run_the_flat_form).

 - every member against the oracle at the project's tolerances (2e-8 rel CO2, 2e-8 K), the stash
   schedule year by year, clean status words;
 - the oracle's own schedule does take every branch of the max_timestep controller in every case
   (years of 1, 2 and 3+ stashes; a halving; a doubling that re-arms the timeout; a doubling back
   to exactly 1; a wavefront's worth of members that differ in segment count within a year);
 - the same bits member by member in natural, reversed and permuted order;
 - the same bits as the commit before the change: tests/golden/stash_control_parent.npz
   (tools/make_stash_control_golden.py).  The golden's "gpu/" entries are that commit's GPU run:
   the stash schedule and the status words -- the decisions -- are held to them here, the floating-
   point outputs to its "emul/" entries, that commit's host emulation (the host compiler's
   arithmetic is not the GPU's bit for bit: the two halves of the golden differ in CO2 already);
 - the flag paths (HX_ERR_NEGPOOL, HX_ERR_MASS, a flagged member idling through its wave-mates'
   stashes) give the status words and outputs of the old form's host emulation.

(GPU twin: test_gpu_stash_control.py.)"""
import numpy as np
import pytest

import stash_control_cases as sc


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN)


@pytest.fixture(scope="module")
def oracles(oracle):
    """(scenario, one biome | four) -> the oracle's members, once.  (`oracle`: builds the library.)"""
    o = {(s, k): sc.oracle_case(s, k) for s in sc.SCENARIOS for k in ("run", "run_b4")}
    o.update({("ssp245", k): sc.oracle_case("ssp245", k) for k in sc.EXTRA if k not in ("b1_npp", "b4_npp")})
    o["ssp245", "b1_npp"], o["ssp245", "b4_npp"] = o["ssp245", "run"], o["ssp245", "run_b4"]   # (the same members)
    o.update({(s, "run2"): o[s, "run"] for s in sc.SCENARIOS})
    return o


@pytest.fixture(scope="module")
def runs(emul_lib):
    return {(s, k, o): sc.run_case(emul_lib, s, k, order, allow_emulation=True)
            for s, k in sc.CASES for o, order in sc.ORDERS.items()}


def _oracle_of(oracles, scen, kernel):
    return oracles[scen, kernel]


@pytest.mark.parametrize("scen,kernel", sc.CASES)
def test_every_member_against_the_oracle(runs, oracles, scen, kernel):
    o = _oracle_of(oracles, scen, kernel)
    missing = sc.COVERAGE - sc.coverage(o)
    assert not missing, (scen, kernel, missing)
    sc.check_against_oracle(runs[scen, kernel, "natural"], o, "emulation %s %s" % (scen, kernel))


@pytest.mark.parametrize("scen,kernel", sc.CASES)
def test_wave_mates_do_not_matter(runs, scen, kernel):
    ref = runs[scen, kernel, "natural"]
    for name in ("reversed", "permuted"):
        r = runs[scen, kernel, name]
        for v in sc.OUTS + ["status"]:
            assert np.array_equal(r[v], ref[v]), (scen, kernel, name, v)


@pytest.mark.parametrize("scen,kernel", sc.CASES)
def test_same_bits_as_the_commit_before_the_change(runs, golden, scen, kernel):
    assert np.array_equal(golden["S"], sc.ensemble96()[0]) and np.array_equal(golden["q10"], sc.ensemble96()[1])
    assert tuple(int(y) for y in golden["years"]) == sc.GOLDEN_YEARS
    r = runs[scen, kernel, "natural"]
    sc.check_against_golden(r, golden, "emul/%s/%s/" % (scen, kernel), (scen, kernel))
    # the decisions are the GPU's of that commit too
    g = "gpu/%s/%s/" % (scen, kernel)
    assert np.array_equal(golden[g + "timesteps"], r["timesteps"].astype(np.uint8))
    assert np.array_equal(golden[g + "status"], r["status"].astype(np.int64))


def test_which_cases_run_the_flat_form():
    """Of the issue's three kernels only the plain one-biome kernel takes the flat form; every
    further case and three of the four flag cases run an instantiation of hx_flat_stash."""
    assert [k for k in sc.KERNELS if sc.flat_stash(*sc.VARIANT[k])] == ["run"]
    assert all(sc.flat_stash(*sc.VARIANT[k]) for k in sc.EXTRA)
    families = {sc.VARIANT[k][0] for k in sc.EXTRA} | {sc.VARIANT["run"][0]}
    assert families == {1, 2, 3, 4, 101}
    assert {sc.VARIANT[k][3] for k in sc.EXTRA} >= {0, -2}
    assert [w for w in sc.FLAG_CASES if not sc.flat_stash(*sc.FLAG_VARIANT[w])] == ["mass"]
    assert sc.FLAG_VARIANT["mass_diff"][3] == 1 and sc.FLAG_VARIANT["runaway_nbp"][3] == 1


@pytest.mark.parametrize("which,bit", sorted(sc.FLAG_CASES.items()))
def test_flag_paths_as_in_the_old_form(emul_lib, golden, which, bit):
    r = sc.run_flag_case(emul_lib, which, allow_emulation=True)
    st = r["status"]
    assert (st & bit).any() and (st == 0).any(), st      # a member raises the flag, others run clean
    assert np.array_equal(st.astype(np.int64), golden["emul/flag_%s/status" % which])
    assert np.array_equal(st.astype(np.int64), golden["gpu/flag_%s/status" % which])
    for v in sc.FLAG_OUTS:
        assert sc.digest(r[v]) == str(golden["emul/flag_%s/%s_sha256" % (which, v)]), (which, v)
    ts = r["timesteps"][1:]
    clean = np.where(st == 0)[0]
    assert (ts[:, clean] >= 1).all()
    assert np.isfinite(r["CO2_concentration"]).all()


def test_flagged_member_does_not_touch_its_neighbours(emul_lib):
    r = sc.run_flag_case(emul_lib, "negpool", allow_emulation=True)
    for v in sc.FLAG_OUTS:
        assert np.array_equal(r[v][:, 0], r[v][:, 2]), v
