"""The per-lane control of the stash and of the segment loop around it (stash(), solve_year() in
hx_dev_solver.h: decisions as selects on lane masks, hx_flat_stash) on the MI355X, on wavefronts
that MIX what the control has to tell apart -- the host emulation runs one lane at a time.

The cases of stash_control_cases.py: the 96 members of test_gpu_step_control.py (S 1.5-6 x Q10
1.2-4: one full wavefront and a half-filled one) on the run kernel, SSP2-4.5 and SSP5-8.5, plain
kernel, two-wave flavour and four biomes; 555 years of 96 members each.
Five further cases on SSP2-4.5 (per-member diffusivity, heat flux or NPP recorded; two-wave, two,
three and four biomes) run instantiations that DO take the flat form -- of the three above only
the plain one-biome kernel does (test_which_cases_run_the_flat_form).

 - every member against the oracle at the project's tolerances (2e-8 rel CO2, 2e-8 K), the stash
   schedule year by year, clean status words;
 - the oracle's own schedule takes every branch of the max_timestep controller in every case, and
   the first wavefront mixes lanes of different segment counts within a year;
 - the same bits member by member in natural, reversed and permuted lane order;
 - np.array_equal with the GPU run of the commit before the change (tests/golden/
   stash_control_parent.npz, tools/make_stash_control_golden.py): CO2, tas, sst, land_tas, the
   stash counts of every year and the status words;
 - the flag paths (HX_ERR_NEGPOOL, HX_ERR_MASS, a flagged member idling through its wave-mates'
   stashes): the status words of the old form, on the GPU and under host emulation.

(Host twin: test_stash_control_emulation.py.)"""
import numpy as np
import pytest

import stash_control_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN)


@pytest.fixture(scope="module")
def oracles(oracle):
    o = {(s, k): sc.oracle_case(s, k) for s in sc.SCENARIOS for k in ("run", "run_b4")}
    o.update({("ssp245", k): sc.oracle_case("ssp245", k) for k in sc.EXTRA if k not in ("b1_npp", "b4_npp")})
    o["ssp245", "b1_npp"], o["ssp245", "b4_npp"] = o["ssp245", "run"], o["ssp245", "run_b4"]   # (the same members)
    o.update({(s, "run2"): o[s, "run"] for s in sc.SCENARIOS})
    return o


@pytest.fixture(scope="module")
def runs(hip_lib):
    return {(s, k, o): sc.run_case(hip_lib, s, k, order, device=0)
            for s, k in sc.CASES for o, order in sc.ORDERS.items()}


@pytest.mark.parametrize("scen,kernel", sc.CASES)
def test_every_member_against_the_oracle(runs, oracles, scen, kernel):
    o = oracles[scen, kernel]
    missing = sc.COVERAGE - sc.coverage(o)
    assert not missing, (scen, kernel, missing)
    sc.check_against_oracle(runs[scen, kernel, "natural"], o, "gpu %s %s" % (scen, kernel))


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
    sc.check_against_golden(runs[scen, kernel, "natural"], golden, "gpu/%s/%s/" % (scen, kernel), (scen, kernel))


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
def test_flag_paths_as_in_the_old_form(hip_lib, golden, which, bit):
    r = sc.run_flag_case(hip_lib, which, device=0)
    st = r["status"]
    assert (st & bit).any() and (st == 0).any(), st      # a member raises the flag, others run clean
    assert np.array_equal(st.astype(np.int64), golden["emul/flag_%s/status" % which])
    assert np.array_equal(st.astype(np.int64), golden["gpu/flag_%s/status" % which])
    for v in sc.FLAG_OUTS:
        assert sc.digest(r[v]) == str(golden["gpu/flag_%s/%s_sha256" % (which, v)]), (which, v)
    clean = np.where(st == 0)[0]
    assert (r["timesteps"][1:][:, clean] >= 1).all()     # they stash on beside the flagged member
    assert np.isfinite(r["CO2_concentration"]).all()
    if which in ("negpool", "runaway_nbp"):
        for v in sc.FLAG_OUTS:
            assert np.array_equal(r[v][:, 0], r[v][:, 2]), v
