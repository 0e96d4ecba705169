"""Mixes of the gas pre-pass's inputs and whole scenarios as members, on the device: 130 members
(npad 192: three wavefronts, two real lanes in the last), unsorted S -- the device build of
hx_gas_mix_kernel against the oracle and against itself bit for bit.  (tests/test_member_gas_mix.py:
the helpers, the inputs and the host-build tier.)"""
import numpy as np
import pytest

import test_member_gas_mix as gm
from test_member_mix import assert_equal_results
from test_member_series import END, FLAVOURS, Y0

pytestmark = pytest.mark.gpu

N = 130
GPU = dict(device=0)   # (no allow_emulation: make_core() asserts core.backend == "hip")


@pytest.fixture(scope="module")
def scen_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("reduced_scenarios")


@pytest.mark.parametrize("flavour", ["run", "run2", "b4", "b9"])
def test_scenario_members_equal_their_scenarios_on_gpu(hip_lib, oracle, scen_dir, flavour):
    gm.check_scenario_members(hip_lib, scen_dir, flavour, N, GPU)


@pytest.mark.parametrize("name", gm.NEW_NAMES)
def test_each_name_alone_vs_oracle_on_gpu(hip_lib, oracle, tmp_path, name):
    gm.check_one_name(hip_lib, tmp_path, name, N, GPU)


def test_one_vector_at_the_scenario_ends_vs_oracle_on_gpu(hip_lib, oracle, tmp_path):
    gm.check_mixes_vs_oracle(hip_lib, tmp_path, "run", N, GPU, gm.edge_mixes(N), "edges")


def test_results_do_not_depend_on_how_the_core_got_there_on_gpu(hip_lib):
    gm.check_invariances(hip_lib, N, GPU)


def test_sharded_core_equals_one_core_on_gpu(hip_lib, scen_dir, monkeypatch):
    """Two shards of 65 members on one device (the rehearsal switch): each shard takes its members'
    columns of the coefficients and the whole basis -- for single mixes and for whole scenarios."""
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    fl = FLAVOURS["run"]
    one = gm.straight_run(hip_lib, N, GPU)
    many = gm.gas_core(hip_lib, fl, N, dict(devices=[0, 0]))
    assert many.backend == "hip" and many.shards() == ([0, 0], [0, 65, 130])
    gm.set_mixes(many, gm.standard_mixes(N))
    many.run(END)
    assert_equal_results(gm.result(many, fl), one, "sharded")
    many.shutdown()
    paths, labels = gm.reduced_scenarios(scen_dir), gm.scenario_labels(N)
    res = []
    for kw in (GPU, dict(devices=[0, 0])):
        c = gm.gas_core(hip_lib, fl, N, kw)
        assert c.setvar_scenarios(paths, labels) > 7
        c.run(END)
        res.append(gm.result(c, fl))
        c.shutdown()
    assert (res[0]["status"] == 0).all()
    assert np.ptp(res[0]["N2O_concentration"][2100 - Y0]) > 1.0
    assert_equal_results(res[1], res[0], "scenarios, sharded")
