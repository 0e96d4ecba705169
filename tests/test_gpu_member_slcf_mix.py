"""Mixes of the aerosol and ozone / OH precursor emissions and the shipped SSPs as members of one
core, on the device: 130 members (npad 192: three wavefronts, two real lanes in the last), unsorted S
-- the device build of hx_slcf_mix_kernel and of the run kernels' guarded loads against the oracle and
against themselves bit for bit.  (tests/test_member_slcf_mix.py: the helpers, the inputs and the
host-build tier.)"""
import numpy as np
import pytest

import test_member_gas_mix as gm
import test_member_slcf_mix as sm
from test_member_mix import assert_equal_results
from test_member_series import END, FLAVOURS, Y0

pytestmark = pytest.mark.gpu

N = 130
GPU = dict(device=0)   # (no allow_emulation: make_core() asserts core.backend == "hip")


@pytest.mark.parametrize("flavour", ["run", "run2", "b4", "b9", "trk"])
def test_shipped_ssps_are_members_of_one_core_on_gpu(hip_lib, oracle, flavour):
    sm.check_ssp_members(hip_lib, flavour, N, GPU)


@pytest.mark.parametrize("name", sm.NAMES)
def test_each_name_alone_vs_oracle_on_gpu(hip_lib, oracle, tmp_path, name):
    sm.check_one_name(hip_lib, tmp_path, name, N, GPU)


def test_one_vector_at_the_scenario_ends_vs_oracle_on_gpu(hip_lib, oracle, tmp_path):
    sm.check_mixes_vs_oracle(hip_lib, tmp_path, "run", N, GPU, sm.edge_mixes(N), "edges")


@pytest.mark.parametrize("flavour", ["run", "run2", "b4"])
def test_identity_mixes_change_no_bit_on_gpu(hip_lib, flavour):
    sm.check_identity_mixes(hip_lib, flavour, N, GPU)


def test_results_do_not_depend_on_how_the_core_got_there_on_gpu(hip_lib):
    sm.check_invariances(hip_lib, N, GPU)


def test_refused_calls_change_nothing_on_gpu(hip_lib, tmp_path):
    sm.check_refusals(hip_lib, tmp_path, N, GPU)


def test_sharded_core_equals_one_core_on_gpu(hip_lib, monkeypatch):
    """Two shards of 65 members on one device (the rehearsal switch): each shard takes its members'
    columns of the coefficients and the whole basis -- for single mixes and for the shipped scenarios."""
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    fl = FLAVOURS["run"]
    ext = sm.kernel_of(fl)
    one = sm.straight_run(hip_lib, N, GPU)
    many = sm.slcf_core(hip_lib, fl, N, dict(devices=[0, 0]))
    assert many.backend == "hip" and many.shards() == ([0, 0], [0, 65, 130])
    sm.set_mixes(many, sm.standard_mixes(N))
    many.run(END)
    assert_equal_results(sm.result(many, ext), one, "sharded")
    many.shutdown()
    labels = gm.scenario_labels(N)
    res = []
    for kw in (GPU, dict(devices=[0, 0])):
        c = sm.slcf_core(hip_lib, fl, N, kw)
        assert c.setvar_scenarios(sm.SHIPPED, labels) > 14
        c.run(END)
        res.append(sm.result(c, ext))
        c.shutdown()
    assert (res[0]["status"] == 0).all()
    assert np.ptp(res[0]["RF_aci"][2100 - Y0]) > 0.01
    assert_equal_results(res[1], res[0], "scenarios, sharded")
