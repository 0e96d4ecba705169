"""Per-member input series on the device: 130 members (npad 192: three wavefronts, two real lanes
in the last), unsorted S, every kernel flavour of the run kernels against the oracle -- the
device build of upload_member_series() and of the kernels' reads behind the ms_mask bits.
(tests/test_member_series.py: the helpers, the inputs and the host-build tier.)"""
import numpy as np
import pytest

import test_member_series as ms
from test_member_series import ALL_FLAVOURS, BITWISE, END, FLAVOURS, Y0

pytestmark = pytest.mark.gpu

N = 130
GPU = dict(device=0)   # (no allow_emulation: make_core() asserts core.backend == "hip")


@pytest.mark.parametrize("flavour", ALL_FLAVOURS)
def test_five_emission_series_per_member_on_gpu(hip_lib, oracle, tmp_path, flavour):
    ms.check_flavour(hip_lib, oracle, tmp_path, flavour, N, GPU)


@pytest.mark.parametrize("flavour", ["run", "run2", "b4"])
def test_member_constraints_differ_on_gpu(hip_lib, oracle, tmp_path, flavour):
    ms.check_constraints(hip_lib, oracle, tmp_path, flavour, N, GPU)


@pytest.mark.parametrize("flavour", ["run", "run2"])
def test_values_at_the_scenario_ends_on_gpu(hip_lib, oracle, tmp_path, flavour):
    ms.check_edges(hip_lib, oracle, tmp_path, flavour, N, GPU)


def test_segments_on_gpu(hip_lib, oracle, tmp_path):
    ms.check_segments(hip_lib, oracle, tmp_path, N, GPU)


def test_series_set_after_a_run_with_history_on_gpu(hip_lib, oracle, tmp_path):
    ms.check_history_rerun(hip_lib, oracle, tmp_path, N, GPU)


def test_shared_value_after_member_series_on_gpu(hip_lib, oracle, tmp_path):
    ms.check_shared_after_members(hip_lib, oracle, tmp_path, N, GPU)


def test_series_follow_their_members_when_lanes_move_on_gpu(hip_lib, oracle, tmp_path, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_CALIBRATE_ALWAYS", "1")
    ms.check_lane_moves(hip_lib, oracle, tmp_path, N, GPU)


def test_member_series_next_to_member_gas_params_on_gpu(hip_lib, oracle, tmp_path):
    ms.check_with_gas_params(hip_lib, oracle, tmp_path, N, GPU)


def test_sharded_core_with_member_series_equals_one_core_on_gpu(hip_lib, monkeypatch):
    """Two shards of 65 members on one device (the rehearsal switch), the run kernel on both
    sides: each shard uploads its own members' columns of the five emission series."""
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    fl = FLAVOURS["run"]
    series = ms.emission_series(N)
    one = ms.make_core(hip_lib, fl, N, GPU, series=series)
    many = ms.make_core(hip_lib, fl, N, dict(devices=[0, 0]), series=series)
    assert one.backend == "hip" and many.backend == "hip"
    assert many.shards() == ([0, 0], [0, 65, 130])
    for c in (one, many):
        c.run(END)
        ms.assert_flavour(c, fl)
        assert (c.status() == 0).all()
    assert not np.array_equal(one.lane_of_member(), np.arange(N))
    for v in BITWISE:
        np.testing.assert_array_equal(one.fetchvars(v, (Y0, END)), many.fetchvars(v, (Y0, END)), err_msg=v)
    ms.assert_series_come_back(many, series, "sharded")
    for name, years, _ in series:
        np.testing.assert_array_equal(one.fetchvars(name, (years.min(), years.max())),
                                      many.fetchvars(name, (years.min(), years.max())), err_msg=name)
    one.shutdown(); many.shutdown()
