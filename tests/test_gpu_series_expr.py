"""hx_series_eval on the MI355X (Core.derive_expr): the bodies of tests/series_expr_cases.py on the
product library -- 300 members: two 256-lane blocks, the second with 44 real lanes and a partial
last wavefront; 46 rows, no multiple of a batch; rows behind the valid end.
"""
import pytest

import series_expr_cases as sc

pytestmark = pytest.mark.gpu
N = 300


@pytest.fixture(scope="module")
def core(hip_lib):
    """One core for the bodies that leave it as they found it (the model runs once)."""
    c = sc.make_core(N, hip_lib)
    assert c.backend == "hip"
    yield c
    c.shutdown()


def test_special_value_matrix_bit_for_bit_gpu(core):
    sc.check_special_values(core)
    assert core.series() == {}


def test_log_exp_against_longdouble_and_exact_specials_gpu(core):
    sc.check_log_exp(core)
    assert core.series() == {}


def test_every_op_on_model_data_gpu(hip_lib):
    c = sc.make_core(N, hip_lib)
    sc.check_model_data(c)
    c.shutdown()


def test_probabilities_of_an_indicator_series_gpu(core):
    sc.check_probabilities_of_an_indicator(core)
    core.drop_series("ind")


def test_program_edges_gpu(core):
    sc.check_program_edges(core)
    core.drop_series("z")


def test_lags_gpu(core):
    sc.check_lags(core)
    core.drop_series("z").drop_series("delta10")


def test_validity_and_rows_behind_it_gpu(hip_lib):
    sc.check_validity(hip_lib, N)


def test_store_rules_gpu(hip_lib):
    c = sc.make_core(N, hip_lib)
    sc.check_store_rules(c)
    c.shutdown()


def test_equals_derive_for_the_four_operations_gpu(core):
    sc.check_equals_derive(core)


def test_two_shards_on_one_device_give_the_one_shard_block_gpu(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    n = 2 * N + 3
    one, many = sc.make_core(n, hip_lib), sc.make_core(n, hip_lib, devices=[0, 0])
    sc.check_shards(one, many)
    one.shutdown()
    many.shutdown()


def test_refusals_gpu(hip_lib):
    c, fresh = sc.make_core(N, hip_lib), sc.make_core(N, hip_lib, run_to=0)
    sc.check_refusals(c, fresh)
    c.shutdown()
    fresh.shutdown()
