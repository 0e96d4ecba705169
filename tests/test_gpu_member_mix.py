"""Per-member input series as mixes on the device: 130 members (npad 192: three wavefronts, two
real lanes in the last), unsorted S -- the device build of hx_mseries_mix_kernel and of prepare()'s
replay of the recipe, against the dense path bit for bit.  (tests/test_member_mix.py: the helpers,
the inputs and the host-build tier.)"""
import numpy as np
import pytest

import test_member_mix as mm
from test_member_mix import assert_equal_results, reference, result, set_mixes, standard_mixes
from test_member_series import END, FLAVOURS, UNIT, Y0, make_core, member_S, set_series

pytestmark = pytest.mark.gpu

N = 130
GPU = dict(device=0)   # (no allow_emulation: make_core() asserts core.backend == "hip")


@pytest.mark.parametrize("flavour", ["run", "run2", "b4"])
def test_mix_equals_the_dense_path_on_gpu(hip_lib, flavour):
    mm.check_equality(hip_lib, flavour, N, GPU)


def test_products_are_added_in_ascending_k_on_gpu(hip_lib):
    mm.check_order(hip_lib, N, GPU)


def test_one_vector_at_the_scenario_ends_on_gpu(hip_lib):
    mm.check_edges(hip_lib, N, GPU)


def test_recipe_is_replayed_when_lanes_move_on_gpu(hip_lib, monkeypatch):
    """Run, then another S for every member (the parameter key and the measured cost both order
    the lanes anew), reset, run: the table is built again in the new lane order, like the dense
    core's that is taken through the same steps."""
    monkeypatch.setenv("HECTOR_AMD_CALIBRATE_ALWAYS", "1")
    fl = FLAVOURS["run"]
    mixes = standard_mixes(N)
    S2 = member_S(N)[::-1].copy()
    res = []
    for how in ("mix", "dense"):
        c = make_core(hip_lib, fl, N, GPU)
        if how == "mix":
            set_mixes(c, mixes)
        else:
            set_series(c, mm.as_dense(mixes))
        c.run(END)
        lane0 = c.lane_of_member().copy()
        first = result(c, fl)
        if how == "mix":
            assert_equal_results(first, reference(hip_lib, "run", N, GPU, "std", mixes, "mix"), "first run")
        c.setvar("S", S2, "degC")
        c.reset(Y0)
        c.run(END)
        assert not np.array_equal(lane0, c.lane_of_member()), how
        res.append(result(c, fl))
        assert not np.array_equal(res[-1]["global_tas"], first["global_tas"])
        c.shutdown()
    assert (res[1]["status"] == 0).all()
    assert_equal_results(res[0], res[1], "after the lanes moved")


def test_new_coefficients_for_the_same_years_and_basis_on_gpu(hip_lib):
    """Three successive mixes that differ in their coefficients alone, each followed by reset and
    run: the last equals a fresh core given only the last mix."""
    fl = FLAVOURS["run"]
    last = standard_mixes(N)
    c = make_core(hip_lib, fl, N, GPU)
    seen = []
    for seed in (101, 102, None):
        rng = np.random.default_rng(seed)
        for name, years, basis, coeff in last:
            w = coeff if seed is None else coeff * rng.uniform(0.97, 1.03, coeff.shape)
            c.setvar_dated_mix(name, years, basis, w, UNIT[name])
        c.reset(Y0)
        c.run(END)
        seen.append(result(c, fl))
    assert not np.array_equal(seen[0]["CO2_concentration"], seen[1]["CO2_concentration"])
    assert not np.array_equal(seen[1]["CO2_concentration"], seen[2]["CO2_concentration"])
    assert_equal_results(seen[2], reference(hip_lib, "run", N, GPU, "std", last, "mix"), "third set of coefficients")
    c.shutdown()


def test_sharded_core_with_mixes_equals_one_core_on_gpu(hip_lib, monkeypatch):
    """Two shards of 65 members on one device (the rehearsal switch): each shard takes its members'
    columns of coeff and the whole basis."""
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")
    fl = FLAVOURS["run"]
    mixes = standard_mixes(N)
    one = reference(hip_lib, "run", N, GPU, "std", mixes, "mix")
    many = make_core(hip_lib, fl, N, dict(devices=[0, 0]))
    assert many.backend == "hip" and many.shards() == ([0, 0], [0, 65, 130])
    set_mixes(many, mixes)
    many.run(END)
    assert_equal_results(result(many, fl), one, "sharded")
    # a refused call leaves every shard as it was: the fault lies in the second shard's columns
    name, years, basis, coeff = mixes[0]
    bad = coeff.copy()
    bad[1, N - 1] = np.nan
    with pytest.raises(mm.Error, match="hx_setvar_dated_mix: .*finite"):
        many.setvar_dated_mix(name, years[:5], basis[:, :5], bad, UNIT[name])
    assert np.array_equal(many.fetchvars(name, (Y0, END)), one["in:" + name])
    many.shutdown()
