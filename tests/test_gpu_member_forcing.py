"""Per-member forcing efficacies (Core.enable_member_forcing) on the device: every kernel flavour
against the oracle with all seven names perturbed, a partial second wavefront, bitwise
independence of lane order, member sorting and shard layout, members that hold the scenario's own
values, and the summary verbs over the names and the derived forcings.  (tests/test_member_forcing.py:
the host-build tier, and the helpers.)"""
import numpy as np
import pytest

import hector_amd
from test_gpu_one_factor import GPU_FLAVOURS, N, SHUFFLE
from test_member_forcing import (FLAVOURS, NAMES, RUN_TO, UNITS, Y0, all_outputs, check_members_vs_oracle, draws,
                                 expect_kernel, forcing_core, own_values_identity, scenario_values, set_env)

pytestmark = pytest.mark.gpu


def base_values(hip_lib):
    return scenario_values(hip_lib, device=0)


@pytest.mark.parametrize("flavour", GPU_FLAVOURS)
def test_all_seven_per_member_on_every_flavour(hip_lib, tmp_path, monkeypatch, flavour):
    fl = FLAVOURS[flavour]
    set_env(monkeypatch, fl)
    vals, S = draws(base_values(hip_lib), N)
    c = forcing_core(hip_lib, fl, vals, S, device=0)
    expect_kernel(c, fl)
    check_members_vs_oracle(c, tmp_path, vals, S, fl["B"], flavour)


@pytest.mark.parametrize("flavour", ["run", "pair"])
def test_partial_second_wavefront(hip_lib, tmp_path, flavour):
    """70 members: the second wavefront's padding lanes take the last member's values."""
    fl = FLAVOURS[flavour]
    vals, S = draws(base_values(hip_lib), 70, seed=70)
    c = forcing_core(hip_lib, fl, vals, S, device=0)
    expect_kernel(c, fl)
    assert (c.status() == 0).all()
    check_members_vs_oracle(c, tmp_path, vals, S, 1, flavour + "-70")


@pytest.mark.parametrize("flavour", ["run", "run2", "pair", "b4"])
def test_shuffled_members_and_member_sorting_move_no_bit(hip_lib, flavour):
    fl = FLAVOURS[flavour]
    vals, S = draws(base_values(hip_lib), N)
    first = all_outputs(forcing_core(hip_lib, fl, vals, S, device=0), fl)
    c = forcing_core(hip_lib, fl, {k: v[SHUFFLE] for k, v in vals.items()}, S[SHUFFLE], device=0)
    expect_kernel(c, fl)
    again = all_outputs(c, fl)
    for v in first:   # (member i holds what member SHUFFLE[i] held)
        assert np.array_equal(again[v], first[v][:, SHUFFLE]), (flavour, "shuffled", v)
    u = forcing_core(hip_lib, fl, vals, S, run=False, device=0)
    u.set_member_sorting(False)
    u.run(RUN_TO)
    expect_kernel(u, fl)
    unsorted = all_outputs(u, fl)
    for v in first:
        assert np.array_equal(unsorted[v], first[v]), (flavour, "unsorted", v)


@pytest.mark.parametrize("flavour", ["run", "run2", "pair"])
def test_members_with_the_scenarios_own_values_have_the_bits_of_a_shared_core(hip_lib, monkeypatch, flavour):
    own_values_identity(hip_lib, monkeypatch, flavour, n=N, device=0)


def test_two_shards_on_one_device_equal_one_core(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_FLEET_REHEARSAL", "1")   # (two shards on one GPU)
    fl = FLAVOURS["run"]
    vals, S = draws(base_values(hip_lib), N)
    one = forcing_core(hip_lib, fl, vals, S, device=0)
    two = forcing_core(hip_lib, fl, vals, S, devices=[0, 0])
    for k in NAMES:
        assert np.array_equal(two.getvar(k), vals[k]), k
    a, b = all_outputs(one, fl), all_outputs(two, fl)
    for v in a:
        assert np.array_equal(a[v], b[v]), v
    assert np.array_equal(one.status(), two.status())


def test_summary_verbs_take_the_names_and_the_derived_forcings(hip_lib):
    fl = FLAVOURS["run"]
    vals, S = draws(base_values(hip_lib), N)
    c = forcing_core(hip_lib, fl, vals, S, device=0)
    a = c.moments("global_tas", [RUN_TO], against=["rho_so2", "delta_co2"])
    b = c.moments("global_tas", [RUN_TO], against=[vals["rho_so2"], vals["delta_co2"]])
    assert np.array_equal(a.sums, b.sums) and np.array_equal(a.shift, b.shift)
    assert np.array_equal(a.wsum, b.wsum) and np.array_equal(a.pshift, b.pshift)
    assert np.array_equal(a.src(), b.src()) and np.isfinite(a.src()).all()
    # the efficacies are felt: more CO2 efficacy, more warming; rho_so2 < 0 scaled up, less
    assert a.corr[0, 1] > 0
    probs = (0.05, 0.5, 0.95)
    for var in ("RF_CH4", "RF_N2O"):
        x = c.fetchvars(var, (2000, RUN_TO))
        assert np.ptp(x[-1]) > 0.01, var   # (the members' own delta_* reached the derived forcing)
        q = c.quantiles(var, probs, dates=(2000, RUN_TO))
        assert np.array_equal(q, np.quantile(x, probs, axis=1, method="inverted_cdf").T), var
