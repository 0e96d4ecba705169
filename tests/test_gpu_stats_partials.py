"""Ensemble statistics from the run kernel's per-wavefront partials (hx_wave_partials,
hx_combine_partials_kernel) against the second pass over the rows (hx_stats_kernel,
HECTOR_AMD_STATS_PARTIALS=0) and against math.fsum.

130 members on the plain run kernel: three wavefronts, two full and one with 2 live and 62 padded
lanes.  1745-2300: 556 rows, 17 tiles of 32 and a remainder of 12.

Bounds (eps = 2^-52): two summation orders of n fp64 terms differ by at most 2 (n - 1) eps sum|x|,
each lies within (n - 1) eps sum|x| of the exact sum; count, min and max are order-free: bitwise.
"""
import math
import os

import numpy as np
import pytest

import hector_amd
from hector_amd import ensemble
from conftest import SCENARIO

pytestmark = pytest.mark.gpu

N = 130
Y0, Y1 = 1745, 2300
VARS = ["CO2_concentration", "global_tas"]
EPS = 2.0 ** -52


def _core(hip_lib, outputs=None, biomes=None, two_wave=False, beta=None):
    S, q10 = ensemble.ecs_q10(N)
    c = hector_amd.Core(SCENARIO, N, device=0, lib_path=hip_lib)
    c.set_pair_kernel_limit(0)          # the plain run kernel (HECTOR_AMD_PAIR_MAX_MEMBERS=0)
    if two_wave:
        c.set_two_wave_from(1)          # (HECTOR_AMD_TWO_WAVE_FROM=1)
    if biomes:
        c.split_biome(biomes)
    c.setvar("S", S, "degC")
    if not biomes:
        c.setvar("q10_rh", q10)
    if beta is not None:
        c.setvar("beta", [beta])
    if outputs:
        c.set_outputs(outputs)
    return c


def _stats(c, variables, y0, y1, partials=True):
    """[variable][year][5] through hx_ensemble_stats; partials=False: HECTOR_AMD_STATS_PARTIALS=0."""
    old = os.environ.get("HECTOR_AMD_STATS_PARTIALS")
    if not partials:
        os.environ["HECTOR_AMD_STATS_PARTIALS"] = "0"
    try:
        return np.array(c.ensemble_stats(list(variables), (y0, y1)))
    finally:
        if not partials:
            if old is None:
                del os.environ["HECTOR_AMD_STATS_PARTIALS"]
            else:
                os.environ["HECTOR_AMD_STATS_PARTIALS"] = old


def _exact(c, var, y0, y1):
    """-> (fsum x, fsum x^2, fsum |x|) per year over the members, from fetchvars."""
    x = c.fetchvars(var, (y0, y1))
    s = np.array([math.fsum(r) for r in x])
    q = np.array([math.fsum(r * r) for r in x])
    a = np.array([math.fsum(np.abs(r)) for r in x])
    return x, s, q, a


def _check_against_exact(st, c, var, y0, y1):
    x, s, q, a = _exact(c, var, y0, y1)
    n = x.shape[1]
    np.testing.assert_array_equal(st[:, 0], np.full(len(s), float(n)))
    np.testing.assert_array_equal(st[:, 3], x.min(1))
    np.testing.assert_array_equal(st[:, 4], x.max(1))
    ds, dq = np.abs(st[:, 1] - s), np.abs(st[:, 2] - q)
    print("%s %d-%d: max |sum - fsum| / bound %.3f, sumsq %.3f" %
          (var, y0, y1, (ds / ((n - 1) * EPS * a + 1e-300)).max(), (dq / ((n - 1) * EPS * q + 1e-300)).max()))
    assert (ds <= (n - 1) * EPS * a).all()
    assert (dq <= (n - 1) * EPS * q).all()
    return a, q


@pytest.fixture(scope="module")
def base(hip_lib):
    """One complete run on the plain kernel; read only."""
    c = _core(hip_lib)
    c.run(Y1)
    assert c.last_run_kernel() == "run" and c.last_run_variant() == 0
    assert len(c.wave_epilogue_clock()) == 3      # the launch wrote partials, three wavefronts
    assert (c.status() == 0).all()
    yield c
    c.shutdown()


@pytest.fixture(scope="module")
def base_stats(base):
    return _stats(base, VARS, Y0, Y1)


def test_partials_against_second_pass_and_fsum(base, base_stats):
    fb = _stats(base, VARS, Y0, Y1, partials=False)
    for k, v in enumerate(VARS):
        a, q = _check_against_exact(base_stats[k], base, v, Y0, Y1)
        _check_against_exact(fb[k], base, v, Y0, Y1)
        for col in (0, 3, 4):
            np.testing.assert_array_equal(base_stats[k][:, col], fb[k][:, col])
        assert (np.abs(base_stats[k][:, 1] - fb[k][:, 1]) <= 2 * (N - 1) * EPS * a).all()
        assert (np.abs(base_stats[k][:, 2] - fb[k][:, 2]) <= 2 * (N - 1) * EPS * q).all()


@pytest.mark.parametrize("y0,y1", [(1745, 2300), (1745, 1745), (1800, 1850), (2300, 2300)])
def test_ranges(base, base_stats, y0, y1):
    st = _stats(base, VARS, y0, y1)
    np.testing.assert_array_equal(st, base_stats[:, y0 - Y0:y1 - Y0 + 1])     # a row's bits: its own
    for k, v in enumerate(VARS):
        _check_against_exact(st[k], base, v, y0, y1)
    one = _stats(base, VARS[1:], y0, y1)                                       # one variable a launch
    np.testing.assert_array_equal(one[0], st[1])


def test_segmented_run_and_rerun_after_reset(hip_lib, base_stats):
    c = _core(hip_lib)
    c.run(2000)
    np.testing.assert_array_equal(_stats(c, VARS, Y0, 2000), base_stats[:, :2000 - Y0 + 1])
    c.run(Y1)                       # block boundaries fall elsewhere, iy_from != 0
    assert len(c.wave_epilogue_clock()) == 3
    np.testing.assert_array_equal(_stats(c, VARS, Y0, Y1), base_stats)
    c.reset(Y0)
    c.run(Y1)
    np.testing.assert_array_equal(_stats(c, VARS, Y0, Y1), base_stats)
    c.shutdown()


def test_fallback_other_variable(base):
    np.testing.assert_array_equal(_stats(base, ["sst"], Y0, Y1), _stats(base, ["sst"], Y0, Y1, partials=False))
    mixed = _stats(base, ["sst", "global_tas"], Y0, Y1)
    np.testing.assert_array_equal(mixed[1], _stats(base, ["global_tas"], Y0, Y1)[0])


@pytest.mark.parametrize("kind", ["npp", "four_biomes", "two_wave"])
def test_fallback_other_kernel_flavours(hip_lib, kind):
    if kind == "npp":
        c = _core(hip_lib, outputs=VARS + ["NPP"])
    elif kind == "four_biomes":
        c = _core(hip_lib, biomes=["b1", "b2", "b3", "b4"])
    else:
        c = _core(hip_lib, two_wave=True)
    c.run(Y1)
    assert c.last_run_kernel() == ("run2" if kind == "two_wave" else "run")
    assert len(c.wave_epilogue_clock()) == 0      # no partials from this flavour
    st = _stats(c, VARS, Y0, Y1)
    np.testing.assert_array_equal(st, _stats(c, VARS, Y0, Y1, partials=False))
    for k, v in enumerate(VARS):
        _check_against_exact(st[k], c, v, Y0, Y1)
    c.shutdown()


def test_stale_partials_are_not_used(hip_lib, base_stats):
    c = _core(hip_lib)
    c.run(Y1)
    np.testing.assert_array_equal(_stats(c, VARS, Y0, Y1), base_stats)
    c.set_outputs(VARS + ["NPP"])    # another flavour writes the rows from here on
    c.setvar("beta", [0.5])          # ... and other values
    c.run(Y1)
    assert len(c.wave_epilogue_clock()) == 0
    st = _stats(c, VARS, Y0, Y1)
    np.testing.assert_array_equal(st, _stats(c, VARS, Y0, Y1, partials=False))
    assert not np.array_equal(st[:, :, 1], base_stats[:, :, 1])
    for k, v in enumerate(VARS):
        _check_against_exact(st[k], c, v, Y0, Y1)
    c.shutdown()


@pytest.mark.parametrize("skip", [1, 3])
def test_skipped_wavefronts(hip_lib, base_stats, monkeypatch, skip):
    monkeypatch.setenv("HECTOR_AMD_STATS_SKIP_WAVES", str(skip))
    c = _core(hip_lib)
    c.run(Y1)
    clk = c.wave_epilogue_clock()
    assert len(clk) == 3 and (clk[:skip] == 0).all() and (clk[skip:] > 0).all()
    st = _stats(c, VARS, Y0, Y1)
    for k, v in enumerate(VARS):
        a, q = _check_against_exact(st[k], c, v, Y0, Y1)
        for col in (0, 3, 4):
            np.testing.assert_array_equal(st[k][:, col], base_stats[k][:, col])
        assert (np.abs(st[k][:, 1] - base_stats[k][:, 1]) <= 2 * (N - 1) * EPS * a).all()
        assert (np.abs(st[k][:, 2] - base_stats[k][:, 2]) <= 2 * (N - 1) * EPS * q).all()
    c.shutdown()


def test_stats_device_and_ensemble_stats_agree(base, base_stats):
    import torch
    for k, v in enumerate(VARS):
        d = torch.zeros((Y1 - Y0 + 1, 5), dtype=torch.float64, device="cuda:0")
        base.stats_device(v, Y0, Y1, d.data_ptr())
        np.testing.assert_array_equal(d.cpu().numpy(), base_stats[k])
