"""hx_member_score (Core.score): the misfit of every member against an observed record.

The definition fixes the order of every operation (include/hector_amd.h), in IEEE double without
fused multiply-add, so numpy -- a Python loop over the years, vectorised over the members, on
fetchvars output -- reproduces the device result bit for bit: no tolerance anywhere below.  The
kernel exchanges nothing between lanes, so the host-emulation build runs it faithfully (CPU part);
the same body runs on the GPU against the product library.
"""
import glob
import os
import re

import numpy as np
import pytest

import hector_amd
from conftest import ROOT

RUN_TO = 2100
VARS = ("CO2_concentration", "global_tas")


def _params(n):
    u = (np.arange(n) + 0.5) / n
    S = 1.5 + 4.5 * u
    q10 = 1.0 + 2.0 * np.fmod(np.arange(n) * 0.6180339887498949, 1.0)
    beta = 0.1 + 0.8 * np.fmod(np.arange(n) * 0.7548776662466927, 1.0)
    return S, q10, beta


def _core(n, lib, **kw):
    if lib is None:
        c = hector_amd.Core(n_members=n, device=0, **kw)
    else:
        c = hector_amd.Core(n_members=n, lib_path=lib, allow_emulation=True, **kw)
    S, q10, beta = _params(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10).setvar("beta", beta)
    return c


def numpy_score(x, y0, years, obs, sigma, baseline):
    """The exact sequence of include/hector_amd.h on x[year - y0, member]."""
    n = x.shape[1]
    base = None
    if baseline is not None:
        s = np.zeros(n)
        for y in range(baseline[0], baseline[1] + 1):
            s = s + x[y - y0]
        base = s / float(baseline[1] - baseline[0] + 1)
    chi = np.zeros(n)
    used = 0
    for i, y in enumerate(years):
        if np.isnan(obs[i]):
            continue
        used += 1
        r = (x[y - y0] - base) - obs[i] if base is not None else x[y - y0] - obs[i]
        if sigma is not None:
            r = r / sigma[i]
        r2 = r * r
        chi = chi + r2
    return chi, used


def _cases(rng):
    years = np.arange(1850, 2015)
    rng.shuffle(years)                      # out of order
    obs_co2 = 280.0 + 0.6 * (years - 1850) + rng.normal(0, 2.0, years.size)
    obs_tas = 0.006 * (years - 1850) + rng.normal(0, 0.1, years.size)
    for o in (obs_co2, obs_tas):
        o[rng.choice(years.size, 17, replace=False)] = np.nan
    sig_co2 = 0.5 + rng.random(years.size)
    sig_tas = 0.05 + 0.1 * rng.random(years.size)
    return years, {"CO2_concentration": (obs_co2, sig_co2), "global_tas": (obs_tas, sig_tas)}


def _check_scores(core):
    rng = np.random.default_rng(20251016)
    years, cases = _cases(rng)
    y0 = core.strtdate
    for var in VARS:
        x = core.fetchvars(var, (y0, RUN_TO))
        obs, sig = cases[var]
        for sigma in (None, sig):
            for baseline in (None, (1850, 1900)):
                got, used = core.score(var, years, obs, sigma=sigma, baseline=baseline, return_used=True)
                ref, ref_used = numpy_score(x, y0, years, obs, sigma, baseline)
                assert used == ref_used == years.size - 17
                assert got.shape == (core.n_members,) and np.isfinite(got).all()
                assert np.array_equal(got, ref), (var, sigma is not None, baseline,
                                                  np.abs(got - ref).max())
    # one year, the first and the last recorded one
    for y in (y0, RUN_TO):
        x = core.fetchvars("global_tas", (y, y))
        got = core.score("global_tas", [y], [0.25])
        assert np.array_equal(got, (x[0] - 0.25) * (x[0] - 0.25))
    return years, cases


def _check_errors(core):
    with pytest.raises(hector_amd.HectorAmdError, match="not enabled"):
        core.score("RF_tot", [1900], [1.0])
    with pytest.raises(hector_amd.HectorAmdError, match="current date"):
        core.score("global_tas", [1900, RUN_TO + 1], [1.0, 1.0])
    with pytest.raises(hector_amd.HectorAmdError, match="reference period"):
        core.score("global_tas", [1900], [1.0], baseline=(1850, RUN_TO + 1))
    with pytest.raises(hector_amd.HectorAmdError, match="n < 1"):
        core.score("global_tas", [], [])
    # the failed calls left the core as it was
    assert core.current_date == RUN_TO


def _body(n, lib):
    core = _core(n, lib)
    core.run(RUN_TO)
    before = {v: core.fetchvars(v, (core.strtdate, RUN_TO)) for v in VARS}
    status, ms = core.status(), core.last_run_ms()
    years, cases = _check_scores(core)
    _check_errors(core)
    # scoring reads results: it changes none of them
    for v in VARS:
        assert np.array_equal(before[v], core.fetchvars(v, (core.strtdate, RUN_TO)))
    assert np.array_equal(status, core.status()) and core.last_run_ms() == ms
    obs, sig = cases["global_tas"]
    sorted_score = core.score("global_tas", years, obs, sigma=sig, baseline=(1850, 1900))
    core.shutdown()
    # another lane order, the same members: the same bits
    plain = _core(n, lib)
    plain.set_member_sorting(False)
    plain.run(RUN_TO)
    assert np.array_equal(plain.lane_of_member(), np.arange(n))
    x = plain.fetchvars("global_tas", (plain.strtdate, RUN_TO))
    got = plain.score("global_tas", years, obs, sigma=sig, baseline=(1850, 1900))
    assert np.array_equal(got, numpy_score(x, plain.strtdate, years, obs, sig, (1850, 1900))[0])
    if np.array_equal(x, before["global_tas"]):   # (the trajectories themselves agree bit for bit)
        assert np.array_equal(got, sorted_score)
    plain.shutdown()


def test_score_equals_numpy_bit_for_bit_in_the_emulation(emul_lib):
    _body(200, emul_lib)


@pytest.mark.gpu
def test_score_equals_numpy_bit_for_bit_on_the_gpu(hip_lib):
    _body(4096 + 37, None)


def test_sharded_core_scores_equal_the_single_core(emul_lib):
    n = 11   # 4 + 4 + 3
    one = _core(n, emul_lib)
    many = _core(n, emul_lib, devices=[0, 0, 0])
    rng = np.random.default_rng(7)
    years, cases = _cases(rng)
    for c in (one, many):
        c.run(2020)
    for var in VARS:
        obs, sig = cases[var]
        a, ua = one.score(var, years, obs, sigma=sig, baseline=(1850, 1900), return_used=True)
        b, ub = many.score(var, years, obs, sigma=sig, baseline=(1850, 1900), return_used=True)
        assert ua == ub and np.array_equal(a, b)
        assert np.array_equal(one.score(var, years, obs), many.score(var, years, obs))
    with pytest.raises(hector_amd.HectorAmdError, match="current date"):
        many.score("global_tas", [2021], [1.0])
    assert np.array_equal(one.status(), many.status())   # the refused call poisoned nothing
    one.shutdown(); many.shutdown()


def test_quantiles_are_refused_in_the_emulation(emul_lib):
    """The quantile kernels are cooperative (LDS atomics, cross-lane): one lane at a time cannot run
    them, and the emulation says so instead of returning numbers."""
    one = _core(5, emul_lib)
    many = _core(5, emul_lib, devices=[0, 0])
    for c in (one, many):
        c.run(1760)
        with pytest.raises(hector_amd.HectorAmdError, match="not available in the host-emulation build"):
            c.quantiles("global_tas", [0.5])
        assert np.isfinite(c.fetchvars("global_tas", (1745, 1760))).all()
        c.shutdown()


def test_score_kernel_has_no_contracted_multiply_add():
    """fp contraction is off for the score kernel: r * r and chi + r2 are a v_mul_f64 and a v_add_f64.
    gfx950 has no fp64 divide instruction; the compiler's correctly rounded expansion of the two
    divisions (v_div_scale .. v_div_fmas, v_div_fixup) holds the only fused multiply-adds, all of
    them ahead of the v_div_fmas of their division."""
    files = glob.glob(os.path.join(ROOT, "hector_amd", "build", "hx_post-hip-amdgcn-amd-amdhsa-gfx950.s"))
    if not files:
        pytest.skip("no assembly in hector_amd/build (the library was not built in this tree)")
    text = open(files[0], errors="replace").read()
    k = text.index("_Z15hx_score_kernel")
    k = text.index("\n", text.index("_Z15hx_score_kernel", k + 1))   # the label, not the .globl line
    body = text[k:text.index(".Lfunc_end", k)]
    ops = re.findall(r"^\s+(v_\w+_f64\w*)", body, flags=re.M)
    assert "v_mul_f64" in ops and "v_add_f64" in ops
    in_div = False
    for op in ops:
        if op.startswith("v_div_scale"):
            in_div = True
        elif op.startswith("v_div_fmas") or op.startswith("v_div_fixup"):
            in_div = False
        elif op.startswith("v_fma") or op.startswith("v_mac") or op.startswith("v_pk_fma"):
            assert in_div, "a fused multiply-add outside a division: %r" % ops
    assert sum(o.startswith("v_div_fixup") for o in ops) == 2
