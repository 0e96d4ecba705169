"""hx_series_rank / hx_metric_ranks / hx_ensemble_crps (Core.rank_series, Core.metric_ranks,
Core.crps, Core.spearman) and their numpy restatements hector_amd.ensemble.midpit / .crps: the parts
that need no GPU.

midpit is held against a brute-force O(n^2) count in Python integers and against the average rank;
crps against the energy form sum p |x - y| - 1/2 sum sum p p' |x - x'| in longdouble, which shares
nothing with the gap form the header defines.  The sort is cooperative (ballots, LDS atomics), so the
host-emulation build refuses the three verbs by name; the argument checks of the binding are raised
before the library is called.  The GPU part is tests/test_gpu_ranks.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import ROOT, SCENARIO

E = hector_amd.HectorAmdError
LD = np.longdouble
U = 2.0 ** -53


def _brute_numerator(x, q):
    """N_i = 2 L_i + E_i and W as Python integers, by comparing every pair."""
    n = x.size
    num, W = [None] * n, 0
    for i in range(n):
        if np.isnan(x[i]):
            continue
        W += int(q[i])
        L = E_ = 0
        for j in range(n):
            if x[j] < x[i]:
                L += int(q[j])
            elif x[j] == x[i]:
                E_ += int(q[j])
        num[i] = 2 * L + E_
    return num, W


def test_midpit_against_a_brute_force_integer_count():
    rng = np.random.default_rng(11)
    n = 500
    x = np.round(rng.normal(0.0, 2.0, n))          # heavy ties
    x[rng.random(n) < 0.1] = np.nan
    x[:4] = (-0.0, 0.0, np.inf, -np.inf)
    w = rng.random(n) ** 12                         # many quantise to 0
    w[5:9] = 0.0
    q = ensemble.quantise(w, n)
    assert (q == 0).sum() > 10 and q.max() == 2 ** 32
    for weights, qq in ((None, np.ones(n, dtype=np.uint64)), (w, q)):
        num, W = _brute_numerator(x, qq)
        assert 0 < 2 * W <= 2 ** 53
        pit = ensemble.midpit(x, weights)
        raw = ensemble.midpit(x, weights, kind="numerator")
        for i in range(n):
            if num[i] is None:
                assert np.isnan(pit[i]) and np.isnan(raw[i])
            else:
                assert raw[i] == float(num[i]) and int(raw[i]) == num[i]
                assert pit[i] == float(num[i]) / float(2 * W) and 0.0 < pit[i] <= 1.0
        assert pit[0] == pit[1]                     # -0.0 and +0.0 tie
    # a zero-weight member still gets a rank; a row without weight is NaN throughout
    z = ensemble.midpit(np.array([1.0, 2.0, 3.0]), np.array([1.0, 0.0, 1.0]))
    assert (z == np.array([0.25, 0.5, 0.75])).all()
    assert np.isnan(ensemble.midpit(np.array([np.nan, 2.0, np.nan]), np.array([1.0, 0.0, 1.0]))).all()
    assert np.isnan(ensemble.midpit(np.full(5, np.nan))).all()
    # rows: the weights stay with the members
    two = ensemble.midpit(np.stack([x, x[::-1]]), w)
    assert np.array_equal(two[0], ensemble.midpit(x, w), equal_nan=True)
    assert np.array_equal(two[1], ensemble.midpit(x[::-1], w), equal_nan=True)
    with pytest.raises(ValueError):
        ensemble.midpit(x, kind="rank")
    with pytest.raises(ValueError):
        ensemble.midpit(x, w[:-1])


def test_midpit_without_weights_is_the_average_rank_bitwise():
    rng = np.random.default_rng(12)
    n = 500
    x = np.round(rng.normal(0.0, 2.0, n))
    avg = np.empty(n)
    for val in np.unique(x):
        m = x == val
        avg[m] = (x < val).sum() + (m.sum() + 1) / 2          # scipy.stats.rankdata, method "average"
    assert np.array_equal(ensemble.midpit(x), (avg - 0.5) / n)
    assert np.array_equal((ensemble.midpit(x, kind="numerator") + 1) / 2, avg)
    assert (ensemble.midpit(np.array([-0.0, 0.0, 1.0, -1.0])) == np.array([0.5, 0.5, 0.875, 0.125])).all()


def _energy(x, q, y):
    part = ~np.isnan(x) & (q > 0)
    v, p = x[part].astype(LD), q[part].astype(LD)
    p = p / p.sum()
    return (p * np.abs(v - LD(y))).sum() - LD(0.5) * (p[:, None] * p[None, :] * np.abs(v[:, None] - v[None, :])).sum()


def test_crps_against_the_energy_form():
    rng = np.random.default_rng(13)
    worst = 0.0
    for n in (1, 2, 65, 777, 1025):
        for case in range(4):
            x = rng.normal(1.5, 0.6, n)
            if case == 1:
                x = np.round(x, 1)
            if case == 2 and n > 2:
                x[rng.random(n) < 0.2] = np.nan
                x[0] = 1.0
            w = None if case == 3 else rng.random(n) ** 8 + (rng.random(n) < 0.02)
            q = ensemble.quantise(w, n)
            ok = x[~np.isnan(x) & (q > 0)]
            for y in (ok.min() - 1.0, ok.max() + 2.0, float(ok[0]), 1.4037, float(np.median(ok))):
                ref, pit, npart, m = ensemble.crps(x, y, w, dtype=LD, full=True)
                e = _energy(x, q, y)
                assert abs(ref - e) <= 1e-15 * n * max(1.0, abs(float(e))), (n, case, y, ref, e)
                got, pit2, npart2, m2 = ensemble.crps(x, y, w, full=True)
                assert (pit2, npart2, m2) == (pit, npart, m) and npart == ok.size and m == np.unique(ok).size
                assert got >= 0.0 and ensemble.crps(x, y, w) == got
                if ref > 0:
                    worst = max(worst, float(abs(LD(got) - ref) / ref) / ((m + 8) * U))
                lt, eq = int(q[~np.isnan(x) & (x < y)].sum()), int(q[~np.isnan(x) & (x == y)].sum())
                assert pit == float(2 * lt + eq) / float(2 * int(q[~np.isnan(x)].sum()))
    print("worst float64 error / ((m + 8) 2^-53): %.3g" % worst)
    assert worst <= 1.0
    # one member: |x - y|; the observation on the only value: 0, pit one half
    assert ensemble.crps(np.array([2.0]), 3.5) == 1.5
    assert ensemble.crps(np.array([2.0, np.nan]), 2.0, full=True) == (0.0, 0.5, 1, 1)
    # NaN observation, nobody taking part
    for r in (ensemble.crps(np.array([1.0, 2.0]), np.nan, full=True),
              ensemble.crps(np.array([np.nan, 2.0]), 1.0, np.array([1.0, 0.0]), full=True)):
        assert np.isnan(r[0]) and np.isnan(r[1]) and r[2:] == (0, 0)
    # rows
    X = np.stack([np.arange(5.0), np.arange(5.0)[::-1] * 2])
    c, p, k, m = ensemble.crps(X, np.array([2.0, np.nan]), full=True)
    assert c[0] == ensemble.crps(X[0], 2.0) and np.isnan(c[1]) and p[0] == 0.5 and list(k) == [5, 0]


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def test_the_three_verbs_exist_and_are_refused_by_name_in_the_emulation(emul_lib):
    from hector_amd import _lib
    lib = _lib.load(emul_lib, allow_emulation=True)
    for sym in ("hx_series_rank", "hx_metric_ranks", "hx_ensemble_crps"):
        assert sym in _lib.ABI_SYMBOLS
        getattr(lib, sym)
    c_int, dp = ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    assert lib.hx_series_rank.argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, c_int, c_int, dp, c_int]
    assert lib.hx_metric_ranks.argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, c_int, dp, c_int, dp]
    assert lib.hx_ensemble_crps.argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(c_int), dp, c_int, dp,
                                             dp, dp, ctypes.POINTER(ctypes.c_longlong)]
    spec = [Metric("mean", (1750, 1760))]
    for devices in (None, [0, 0]):
        c = _core(8, emul_lib, devices=devices)
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        for fn, call in (("hx_series_rank", lambda: c.rank_series("r", "global_tas")),
                         ("hx_series_rank", lambda: c.rank_series("r", "global_tas", (1750, 1755), np.ones(8),
                                                                  "numerator")),
                         ("hx_metric_ranks", lambda: c.metric_ranks("global_tas", spec)),
                         ("hx_ensemble_crps", lambda: c.crps("global_tas", [1750, 1760], [0.0, 0.1])),
                         ("hx_series_rank", lambda: c.spearman("global_tas", ["S", "q10_rh"]))):
            with pytest.raises(E, match=fn + " is not available in the host-emulation build"):
                call()
        assert c.series() == {}
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_argument_errors_are_raised_before_the_call(emul_lib):
    c = _core(8, emul_lib)   # (not run: a call that reached the library would say so, or refuse by name)
    spec = [Metric("mean", (1750, 1760))]
    with pytest.raises(E, match="rank_series: kind must be 'pit' or 'numerator'"):
        c.rank_series("r", "global_tas", kind="average")
    with pytest.raises(E, match="metric_ranks: kind must be 'pit' or 'numerator'"):
        c.metric_ranks("global_tas", spec, kind=1)
    with pytest.raises(E, match="rank_series: weights must have n_members entries"):
        c.rank_series("r", "global_tas", weights=np.ones(7))
    with pytest.raises(E, match="metric_ranks: weights must have n_members entries"):
        c.metric_ranks("global_tas", spec, weights=np.ones((8, 1)))
    with pytest.raises(E, match="metric_ranks: specs must be hector_amd.Metric objects"):
        c.metric_ranks("global_tas", ["mean"])
    with pytest.raises(E, match="crps: weights must have n_members entries"):
        c.crps("global_tas", [1750], [0.0], weights=np.ones(9))
    with pytest.raises(E, match="crps: years and obs must be one-dimensional and of one length"):
        c.crps("global_tas", [1750, 1751], [0.0])
    with pytest.raises(E, match="spearman: weights must have n_members entries"):
        c.spearman("global_tas", ["S"], weights=np.ones(3))
    with pytest.raises(E, match="spearman: entry 0 of against must have n_members values"):
        c.spearman("global_tas", [np.ones(3)])
    with pytest.raises(E, match="spearman: against is empty"):
        c.spearman("global_tas", [])
    # the library's own checks name their function (they come before the emulation's refusal)
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.zeros(8)
    rc = c._lib.hx_series_rank(c._h, b"r", b"global_tas", 1750, 1760, None, 7)
    assert rc != 0 and "hx_series_rank: unknown kind 7" in c._lib.hx_last_error().decode()
    arr, ns = spec[0]._c(), 1   # (one hx_metric)
    rc = c._lib.hx_metric_ranks(c._h, b"global_tas", ctypes.byref(arr), ns, None, -1, out.ctypes.data_as(dp))
    assert rc != 0 and "hx_metric_ranks: unknown kind -1" in c._lib.hx_last_error().decode()
    rc = c._lib.hx_ensemble_crps(c._h, b"global_tas", (ctypes.c_int * 1)(1750), out.ctypes.data_as(dp), 0, None,
                                 out.ctypes.data_as(dp), None, None)
    assert rc != 0 and "hx_ensemble_crps: nyears < 1" in c._lib.hx_last_error().decode()
    rc = c._lib.hx_series_rank(c._h, b"r", b"global_tas", 1750, 1760, (ctypes.c_double * 8)(*([0.0] * 8)), 0)
    assert rc != 0 and "hx_series_rank: the weights are all zero" in c._lib.hx_last_error().decode()
    rc = c._lib.hx_series_rank(c._h, None, b"global_tas", 1750, 1760, None, 0)
    assert rc != 0 and "hx_series_rank: null argument" in c._lib.hx_last_error().decode()
    assert c.series() == {}
    c.shutdown()


def test_the_header_documents_the_symbols_and_the_binding_declares_them():
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    for define in ("#define HX_RANK_PIT 0", "#define HX_RANK_NUMERATOR 1", "#define HX_RANK_SCRATCH_MIB"):
        assert define in text
    assert re.search(r"\bint hx_series_rank\(hx_core \*core, const char \*name, const char \*capability", text)
    for fn in ("hx_metric_ranks", "hx_ensemble_crps"):
        assert re.search(r"\bint %s\(hx_core \*core, const char \*capability" % fn, text)
    doc = text[text.index("Member ranks within a year's row"):text.index("int hx_series_rank(")]
    for phrase in ("rint(w_m / wmax * 2^32)", "-0.0", "N_i = 2 L_i + E_i", "(double) N_i / (double) (2 W)",
                   "such a member still gets a rank", "W = 0 gives NaN for the whole row", "bit for bit",
                   "G_k = (double) (W - C_k) / (double) W", "(v_(k+1) - v_k) * (G_k * G_k)",
                   "(y - v_k) * (F_k * F_k)", "(m + 8) 2^-53", "energy form", "n_part 0", "infinite",
                   "HX_RANK_SCRATCH_MIB MiB", "valid_to = year1", "16-series limit", "member order",
                   "an unknown kind", "nyears < 1", "several shards", "several processes",
                   "no device memory", "host-emulation"):
        assert phrase in doc, phrase
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    for fn in ("hx_series_rank", "hx_metric_ranks", "hx_ensemble_crps"):
        assert "int %s(" % fn in abi
