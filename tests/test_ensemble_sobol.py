"""hx_ensemble_sobol / hx_metric_sobol (Core.sobol, Core.metric_sobol, hector_amd.Sobol) and the
Saltelli design of hector_amd.ensemble: the parts that need no GPU.

The design is held to its layout (groups of k + 2 consecutive rows: A_j, B_j, then A_j with column i
from B_j) and to its counters.  The arithmetic of `Sobol` is held against the header's formulas on
numpy longdouble sums of the Ishigami function (a = 7, b = 0.1), whose indices are known in closed
form: every estimate must lie within 4 of its own standard errors of the analytic value.  The sum
kernel is cooperative (cross-lane reduction), so the host-emulation build refuses both verbs by name;
the argument checks of the binding are raised before the library is called.
The GPU part is tests/test_gpu_sobol.py.
"""
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import ROOT, SCENARIO

E = hector_amd.HectorAmdError
LD = np.longdouble


def test_saltelli_shape_layout_and_offset():
    for n_base, k in ((5, 1), (7, 3), (3, 16)):
        U = ensemble.saltelli(n_base, k)
        assert U.shape == ((k + 2) * n_base, k) and U.dtype == np.float64
        assert (U >= 0).all() and (U < 1).all()
        G = U.reshape(n_base, k + 2, k)
        idx = np.arange(n_base, dtype=np.uint64)
        for i in range(k):
            assert np.array_equal(G[:, 0, i], ensemble.uniform01(idx, i))
            assert np.array_equal(G[:, 1, i], ensemble.uniform01(idx, k + i))
        for r in range(2, k + 2):
            other = np.arange(k) != r - 2
            assert np.array_equal(G[:, r, other], G[:, 0, other])
            assert np.array_equal(G[:, r, r - 2], G[:, 1, r - 2])
        assert not np.array_equal(G[:, 0], G[:, 1])
    big = ensemble.saltelli(40, 3)
    assert np.array_equal(ensemble.saltelli(9, 3, offset=11), big[11 * 5:20 * 5])
    assert not np.array_equal(ensemble.saltelli(9, 3, seed=1), ensemble.saltelli(9, 3))


def _ishigami(u, a=7.0, b=0.1):
    x = -np.pi + 2.0 * np.pi * u
    return np.sin(x[:, 0]) + a * np.sin(x[:, 1]) ** 2 + b * x[:, 2] ** 4 * np.sin(x[:, 0])


def _hand_sums(x, k):
    """The definition of include/hector_amd.h on one row x[(k + 2) n]: differences in float64, the
    sums in longdouble -> shift, sums[4 + 4 k] (longdouble), n."""
    g = x.reshape(-1, k + 2)
    on = ~np.isnan(g).any(axis=1)
    g = g[on]
    c = min(g[:, 0].min(), g[:, 1].min())
    dA, dB = (g[:, 0] - c).astype(LD), (g[:, 1] - c).astype(LD)
    s = [dA.sum(), (dA * dA).sum(), dB.sum(), (dB * dB).sum()]
    for i in range(k):
        t = (g[:, 0] - g[:, 2 + i]).astype(LD) ** 2
        u = (g[:, 1] - g[:, 2 + i]).astype(LD) ** 2
        s += [t.sum(), (t * t).sum(), u.sum(), (u * u).sum()]
    return c, np.array(s, dtype=LD), int(on.sum())


def test_sobol_arithmetic_on_the_ishigami_function():
    n, k = 4096, 3
    x = _ishigami(ensemble.saltelli(n, k))
    c, s, npart = _hand_sums(x, k)
    assert npart == n
    so = hector_amd.Sobol(["x1", "x2", "x3"], [c], s.astype(np.float64)[None, :], [npart])
    # the header's formulas on the longdouble sums
    nl = LD(npart)
    m = (s[0] + s[2]) / (2 * nl)
    V = (s[1] + s[3]) / (2 * nl) - m * m
    assert so.mean[0] == pytest.approx(float(c + m), rel=1e-14)
    assert so.var[0] == pytest.approx(float(V), rel=1e-12)
    assert so.mean[0] == pytest.approx(x.reshape(-1, k + 2)[:, :2].mean(), rel=1e-12)
    assert so.var[0] == pytest.approx(x.reshape(-1, k + 2)[:, :2].var(), rel=1e-10)
    total = np.array([float(s[4 + 4 * i] / (2 * nl * V)) for i in range(k)])
    first = np.array([float(1 - s[6 + 4 * i] / (2 * nl * V)) for i in range(k)])
    tse = np.array([float(np.sqrt((s[5 + 4 * i] / nl - (s[4 + 4 * i] / nl) ** 2) / nl) / (2 * V)) for i in range(k)])
    fse = np.array([float(np.sqrt((s[7 + 4 * i] / nl - (s[6 + 4 * i] / nl) ** 2) / nl) / (2 * V)) for i in range(k)])
    assert so.total.shape == so.first.shape == so.total_se.shape == so.first_se.shape == (1, k)
    assert np.allclose(so.total[0], total, rtol=1e-12, atol=0)
    assert np.allclose(so.first[0], first, rtol=0, atol=1e-13)
    assert np.allclose(so.total_se[0], tse, rtol=1e-10, atol=0)
    assert np.allclose(so.first_se[0], fse, rtol=1e-10, atol=0)
    # ... and the estimates against the closed form
    dev_f = np.abs(so.first[0] - np.array([0.3139, 0.4424, 0.0])) / so.first_se[0]
    dev_t = np.abs(so.total[0] - np.array([0.5576, 0.4424, 0.2437])) / so.total_se[0]
    print("deviation in standard errors: first %r total %r" % (dev_f, dev_t))
    assert (so.first_se[0] > 0).all() and (so.total_se[0] > 0).all()
    assert (dev_f <= 4).all() and (dev_t <= 4).all()
    assert (so.total[0] >= 0).all()


def test_sobol_undefined_rows_and_shape_errors():
    # row 0: nobody takes part; row 1: all values equal (V == 0)
    so = hector_amd.Sobol(["a", "b"], [np.nan, 3.0], np.zeros((2, 12)), [0, 10])
    assert np.isnan(so.mean[0]) and np.isnan(so.var[0]) and so.mean[1] == 3.0 and so.var[1] == 0.0
    for f in (so.first, so.total, so.first_se, so.total_se):
        assert f.shape == (2, 2) and np.isnan(f).all()
    with pytest.raises(E, match="4 \\+ 4 \\* len\\(names\\)"):
        hector_amd.Sobol(["a"], [1.0], np.zeros((1, 12)), [4])
    assert "Sobol" in repr(so)


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    U = ensemble.saltelli(n // 4, 2)
    c.setvar("S", 1.5 + 4.5 * U[:, 0], "degC").setvar("q10_rh", 1.0 + 2.0 * U[:, 1])
    return c


def test_both_verbs_exist_and_are_refused_by_name_in_the_emulation(emul_lib):
    from hector_amd import _lib
    lib = _lib.load(emul_lib, allow_emulation=True)
    assert "hx_ensemble_sobol" in _lib.ABI_SYMBOLS and "hx_metric_sobol" in _lib.ABI_SYMBOLS
    lib.hx_ensemble_sobol, lib.hx_metric_sobol
    spec = [Metric("mean", (1750, 1760))]
    for devices in (None, [0, 0]):
        c = _core(8, emul_lib, devices=devices)
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        for fn, call in (("hx_ensemble_sobol", lambda: c.sobol("global_tas", 2)),
                         ("hx_ensemble_sobol", lambda: c.sobol("global_tas", ["S", "q10_rh"], (1750, 1760),
                                                               use=[1, 0])),
                         ("hx_metric_sobol", lambda: c.metric_sobol("global_tas", spec, 2))):
            with pytest.raises(E, match=fn + " is not available in the host-emulation build"):
                call()
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_argument_errors_are_raised_before_the_call(emul_lib):
    c = _core(8, emul_lib)   # (not run: a call that reached the library would say so, or refuse by name)
    spec = [Metric("mean", (1750, 1760))]
    with pytest.raises(E, match="sobol: use must have n_base entries"):
        c.sobol("global_tas", 2, use=np.ones(3))
    with pytest.raises(E, match="sobol: use must have n_base entries"):
        c.sobol("global_tas", 2, n_base=1, use=np.ones(2))
    with pytest.raises(E, match="metric_sobol: use must have n_base entries"):
        c.metric_sobol("global_tas", spec, ["S", "q10_rh"], use=np.ones((2, 1)))
    with pytest.raises(E, match="sobol: at most 16 factors"):
        c.sobol("global_tas", 17)
    with pytest.raises(E, match="metric_sobol: at most 16 factors"):
        c.metric_sobol("global_tas", spec, ["f%d" % i for i in range(17)])
    with pytest.raises(E, match="metric_sobol: specs must be hector_amd.Metric objects"):
        c.metric_sobol("global_tas", ["mean"], 2)
    c.shutdown()


def test_the_header_documents_the_symbols_and_the_binding_declares_them():
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert "#define HX_SOBOL_MAX_FACTORS 16" in text
    for fn in ("hx_ensemble_sobol", "hx_metric_sobol"):
        assert re.search(r"\bint %s\(hx_core \*core, const char \*capability" % fn, text)
    doc = text[text.index("Variance-based (Sobol) sensitivity sums"):text.index("int hx_ensemble_sobol(")]
    for phrase in ("SA1 = sum dA", "T_i = sum t", "FF_i = sum u u", "total_i = T_i / (2 n V)",
                   "first_i = 1 - F_i / (2 n V)", "with V taken as", "NOT", "from call to call",
                   "k outside 1..16", "several shards", "host-emulation"):
        assert phrase in doc, phrase
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    assert "int hx_ensemble_sobol(" in abi and "int hx_metric_sobol(" in abi
