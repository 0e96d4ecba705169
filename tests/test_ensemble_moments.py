"""hx_ensemble_moments / hx_metric_moments (Core.moments, Core.metric_moments, hector_amd.Moments):
the parts that need no GPU.

The sum kernel is cooperative (cross-lane reduction), so the host-emulation build refuses both verbs
by name; the argument checks of the binding are raised before the library is called; and the
arithmetic of `Moments` -- mean, var, cov, corr, slope and the standardised regression coefficients
-- is held against numpy's weighted formulas on the synthetic data the hand-built sums come from.
The GPU part is tests/test_gpu_moments.py.
"""
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, ensemble
from conftest import ROOT, SCENARIO

E = hector_amd.HectorAmdError


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def test_both_verbs_exist_and_are_refused_by_name_in_the_emulation(emul_lib):
    from hector_amd import _lib
    lib = _lib.load(emul_lib, allow_emulation=True)
    assert "hx_ensemble_moments" in _lib.ABI_SYMBOLS and "hx_metric_moments" in _lib.ABI_SYMBOLS
    lib.hx_ensemble_moments, lib.hx_metric_moments
    spec = [Metric("mean", (1750, 1760))]
    for devices in (None, [0, 0]):
        c = _core(5, emul_lib, devices=devices)
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        for fn, call in (("hx_ensemble_moments", lambda: c.moments("global_tas", against=["S"])),
                         ("hx_ensemble_moments", lambda: c.moments("global_tas", weights=np.ones(5))),
                         ("hx_metric_moments", lambda: c.metric_moments("global_tas", spec, against=["S", "q10_rh"]))):
            with pytest.raises(E, match=fn + " is not available in the host-emulation build"):
                call()
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_argument_errors_are_raised_before_the_call(emul_lib):
    c = _core(6, emul_lib)   # (not run: a call that reached the library would say so, or refuse by name)
    spec = [Metric("mean", (1750, 1760))]
    with pytest.raises(E, match="moments: entry 1 of against must have n_members values"):
        c.moments("global_tas", against=["S", np.zeros(5)])
    with pytest.raises(E, match="metric_moments: entry 0 of against must have n_members values"):
        c.metric_moments("global_tas", spec, against=[np.zeros((6, 2))])
    with pytest.raises(E, match="moments: entry 0 of against must have n_members values"):
        c.moments("global_tas", against=np.zeros(9))     # one array is one entry, not nine
    with pytest.raises(E, match="moments: at most 8 entries in against"):
        c.moments("global_tas", against=[np.zeros(6)] * 9)
    with pytest.raises(E, match="metric_moments: at most 8 entries in against"):
        c.metric_moments("global_tas", spec, against=["S"] * 9)
    with pytest.raises(E, match="moments: weights must have n_members entries"):
        c.moments("global_tas", weights=np.ones(7))
    with pytest.raises(E, match="metric_moments: weights must have n_members entries"):
        c.metric_moments("global_tas", spec, weights=np.ones((6, 1)))
    with pytest.raises(E, match="metric_moments: specs must be hector_amd.Metric objects"):
        c.metric_moments("global_tas", ["mean"])
    c.shutdown()


def _hand_sums(x, q, pred):
    """The definition of include/hector_amd.h, literally, in float64 -> Moments."""
    ny, n = x.shape
    k = pred.shape[0]
    ok = (q > 0) & np.isfinite(pred).all(axis=0)
    pshift = pred[:, ok].min(axis=1)
    shift, sums = np.full(ny, np.nan), np.zeros((ny, 2 + 3 * k))
    wsum, npart = np.zeros(ny, dtype=np.uint64), np.zeros(ny, dtype=np.int64)
    for y in range(ny):
        part = ok & ~np.isnan(x[y])
        if not part.any():
            continue
        w = q[part].astype(np.float64)
        shift[y] = x[y, part].min()
        d = x[y, part] - shift[y]
        wsum[y], npart[y] = int(q[part].sum()), int(part.sum())
        sums[y, 0], sums[y, 1] = (w * d).sum(), (w * d * d).sum()
        for j in range(k):
            e = pred[j, part] - pshift[j]
            sums[y, 2 + 3 * j:5 + 3 * j] = (w * e).sum(), (w * e * e).sum(), (w * d * e).sum()
    return hector_amd.Moments(shift, sums, wsum, npart, ["p%d" % j for j in range(k)], pshift, q, pred)


def test_moments_arithmetic_against_numpy_weighted_formulas():
    rng = np.random.default_rng(17)
    n, k = 400, 3
    pred = rng.normal(0.0, 1.0, (k, n)) * np.array([[1.0], [0.2], [30.0]]) + np.array([[3.0], [2.0], [-50.0]])
    pred[1] += 0.3 * pred[0]                        # correlated predictors: SRC differs from corr
    pred[2, 11] = np.nan                            # member 11 never takes part
    q = rng.integers(0, 2 ** 32, n).astype(np.uint64)
    q[:20] = 0
    x = np.empty((5, n))
    x[0] = 400.0 + 2.0 * pred[0] - 5.0 * pred[1] + rng.normal(0, 1.0, n)
    x[1] = 1.0 + 0.01 * pred[2] + rng.normal(0, 0.1, n)
    x[2] = 278.0                                    # a zero-variance row
    x[3] = x[0]
    x[3, 100:110] = np.nan                          # a row whose n_part differs
    x[4] = np.nan                                   # nobody takes part
    m = _hand_sums(x, q, pred)
    ok = (q > 0) & np.isfinite(pred).all(axis=0)
    assert m.n_part[0] == ok.sum() and m.n_part[3] == ok.sum() - 10 and m.n_part[4] == 0
    for y in range(4):
        part = ok & ~np.isnan(x[y])
        w = q[part].astype(np.float64) / q[part].astype(np.float64).sum()
        xv, pv = x[y, part], pred[:, part]
        mean = (w * xv).sum()
        var = (w * (xv - mean) ** 2).sum()
        pmean = (w * pv).sum(axis=1)
        pvar = (w * (pv - pmean[:, None]) ** 2).sum(axis=1)
        cov = (w * (xv - mean) * (pv - pmean[:, None])).sum(axis=1)
        assert m.mean[y] == pytest.approx(mean, rel=1e-13)
        assert np.allclose(m.pmean[y], pmean, rtol=1e-12, atol=0) and np.allclose(m.pvar[y], pvar, rtol=1e-10, atol=0)
        if y == 2:
            assert m.var[y] == 0.0 and (m.sums[y, :2] == 0).all()
            assert np.isnan(m.corr[y]).all() and np.isnan(m.src()[y]).all()
            assert (m.cov[y] == 0.0).all() and (m.slope[y] == 0.0).all()   # slope needs pvar only
            continue
        assert m.var[y] == pytest.approx(var, rel=1e-10)
        assert np.allclose(m.cov[y], cov, rtol=1e-9, atol=1e-13)
        assert np.allclose(m.corr[y], cov / np.sqrt(var * pvar), rtol=1e-9, atol=1e-12)
        assert np.allclose(m.slope[y], cov / pvar, rtol=1e-9, atol=1e-13)
        # standardised coefficients of the joint weighted least-squares fit
        zx = (xv - mean) / np.sqrt(var)
        zp = (pv - pmean[:, None]) / np.sqrt(pvar)[:, None]
        beta = np.linalg.lstsq((zp * np.sqrt(w)).T, zx * np.sqrt(w), rcond=None)[0]
        if y == 3:
            assert np.isnan(m.src()[y]).all()      # its participants are not those of R_pp
        else:
            assert np.allclose(m.src()[y], beta, rtol=1e-8, atol=1e-10)
            assert not np.allclose(m.src()[y], m.corr[y], rtol=1e-3)
    for f in (m.mean, m.var, m.sd):
        assert np.isnan(f[4])
    for f in (m.pmean, m.pvar, m.cov, m.corr, m.slope, m.src()):
        assert f.shape == (5, k) and np.isnan(f[4]).all()
    assert np.isnan(m.shift[4]) and m.wsum[4] == 0 and (m.sums[4] == 0).all()
    # a zero-variance predictor: corr and slope NaN for it, and no joint solution
    pred2 = pred.copy()
    pred2[1] = 2.5
    m2 = _hand_sums(x[:1], q, pred2)
    assert np.isnan(m2.corr[0, 1]) and np.isnan(m2.slope[0, 1]) and np.isfinite(m2.corr[0, [0, 2]]).all()
    assert np.isnan(m2.src()).all()
    # no predictors
    m0 = hector_amd.Moments([1.0], [[2.0, 8.0]], [4], [4])
    assert m0.mean[0] == 1.5 and m0.var[0] == 1.75 and m0.corr.shape == (1, 0) and m0.src().shape == (1, 0)
    with pytest.raises(E, match="2 \\+ 3 \\* len\\(names\\)"):
        hector_amd.Moments([1.0], [[2.0, 8.0]], [4], [4], names=["S"])


def test_the_header_documents_the_symbols_and_the_binding_declares_them():
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert "#define HX_MOM_MAX_PRED 8" in text
    for fn in ("hx_ensemble_moments", "hx_metric_moments"):
        assert re.search(r"\bint %s\(hx_core \*core, const char \*capability" % fn, text)
    doc = text[text.index("Weighted moments of every recorded year"):text.index("int hx_ensemble_moments(")]
    for phrase in ("A = sum q d", "B = sum q d d", "E_k = sum q d e_k", "NOT bit-identical", "from call to call",
                   "var = B/W - (A/W)^2", "corr_k", "slope_k", "npred outside 0..8", "host-emulation"):
        assert phrase in doc, phrase
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    assert "int hx_ensemble_moments(" in abi and "int hx_metric_moments(" in abi
