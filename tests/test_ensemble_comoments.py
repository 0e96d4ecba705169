"""hx_ensemble_comoments (Core.comoments, hector_amd.CoMoments): the parts that need no GPU.

The Gram kernel runs on the matrix pipe, so the host-emulation build refuses the verb by name; the
argument checks of the binding are raised before the library is called; and the arithmetic of
`CoMoments` -- mean, cov, corr, slope, pca -- is held against numpy's weighted formulas on the
synthetic data the hand-built sums come from.  The GPU part is tests/test_gpu_comoments.py.

Tolerance of the derived statistics: 4 kappa (n + 8) 2^-53, relatively, as tests/test_gpu_moments.py
derives it: kappa_a = (T_a/W) / var_a is the cancellation in var_a = T_a/W - (S_a/W)^2 (mean and
var), and kappa_a kappa_b bounds the cancellation in cov = cross/W - (S_a/W)(S_b/W), since
|cross/W| <= sqrt(T_a/W T_b/W); corr and slope inherit it.  kappa <= KAPPA_MAX of that file is asserted.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import ensemble
from conftest import ROOT, SCENARIO

E = hector_amd.HectorAmdError
LD = np.longdouble
U = 2.0 ** -53
KAPPA_MAX = 3e4     # tests/test_gpu_moments.py (a GPU module: its constant is restated and compared below)


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def hand_comoments(xa, xb, q, symmetric=False):
    """The definition of include/hector_amd.h, literally: d in float64 (one IEEE subtraction), the
    sums in longdouble -> (CoMoments, record of the longdouble sums)."""
    na, nb = xa.shape[0], xb.shape[0]
    part = (q > 0) & ~np.isnan(xa).any(axis=0) & ~np.isnan(xb).any(axis=0)
    rec = dict(part=part, sums_a=np.zeros((na, 2), dtype=LD), sums_b=np.zeros((nb, 2), dtype=LD),
               cross=np.zeros((na, nb), dtype=LD), shift_a=np.full(na, np.nan), shift_b=np.full(nb, np.nan),
               wsum=0, n_part=0)
    if part.any():
        w = q[part].astype(LD)
        rec["wsum"], rec["n_part"] = int(sum(int(v) for v in q[part])), int(part.sum())
        rec["shift_a"], rec["shift_b"] = xa[:, part].min(axis=1), xb[:, part].min(axis=1)
        da = (xa[:, part] - rec["shift_a"][:, None]).astype(LD)
        db = (xb[:, part] - rec["shift_b"][:, None]).astype(LD)
        assert (da >= 0).all() and (db >= 0).all()
        rec["sums_a"] = np.stack([(w * da).sum(axis=1), (w * da * da).sum(axis=1)], axis=1)
        rec["sums_b"] = np.stack([(w * db).sum(axis=1), (w * db * db).sum(axis=1)], axis=1)
        rec["cross"] = (w * da) @ db.T
    cm = hector_amd.CoMoments(rec["shift_a"], rec["sums_a"].astype(np.float64), rec["shift_b"],
                              rec["sums_b"].astype(np.float64), rec["cross"].astype(np.float64), rec["wsum"],
                              rec["n_part"], symmetric=symmetric)
    return cm, rec


def test_the_header_documents_the_symbol_and_the_libraries_export_it(emul_lib, hip_lib):
    from hector_amd import _lib
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert re.search(r"\bint hx_ensemble_comoments\(hx_core \*core, const char \*cap_a, int a_year0, int a_year1,", text)
    doc = text[text.index("Year-by-year co-moments of two windows"):text.index("int hx_ensemble_comoments(")]
    for phrase in ("COMPLETE CASES", "ONE W", "ONE n_part", "hx_ensemble_moments, where participation is per row",
                   "positive semi-definite", "ONE IEEE subtraction", "cross[a * nb + b] = sum (q d_a) d_b",
                   "(n_part + 8) 2^-53", "cov[a][b] = cross[a][b]/W - (S_a/W)(S_b/W)", "corr[a][b]",
                   "SYMMETRIC call", "EXACTLY symmetric", "sums_a[a * 2 + 1] is\n * set to cross[a * na + a]",
                   "Nobody takes part", "NOT bit-identical", "from call to call", "ascending chunk order",
                   "a core that has not\n * run", "several processes is refused", "host-emulation",
                   "Out of scope: a metric x metric variant, and per-entry (pairwise) participation"):
        assert phrase in doc, phrase
    assert "hx_ensemble_comoments" in _lib.ABI_SYMBOLS
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    assert "int hx_ensemble_comoments(" in abi and "hx_ensemble_comoments: null argument" in abi
    post = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_post.h")).read()
    for name in ("HXC_TILE", "HXC_CHUNK"):
        assert re.search(r"^#define %s \d+" % name, post, re.M), name
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in post[post.index("hx_co_gram_kernel"):]
    _lib.load(emul_lib, allow_emulation=True).hx_ensemble_comoments
    assert os.path.exists(hip_lib)    # (the product library: built by build(), loads without a GPU)
    ctypes.CDLL(hip_lib).hx_ensemble_comoments


def test_the_emulation_refuses_by_name_and_changes_nothing(emul_lib):
    for devices in (None, [0, 0]):
        c = _core(5, emul_lib, devices=devices)
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        for call in (lambda: c.comoments("global_tas"),
                     lambda: c.comoments("global_tas", (1750, 1760), weights=np.ones(5)),
                     lambda: c.comoments("global_tas", (1750, 1755), "global_tas", (1756, 1760))):
            with pytest.raises(E, match="hx_ensemble_comoments is not available in the host-emulation build"):
                call()
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_argument_errors_are_raised_before_the_call(emul_lib):
    c = _core(6, emul_lib)   # (not run: a call that reached the library would say so, or refuse by name)
    with pytest.raises(E, match="comoments: weights must have n_members entries"):
        c.comoments("global_tas", weights=np.ones(7))
    with pytest.raises(E, match="comoments: weights must have n_members entries"):
        c.comoments("global_tas", (1750, 1760), "global_tas", (1750, 1760), weights=np.ones((6, 1)))
    # a window outside the scenario is refused by name before anything is sized from it
    for dates in ((0, 10 ** 9), (1745, 2 ** 31 - 1), (-2 ** 31, 1800), (-2 ** 31, 2 ** 31 - 1)):
        with pytest.raises(E, match="hx_ensemble_comoments: dates must lie between"):
            c.comoments("global_tas", dates)
        with pytest.raises(E, match="hx_ensemble_comoments: dates must lie between"):
            c.comoments("global_tas", (1750, 1760), "global_tas", dates)
    # null arguments of the C ABI are refused by name before the core is looked at
    dp = ctypes.POINTER(ctypes.c_double)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(dp)
    for args in ((None, 1745, 1745, None, 0, 0, None, p, p, None, None, p, None, None),
                 (b"global_tas", 1745, 1745, None, 0, 0, None, p, p, None, None, None, None, None),
                 (b"global_tas", 1745, 1745, b"global_tas", 1745, 1745, None, p, p, None, None, p, None, None)):
        assert c._lib.hx_ensemble_comoments(c._h, *args) != 0
        assert "hx_ensemble_comoments: null argument" in c._lib.hx_last_error().decode()
    c.shutdown()
    with pytest.raises(E, match="CoMoments: sums_a"):
        hector_amd.CoMoments([0.0, 0.0], [[1.0, 1.0]], [0.0], [[1.0, 1.0]], [[1.0], [1.0]], 1, 1)


def test_comoments_arithmetic_against_numpy_weighted_formulas():
    assert KAPPA_MAX == float(re.search(r"^KAPPA_MAX = (\S+)", open(os.path.join(
        ROOT, "tests", "test_gpu_moments.py")).read(), re.M).group(1))
    rng = np.random.default_rng(29)
    n, na, nb = 500, 6, 4
    f = rng.normal(0.0, 1.0, (2, n))                     # two common factors: robust correlations
    xa = 14.0 + np.outer(np.linspace(0.5, 2.0, na), f[0]) + np.outer(np.linspace(0.5, 1.5, na), f[1]) \
        + 0.3 * rng.normal(0.0, 1.0, (na, n))
    xb = 300.0 + np.outer(np.linspace(5.0, 9.0, nb), f[0]) + np.outer([2.0, 3.0, 4.0, 6.0], f[1]) \
        + rng.normal(0.0, 1.0, (nb, n))
    xa[2, 7] = np.nan                                    # NaN in A only, in B only, in both
    xb[1, 9] = np.nan
    xa[0, 11] = xb[3, 11] = np.nan
    xa[5, 0] = xb[0, n - 1] = np.nan                     # the first and the last member
    q = rng.integers(0, 2 ** 32, n).astype(np.uint64)
    q[20:40] = 0
    cm, rec = hand_comoments(xa, xb, q)
    part = rec["part"]
    assert cm.n_part == n - 20 - 5 == part.sum() and cm.wsum == int(q[part].astype(object).sum())
    w = q[part].astype(LD) / q[part].astype(LD).sum()
    A, B = xa[:, part].astype(LD), xb[:, part].astype(LD)
    ma, mb = (w * A).sum(axis=1), (w * B).sum(axis=1)
    va, vb = (w * (A - ma[:, None]) ** 2).sum(axis=1), (w * (B - mb[:, None]) ** 2).sum(axis=1)
    cov = (w * (A - ma[:, None])) @ (B - mb[:, None]).T
    corr, slope = cov / np.sqrt(np.outer(va, vb)), cov / vb[None, :]
    W = LD(rec["wsum"])
    ka, kb = (rec["sums_a"][:, 1] / W) / va, (rec["sums_b"][:, 1] / W) / vb
    kab = np.outer(ka, kb)
    assert 1.0 <= ka.min() and 1.0 <= kb.min() and float(kab.max()) <= KAPPA_MAX, (ka, kb)
    assert np.abs(corr).min() > 0.05                     # (relative tolerances on cov need it away from 0)
    tol = 4.0 * (cm.n_part + 8) * U
    assert (np.abs(cm.mean_a - ma) <= tol * ka * np.abs(ma)).all() and (np.abs(cm.mean_b - mb) <= tol * kb * np.abs(mb)).all()
    assert (np.abs(cm.var_a - va) <= tol * ka * va).all() and (np.abs(cm.var_b - vb) <= tol * kb * vb).all()
    for name, got, ref in (("cov", cm.cov, cov), ("corr", cm.corr, corr), ("slope", cm.slope, slope)):
        err = np.abs(got.astype(LD) - ref)
        assert (err <= tol * kab * np.abs(ref)).all(), (name, float((err / (tol * kab * np.abs(ref))).max()))
    assert cm.cov.shape == cm.corr.shape == cm.slope.shape == (na, nb)
    assert np.array_equal(cm.years_a, np.arange(na)) and np.array_equal(cm.years_b, np.arange(nb))
    # a zero-variance row of B: corr and slope NaN in its column; of A: corr NaN, slope 0
    xb2, xa2 = xb.copy(), xa.copy()
    xb2[2] = 278.0
    xa2[4] = -3.0
    z, _ = hand_comoments(xa2, xb2, q)
    assert z.var_b[2] == 0.0 and z.var_a[4] == 0.0
    assert np.isnan(z.corr[:, 2]).all() and np.isnan(z.slope[:, 2]).all() and np.isnan(z.corr[4]).all()
    keep = np.arange(nb) != 2
    assert (z.slope[4, keep] == 0.0).all() and np.isfinite(z.corr[np.arange(na) != 4][:, keep]).all()
    # nobody takes part: NaN shifts, zero sums, W = n_part = 0, NaN statistics
    e, _ = hand_comoments(xa, np.full((nb, n), np.nan), q)
    assert e.wsum == 0 and e.n_part == 0 and np.isnan(e.shift_a).all() and np.isnan(e.shift_b).all()
    assert (e.cross == 0).all() and (e.sums_a == 0).all() and (e.sums_b == 0).all()
    for fld in (e.mean_a, e.mean_b, e.var_a, e.var_b, e.cov, e.corr, e.slope):
        assert np.isnan(fld).all()
    assert e.cov.shape == (na, nb)


def test_pca_of_a_rank_two_matrix():
    rng = np.random.default_rng(31)
    n, na = 4000, 7
    # two orthogonal patterns with exactly orthogonal, centred, unit-variance scores
    p = np.linalg.qr(rng.normal(size=(na, 2)))[0].T
    s = rng.normal(size=(2, n))
    s -= s.mean(axis=1, keepdims=True)
    s = np.linalg.qr(s.T)[0].T * np.sqrt(n)
    lam = np.array([9.0, 2.25])
    x = 5.0 + (p.T * np.sqrt(lam)) @ s
    cm, _ = hand_comoments(x, x, np.ones(n, dtype=np.uint64), symmetric=True)
    val, share, pat = cm.pca(2)
    assert np.allclose(val, lam, rtol=1e-10, atol=0)
    assert share.sum() == pytest.approx(1.0, abs=1e-10) and share[0] == pytest.approx(9.0 / 11.25, rel=1e-10)
    for k in range(2):
        assert pat[k, np.argmax(np.abs(pat[k]))] > 0
        assert abs(abs(pat[k] @ p[k]) - 1.0) < 1e-9
    val7, share7, pat7 = cm.pca(na)
    assert pat7.shape == (na, na) and share7.sum() == pytest.approx(1.0, abs=1e-10) and (np.diff(val7) <= 0).all()
    assert np.abs(val7[2:]).max() < 1e-10
    with pytest.raises(E, match="CoMoments.pca: k must lie in 1..7"):
        cm.pca(8)
    cross, _ = hand_comoments(x, x, np.ones(n, dtype=np.uint64))
    with pytest.raises(E, match="CoMoments.pca: needs a symmetric result"):
        cross.pca(2)
