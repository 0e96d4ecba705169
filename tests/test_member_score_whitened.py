"""hx_member_score_whitened (Core.score with cov=, ar1= or whiten=; hector_amd.whiten): the parts
that need no GPU.

The contraction runs on the fp64 matrix pipe, so the host-emulation build refuses the verb by name --
after the argument checks, which are therefore testable here one by one.  `hector_amd.whiten` is
plain numpy and is held to exact results where they exist (powers of two) and to a bound where they
do not.  The GPU part is tests/test_gpu_score_whitened.py.

Bound of W C W^T = I for W = tril(solve(L, I)), L = cholesky(C): backward-stable factorisation and
triangular solves leave a residual of a small multiple of n u cond_2(C); 8 n cond_2(C) 2^-53 is what
this file asks.
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
FN = "hx_member_score_whitened"
NMAX = 256


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def _ar1(years, sigma, rho):
    years = np.asarray(years)
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), years.shape)
    return s[:, None] * s[None, :] * rho ** np.abs(years[:, None] - years[None, :])


def test_the_header_documents_the_symbol_and_the_libraries_export_it(emul_lib, hip_lib):
    from hector_amd import _lib
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert re.search(r"\bint hx_member_score_whitened\(hx_core \*core, const char \*capability, const int \*years, "
                     r"const double \*obs,\s+const double \*whiten, int n, int base_year0, int base_year1, "
                     r"double \*out\);", text)
    assert re.search(r"^#define HX_SCORE_WHITENED_MAX 256$", text, re.M)
    doc = text[text.index("whose errors are CORRELATED"):text.index("int hx_member_score_whitened(")]
    for phrase in ("r_k = (x(years[k], member) - base(member)) - obs[k]",
                   "y_i = sum_{k <= i} whiten[i * n + k] * r_k", "chi2[member] = sum_i y_i^2",
                   "ONE division", "two IEEE subtractions", "ONLY the entries with k <= i are read",
                   "1 <= n <= HX_SCORE_WHITENED_MAX", "NO skipping", "any order, repeats allowed",
                   "NOT part of the definition", "(3 n + 8) 2^-53 sum_i s_i^2", "ONE\n * fixed order",
                   "nor on which other members exist", "gets NaN", "shard by shard", "host-emulation build refuses"):
        assert phrase in doc, phrase
    assert FN in _lib.ABI_SYMBOLS
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    assert "int %s(" % FN in abi and "%s: null argument" % FN in abi
    post = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_post.h")).read()
    assert re.search(r"^#define HXW_TILE 16\b", post, re.M) and re.search(r"^#define HXW_MAX 256\b", post, re.M)
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in post[post.index("hx_score_whiten_kernel("):]
    lib = _lib.load(emul_lib, allow_emulation=True)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.hx_member_score_whitened.argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                                     dp, dp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    assert os.path.exists(hip_lib)
    ctypes.CDLL(hip_lib).hx_member_score_whitened


def _call(c, var, years, obs, W, b0=1, b1=0, n=None):
    """The C ABI directly: -> (return code, error text)."""
    dp = ctypes.POINTER(ctypes.c_double)
    yr = np.ascontiguousarray(years, dtype=np.int32)
    ob = np.ascontiguousarray(obs, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float64)
    out = np.full(c.n_members, -7.0)
    rc = c._lib.hx_member_score_whitened(c._h, var, yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                         ob.ctypes.data_as(dp), W.ctypes.data_as(dp),
                                         yr.size if n is None else n, b0, b1, out.ctypes.data_as(dp))
    assert (out == -7.0).all()      # (every call of this file is refused: nothing is written)
    return rc, c._lib.hx_last_error().decode()


def test_the_emulation_checks_every_argument_then_refuses_by_name(emul_lib):
    for devices in (None, [0, 0]):
        c = _core(5, emul_lib, devices=devices)
        years = np.arange(1750, 1760)
        obs = np.linspace(0.0, 1.0, 10)
        W = np.tril(np.ones((10, 10)))
        # before the core has run (a recorded output has no current date to be inside of yet, or no rows)
        rc, msg = _call(c, b"global_tas", [1745], [0.0], [[1.0]])
        assert rc != 0 and msg.startswith(FN + ":"), msg
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        dp = ctypes.POINTER(ctypes.c_double)
        p = obs.ctypes.data_as(dp)
        ip = np.ascontiguousarray(years, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        for args in ((None, ip, p, p, 1, 1, 0, p), (b"global_tas", None, p, p, 1, 1, 0, p),
                     (b"global_tas", ip, None, p, 1, 1, 0, p), (b"global_tas", ip, p, None, 1, 1, 0, p),
                     (b"global_tas", ip, p, p, 1, 1, 0, None)):
            assert c._lib.hx_member_score_whitened(c._h, *args) != 0
            assert c._lib.hx_last_error().decode() == FN + ": null argument"
        for n in (0, -1, NMAX + 1, 2 ** 31 - 1):
            rc, msg = _call(c, b"global_tas", years, obs, W, n=n)
            assert rc != 0 and msg == FN + ": n must lie in 1..256", (n, msg)
        for bad in (np.nan, np.inf, -np.inf):
            o = obs.copy()
            o[7] = bad
            rc, msg = _call(c, b"global_tas", years, o, W)
            assert rc != 0 and msg.startswith(FN + ": an observation is NaN or infinite"), msg
        for (i, k), bad in (((9, 0), np.nan), ((4, 4), np.inf), ((0, 0), -np.inf), ((9, 8), np.nan)):
            Wb = W.copy()
            Wb[i, k] = bad
            rc, msg = _call(c, b"global_tas", years, obs, Wb)
            assert rc != 0 and msg.startswith(FN + ": an entry of whiten on or below the diagonal is NaN or infinite"), msg
        for yrs in ([1744] + list(years[1:]), list(years[:-1]) + [1761], [2 ** 31 - 1] * 10, [-2 ** 31] * 10):
            rc, msg = _call(c, b"global_tas", yrs, obs, W)
            assert rc != 0 and msg == FN + ": dates must lie between startDate and the current date", msg
        for b0, b1 in ((1744, 1750), (1750, 1761), (-2 ** 31, 1750), (1750, 2 ** 31 - 1)):
            rc, msg = _call(c, b"global_tas", years, obs, W, b0, b1)
            assert rc != 0 and msg == FN + ": the reference period must lie between startDate and the current date", msg
        rc, msg = _call(c, b"no_such_variable", years, obs, W)
        assert rc != 0 and msg.startswith(FN + ":") and "no_such_variable" in msg, msg
        rc, msg = _call(c, b"RF_tot", years, obs, W)          # (a capability that is not recorded)
        assert rc != 0 and msg.startswith(FN + ":"), msg
        # a NaN (anything) in the UPPER triangle passes the validation: what is left is the refusal
        Wu = W.copy()
        Wu[np.triu_indices(10, 1)] = np.nan
        Wu[0, 9] = np.inf
        for b0, b1, yrs in ((1, 0, years), (1745, 1750, years), (1, 0, years[::-1]), (1, 0, [1750] * 10)):
            rc, msg = _call(c, b"global_tas", yrs, obs, Wu, b0, b1)
            assert rc != 0 and msg.startswith(FN + " is not available in the host-emulation build"), msg
        with pytest.raises(E, match=FN + " is not available in the host-emulation build"):
            c.score("global_tas", years, obs, whiten=Wu)
        with pytest.raises(E, match=FN + " is not available in the host-emulation build"):
            c.score("global_tas", years, obs, sigma=0.1, ar1=0.5, baseline=(1745, 1750))
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_a_core_that_has_not_run_is_told_so(emul_lib):
    c = _core(3, emul_lib)
    rc, msg = _call(c, b"slr", [1745], [0.0], [[1.0]])
    assert rc != 0 and msg == FN + ": run the core first", msg
    c.shutdown()


# ---- hector_amd.whiten ------------------------------------------------------------------------------

def test_whiten_is_exact_on_powers_of_two():
    sigma = 2.0 ** np.array([-3, 0, 1, 5, -10, 2])
    W, logdet = hector_amd.whiten(np.diag(sigma ** 2))
    assert np.array_equal(W, np.diag(1.0 / sigma))
    # diag L is sigma exactly, so logdet is this very expression (log det C = 2 (-3+0+1+5-10+2) ln 2 = -10 ln 2)
    assert logdet == 2.0 * float(np.sum(np.log(sigma))) and abs(logdet + 10.0 * np.log(2.0)) <= 8 * 2.0 ** -52
    W1, l1 = hector_amd.whiten([[4.0]])
    assert np.array_equal(W1, [[0.5]]) and l1 == np.log(4.0)


def test_whiten_of_an_ar1_covariance():
    n, rho = 40, 0.6
    years = np.arange(1900, 1900 + n)
    sigma = 0.05 + 0.01 * np.arange(n)
    C = _ar1(years, sigma, rho)
    W, logdet = hector_amd.whiten(C)
    assert W.shape == (n, n) and W.dtype == np.float64
    assert (W[np.triu_indices(n, 1)] == 0.0).all() and not np.signbit(W[np.triu_indices(n, 1)]).any()
    assert (np.diag(W) > 0).all()
    LD = np.longdouble
    resid = np.abs(W.astype(LD) @ C.astype(LD) @ W.astype(LD).T - np.eye(n)).max()
    bound = 8 * n * np.linalg.cond(C, 2) * 2.0 ** -53
    print("whiten AR(1) n = %d: max|W C W^T - I| = %.3g, bound %.3g" % (n, float(resid), bound))
    assert resid <= bound
    sign, ld = np.linalg.slogdet(C)
    assert sign == 1 and abs(logdet - ld) <= 1e-12 * max(1.0, abs(ld)) * n
    # r^T C^-1 r = |W r|^2
    r = np.random.default_rng(1).normal(size=n)
    assert abs(np.sum((W @ r) ** 2) - r @ np.linalg.solve(C, r)) <= 1e-10 * (r @ np.linalg.solve(C, r))


def test_whiten_refuses_what_is_no_covariance():
    C = _ar1(np.arange(5), 1.0, 0.5)
    bad = C.copy()
    bad[0, 1] += 1e-12
    with pytest.raises(E, match="whiten: the covariance is not symmetric"):
        hector_amd.whiten(bad)
    for shape in ((3, 4), (4,), (2, 2, 2), (0, 0)):
        with pytest.raises(E, match="whiten: the covariance must be a square matrix"):
            hector_amd.whiten(np.ones(shape))
    for v in (np.nan, np.inf):
        bad = C.copy()
        bad[2, 2] = v
        with pytest.raises(E, match="whiten: the covariance has a NaN or infinite entry"):
            hector_amd.whiten(bad)
    for M in (-np.eye(3), np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros((2, 2))):
        with pytest.raises(E, match="whiten: the covariance is not positive definite"):
            hector_amd.whiten(M)


# ---- the binding's own checks: raised before the library is called -----------------------------------

class _Spy:
    """Stands in for the library's symbol: records (years, obs, W, n, b0, b1) and returns zeros."""

    def __init__(self):
        self.calls = []

    def __call__(self, h, var, years, obs, W, n, b0, b1, out):
        yr = np.ctypeslib.as_array(years, (n,)).copy()
        ob = np.ctypeslib.as_array(obs, (n,)).copy()
        Wm = np.ctypeslib.as_array(W, (n, n)).copy()
        np.ctypeslib.as_array(out, (1,))[0] = 0.0
        self.calls.append((var, yr, ob, Wm, n, b0, b1))
        return 0


def test_the_bindings_checks_and_what_it_hands_over(emul_lib, monkeypatch):
    c = _core(4, emul_lib)
    spy = _Spy()

    class Lib:       # the loaded library with one symbol replaced
        def __init__(self, lib):
            self._lib = lib
            self.hx_member_score_whitened = spy

        def __getattr__(self, name):
            return getattr(self._lib, name)

    monkeypatch.setattr(c, "_lib", Lib(c._lib))
    years = np.arange(1750, 1760)
    obs = np.linspace(0.0, 1.0, 10)
    C = _ar1(years, 0.1, 0.6)
    for kw, text in ((dict(cov=C, sigma=0.1), "score: sigma goes with ar1 only"),
                     (dict(whiten=np.eye(10), sigma=0.1), "score: sigma goes with ar1 only"),
                     (dict(ar1=0.5), "score: ar1 needs sigma"),
                     (dict(ar1=1.0, sigma=0.1), r"score: ar1 must lie in \[0, 1\)"),
                     (dict(ar1=-0.1, sigma=0.1), r"score: ar1 must lie in \[0, 1\)"),
                     (dict(ar1=np.nan, sigma=0.1), r"score: ar1 must lie in \[0, 1\)"),
                     (dict(cov=C[:9, :9]), "score: cov must be n x n"),
                     (dict(cov=C[0]), "score: cov must be n x n"),
                     (dict(whiten=np.eye(11)), "score: whiten must be n x n"),
                     (dict(cov=C, ar1=0.5, sigma=0.1), "score: cov, ar1 and whiten are mutually exclusive"),
                     (dict(cov=C, whiten=np.eye(10)), "score: cov, ar1 and whiten are mutually exclusive"),
                     (dict(cov=-C), "score: the covariance is not positive definite")):
        with pytest.raises(E, match=text):
            c.score("global_tas", years, obs, **kw)
    with pytest.raises(E, match="score: years and obs must be one-dimensional and of equal length"):
        c.score("global_tas", years, obs[:9], cov=C)
    many = np.arange(1745, 1745 + NMAX + 1)
    for kw in (dict(ar1=0.5, sigma=1.0), dict(cov=np.eye(NMAX + 1)), dict(whiten=np.eye(NMAX + 1))):
        with pytest.raises(E, match="score: more than 256 years"):
            c.score("global_tas", many, np.zeros(NMAX + 1), **kw)
    nan_obs = obs.copy()
    nan_obs[[3, 8]] = np.nan
    with pytest.raises(E, match="score: a NaN observation cannot be skipped under whiten"):
        c.score("global_tas", years, nan_obs, whiten=np.eye(10))
    with pytest.raises(E, match="score: no observation is left"):
        c.score("global_tas", years, np.full(10, np.nan), cov=C)
    assert spy.calls == []
    # NaN observations leave before the factorisation: the W handed over is whiten() of the sub-matrix
    keep = ~np.isnan(nan_obs)
    sig = 0.05 + 0.01 * np.arange(10)
    for kw, Cfull in ((dict(cov=C), C), (dict(ar1=0.6, sigma=0.1), C), (dict(ar1=0.3, sigma=sig), _ar1(years, sig, 0.3))):
        spy.calls.clear()
        out, used = c.score("global_tas", years, nan_obs, baseline=(1746, 1749), return_used=True, **kw)
        (var, yr, ob, Wm, n, b0, b1), = spy.calls
        assert used == n == 8 and var == b"global_tas" and (b0, b1) == (1746, 1749) and out.shape == (4,)
        assert np.array_equal(yr, years[keep]) and np.array_equal(ob, nan_obs[keep])
        assert np.array_equal(Wm, hector_amd.whiten(Cfull[np.ix_(keep, keep)])[0])
    # more than 256 years of which at most 256 are observed is a call; a ready W goes through untouched
    spy.calls.clear()
    o = np.zeros(NMAX + 1)
    o[5] = np.nan
    _, used = c.score("global_tas", many, o, ar1=0.2, sigma=1.0, return_used=True)
    assert used == NMAX and spy.calls[0][4] == NMAX and (spy.calls[0][5], spy.calls[0][6]) == (1, 0)
    spy.calls.clear()
    Wr = np.tril(np.random.default_rng(2).normal(size=(10, 10)))
    Wr[np.triu_indices(10, 1)] = np.nan
    c.score("global_tas", years[::-1], obs, whiten=Wr)
    assert np.array_equal(spy.calls[0][3], Wr, equal_nan=True) and np.array_equal(spy.calls[0][1], years[::-1])
    monkeypatch.undo()
    # without the new keywords the old symbol is called, as before
    c.run(1760)
    a = c.score("global_tas", years, obs, sigma=0.1, baseline=(1745, 1750))
    x = c.fetchvars("global_tas", (1745, 1760))
    base = np.zeros(4)
    for y in range(6):
        base = base + x[y]
    base = base / 6.0
    chi = np.zeros(4)
    for i, y in enumerate(years):
        r = ((x[y - 1745] - base) - obs[i]) / 0.1
        chi = chi + r * r
    assert np.array_equal(a, chi)
    c.shutdown()
