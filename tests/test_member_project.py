"""hx_member_project (Core.project, CoMoments.scores): the parts that need no GPU.

The contraction runs on the fp64 matrix pipe, so the host-emulation build refuses the verb by name --
after the argument checks, which are therefore testable here one by one, through the raw C ABI.  The
binding's own shape and range checks are raised before the library is called: a spy in the symbol's
place shows that, and what a valid call hands over.  The GPU part is tests/test_gpu_project.py.
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
FN = "hx_member_project"
MAX_OUT, MAX_YEARS = 64, 1024


def _core(n, lib, **kw):
    c = hector_amd.Core(SCENARIO, n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    return c


def test_the_header_documents_the_symbol_and_the_libraries_export_it(emul_lib, hip_lib):
    from hector_amd import _lib
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert re.search(r"\bint hx_member_project\(hx_core \*core, const char \*capability, const int \*years, "
                     r"const double \*center,\s+const double \*basis, int n, int m, int base_year0, "
                     r"int base_year1, double \*out\);", text)
    assert re.search(r"^#define HX_PROJECT_MAX_OUT\s+64$", text, re.M)
    assert re.search(r"^#define HX_PROJECT_MAX_YEARS\s+1024$", text, re.M)
    assert text.index("int hx_member_score_whitened(") < text.index("int hx_member_project(")
    doc = text[text.index("onto a caller's basis"):text.index("int hx_member_project(")]
    for phrase in ("r_k = (x(years[k], member) - base(member)) - center[k]",
                   "out[j * n_members + member] = sum_{k < n} basis[j * n + k] * r_k",
                   "any order, repeats allowed", "ONE\n * division", "two IEEE subtractions",
                   "center == NULL means zeros", "- 0.0", "1 <= n <= HX_PROJECT_MAX_YEARS",
                   "1 <= m <= HX_PROJECT_MAX_OUT", "NO skipping", "NaN in ALL m outputs",
                   "a zero coefficient does not mask it", "no other member is affected",
                   "NOT part of the definition", "(n + 2) 2^-53 s_j", "ONE fixed order",
                   "nor on which other members exist", "which other rows basis has", "2 n m n_members flops",
                   "not prepared, spun up or dirtied", "shard by shard", "host-emulation build refuses"):
        assert phrase in doc, phrase
    assert FN in _lib.ABI_SYMBOLS
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    assert "int %s(" % FN in abi and "%s: null argument" % FN in abi
    post = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_post.h")).read()
    for name, value in (("HXP_TILE", 16), ("HXP_MT", 4), ("HXP_MAX_OUT", MAX_OUT), ("HXP_MAX_YEARS", MAX_YEARS)):
        assert re.search(r"^#define %s %d\b" % (name, value), post, re.M), name
    kernel = post[post.index("void hx_project_kernel("):]
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in kernel
    launch = post[post.index("hipError_t hx_launch_project("):]
    assert [int(a) for a in re.findall(r"HXP_CASE\((\d+)\);", launch)] == [1, 2, 3, 4]
    assert "void hx_project_pack(" in post
    lib = _lib.load(emul_lib, allow_emulation=True)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.hx_member_project.argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), dp, dp,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp]
    assert os.path.exists(hip_lib)
    ctypes.CDLL(hip_lib).hx_member_project


def _call(c, var, years, center, basis, b0=1, b1=0, n=None, m=None):
    """The C ABI directly: -> (return code, error text)."""
    dp = ctypes.POINTER(ctypes.c_double)
    yr = np.ascontiguousarray(years, dtype=np.int32)
    ce = None if center is None else np.ascontiguousarray(center, dtype=np.float64)
    B = np.ascontiguousarray(np.atleast_2d(basis), dtype=np.float64)
    out = np.full((MAX_OUT, c.n_members), -7.0)
    rc = c._lib.hx_member_project(c._h, var, yr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                  None if ce is None else ce.ctypes.data_as(dp), B.ctypes.data_as(dp),
                                  yr.size if n is None else n, B.shape[0] if m is None else m, b0, b1,
                                  out.ctypes.data_as(dp))
    assert (out == -7.0).all()      # (every call of this file is refused: nothing is written)
    return rc, c._lib.hx_last_error().decode()


def test_the_emulation_checks_every_argument_then_refuses_by_name(emul_lib):
    for devices in (None, [0, 0]):
        c = _core(5, emul_lib, devices=devices)
        years = np.arange(1750, 1760)
        center = np.linspace(0.0, 1.0, 10)
        B = np.arange(30.0).reshape(3, 10) - 7.0
        # before the core has run (a recorded output has no current date to be inside of yet, or no rows)
        rc, msg = _call(c, b"global_tas", [1745], [0.0], [[1.0]])
        assert rc != 0 and msg.startswith(FN + ":"), msg
        c.run(1760)
        before = c.fetchvars("global_tas", (1745, 1760))
        dp = ctypes.POINTER(ctypes.c_double)
        p = center.ctypes.data_as(dp)
        ip = np.ascontiguousarray(years, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        for args in ((None, ip, p, p, 1, 1, 1, 0, p), (b"global_tas", None, p, p, 1, 1, 1, 0, p),
                     (b"global_tas", ip, p, None, 1, 1, 1, 0, p), (b"global_tas", ip, p, p, 1, 1, 1, 0, None)):
            assert c._lib.hx_member_project(c._h, *args) != 0
            assert c._lib.hx_last_error().decode() == FN + ": null argument"
        for n in (0, -1, MAX_YEARS + 1, 2 ** 31 - 1):
            rc, msg = _call(c, b"global_tas", years, center, B, n=n)
            assert rc != 0 and msg == FN + ": n must lie in 1..1024", (n, msg)
        for m in (0, -1, MAX_OUT + 1, 2 ** 31 - 1):
            rc, msg = _call(c, b"global_tas", years, center, B, m=m)
            assert rc != 0 and msg == FN + ": m must lie in 1..64", (m, msg)
        for bad in (np.nan, np.inf, -np.inf):
            o = center.copy()
            o[7] = bad
            rc, msg = _call(c, b"global_tas", years, o, B)
            assert rc != 0 and msg.startswith(FN + ": an entry of center is NaN or infinite"), msg
        for (j, k), bad in (((2, 0), np.nan), ((1, 4), np.inf), ((0, 0), -np.inf), ((2, 9), np.nan)):
            Bb = B.copy()
            Bb[j, k] = bad
            rc, msg = _call(c, b"global_tas", years, center, Bb)
            assert rc != 0 and msg == FN + ": an entry of basis is NaN or infinite", msg
            rc, msg = _call(c, b"global_tas", years, None, Bb)
            assert rc != 0 and msg == FN + ": an entry of basis is NaN or infinite", msg
        for yrs in ([1744] + list(years[1:]), list(years[:-1]) + [1761], [2 ** 31 - 1] * 10, [-2 ** 31] * 10):
            rc, msg = _call(c, b"global_tas", yrs, center, B)
            assert rc != 0 and msg == FN + ": dates must lie between startDate and the current date", msg
        for b0, b1 in ((1744, 1750), (1750, 1761), (-2 ** 31, 1750), (1750, 2 ** 31 - 1)):
            rc, msg = _call(c, b"global_tas", years, center, B, b0, b1)
            assert rc != 0 and msg == FN + ": the reference period must lie between startDate and the current date", msg
        rc, msg = _call(c, b"no_such_variable", years, center, B)
        assert rc != 0 and msg.startswith(FN + ":") and "no_such_variable" in msg, msg
        rc, msg = _call(c, b"RF_tot", years, center, B)          # (a capability that is not recorded)
        assert rc != 0 and msg.startswith(FN + ":"), msg
        # valid calls: what is left is the refusal, by name -- a NULL center is one of them
        for b0, b1, yrs, ce in ((1, 0, years, center), (1745, 1750, years, None), (1, 0, years[::-1], center),
                                (1, 0, [1750] * 10, None)):
            rc, msg = _call(c, b"global_tas", yrs, ce, B, b0, b1)
            assert rc != 0 and msg.startswith(FN + " is not available in the host-emulation build"), msg
        with pytest.raises(E, match=FN + " is not available in the host-emulation build"):
            c.project("global_tas", years, B, center=center, baseline=(1745, 1750))
        with pytest.raises(E, match=FN + " is not available in the host-emulation build"):
            c.project("global_tas", years, B[0])
        assert np.array_equal(before, c.fetchvars("global_tas", (1745, 1760)))
        assert (c.status() == 0).all()
        c.shutdown()


def test_a_core_that_has_not_run_is_told_so(emul_lib):
    c = _core(3, emul_lib)
    rc, msg = _call(c, b"slr", [1745], None, [[1.0]])
    assert rc != 0 and msg == FN + ": run the core first", msg
    c.shutdown()


# ---- the binding's own checks: raised before the library is called -----------------------------------

class _Spy:
    """Stands in for the library's symbol: records what it is handed and writes j + 1 into row j."""

    def __init__(self):
        self.calls = []

    def __call__(self, h, var, years, center, basis, n, m, b0, b1, out):
        yr = np.ctypeslib.as_array(years, (n,)).copy()
        ce = None if center is None else np.ctypeslib.as_array(center, (n,)).copy()
        B = np.ctypeslib.as_array(basis, (m, n)).copy()
        o = np.ctypeslib.as_array(out, (m, 4))
        o[:] = np.arange(1.0, m + 1.0)[:, None]
        self.calls.append((var, yr, ce, B, n, m, b0, b1))
        return 0


def _with_spy(c, monkeypatch):
    spy = _Spy()

    class Lib:       # the loaded library with one symbol replaced
        def __init__(self, lib):
            self._lib = lib
            self.hx_member_project = spy

        def __getattr__(self, name):
            return getattr(self._lib, name)

    monkeypatch.setattr(c, "_lib", Lib(c._lib))
    return spy


def test_the_bindings_checks_and_what_it_hands_over(emul_lib, monkeypatch):
    c = _core(4, emul_lib)
    spy = _with_spy(c, monkeypatch)
    years = np.arange(1750, 1760)
    B = np.arange(30.0).reshape(3, 10)
    for basis, kw, text in ((B[:, :9], {}, r"project: basis must be \[m, n\]"),
                            (np.zeros((2, 3, 10)), {}, r"project: basis must be \[m, n\]"),
                            (np.zeros((0, 10)), {}, r"project: basis must be \[m, n\]"),
                            (np.zeros(9), {}, r"project: basis must be \[m, n\]"),
                            (np.zeros((MAX_OUT + 1, 10)), {}, "project: more than 64 basis rows"),
                            (B, dict(center=np.zeros(9)), "project: center must have one entry per year"),
                            (B, dict(center=np.zeros((10, 1))), "project: center must have one entry per year"),
                            (B, dict(center=np.where(np.arange(10) == 3, np.nan, 0.0)), "project: center has a NaN or infinite entry"),
                            (B, dict(center=np.where(np.arange(10) == 9, np.inf, 0.0)), "project: center has a NaN or infinite entry"),
                            (np.where(B == 17.0, np.nan, B), {}, "project: basis has a NaN or infinite entry"),
                            (np.where(B == 0.0, -np.inf, B), {}, "project: basis has a NaN or infinite entry")):
        with pytest.raises(E, match=text):
            c.project("global_tas", years, basis, **kw)
    with pytest.raises(E, match="project: years must be one-dimensional and not empty"):
        c.project("global_tas", [], np.zeros((1, 0)))
    with pytest.raises(E, match="project: years must be one-dimensional and not empty"):
        c.project("global_tas", years.reshape(2, 5), B)
    many = np.arange(1745, 1745 + MAX_YEARS + 1)
    with pytest.raises(E, match="project: more than 1024 years"):
        c.project("global_tas", many, np.zeros((2, MAX_YEARS + 1)))
    assert spy.calls == []
    # a valid call: what is handed over, and the shapes that come back
    center = np.linspace(-1.0, 1.0, 10)
    out = c.project("global_tas", years[::-1], B, center=center, baseline=(1746, 1749))
    (var, yr, ce, Bm, n, m, b0, b1), = spy.calls
    assert var == b"global_tas" and (n, m, b0, b1) == (10, 3, 1746, 1749)
    assert np.array_equal(yr, years[::-1]) and np.array_equal(ce, center) and np.array_equal(Bm, B)
    assert out.shape == (3, 4) and np.array_equal(out, np.arange(1.0, 4.0)[:, None] * np.ones(4))
    spy.calls.clear()
    out = c.project("global_tas", years, B.T[:, 1])          # a one-dimensional (strided) basis, no centre, no baseline
    (var, yr, ce, Bm, n, m, b0, b1), = spy.calls
    assert ce is None and (n, m) == (10, 1) and b0 > b1 and np.array_equal(Bm, B.T[:, 1][None, :])
    assert out.shape == (4,) and (out == 1.0).all()
    spy.calls.clear()
    c.project("global_tas", np.full(MAX_YEARS, 1750), np.ones((MAX_OUT, MAX_YEARS)))     # the limits themselves
    assert (spy.calls[0][4], spy.calls[0][5]) == (MAX_YEARS, MAX_OUT)
    c.shutdown()


def test_comoments_scores_is_project_of_the_patterns(emul_lib, monkeypatch):
    c = _core(4, emul_lib)
    spy = _with_spy(c, monkeypatch)
    rng = np.random.default_rng(3)
    na = 6
    d = rng.normal(size=(na, 50))
    shift = d.min(axis=1)
    dd = d - shift[:, None]
    sums = np.stack([dd.sum(axis=1), (dd * dd).sum(axis=1)], axis=1)
    years = np.arange(1900, 1900 + na)
    sym = hector_amd.CoMoments(shift, sums, shift, sums, dd @ dd.T, 50, 50, years, years, symmetric=True)
    out = sym.scores(c, "global_tas", 2)
    (var, yr, ce, Bm, n, m, b0, b1), = spy.calls
    assert var == b"global_tas" and (n, m) == (na, 2) and b0 > b1 and out.shape == (2, 4)
    assert np.array_equal(yr, years) and np.array_equal(ce, sym.mean_a) and np.array_equal(Bm, sym.pca(2)[2])
    spy.calls.clear()
    asym = hector_amd.CoMoments(shift, sums, shift, sums, dd @ dd.T, 50, 50, years, years, symmetric=False)
    with pytest.raises(E, match=r"CoMoments.pca: needs a symmetric result \(comoments\(var, dates\) without var_b\)"):
        asym.scores(c, "global_tas", 2)
    with pytest.raises(E, match=r"CoMoments.pca: k must lie in 1..6"):
        sym.scores(c, "global_tas", 7)
    assert spy.calls == []
    c.shutdown()
