"""TEST INFRASTRUCTURE ONLY: what tests/test_devmath_emulation.py (host build of the probe) and
tests/test_gpu_devmath.py (gfx950 build) have in common -- the loader of a probe library
(devmath_probe.hip through ctypes, no torch), the error measures against
tests/golden/devmath_reference.npz and the checks themselves.  tools/devmath_report.py uses the
same measures for profiles/devmath_report.json.

An error in ulps is (got - ref_hi) / ulp(ref_hi) - ref_lo (tools/make_devmath_golden.py).

The bounds, and where each comes from (none is taken from what the code under test gives):

  exp, every form        1 ulp      hx_dev_math.h ("agree with libm to ~1 ulp"): the reduction and the
                                    degree-13 remainder (5e-18) leave the last fma's rounding
  log, every form        1 ulp      hx_dev_math.h ("< 1 ulp")
  hx_sqrt                1 ulp      hx_dev_math.h ("<= 1 ulp"); perfect squares and 4^k exact
  hx_recip               1 ulp      hx_dev_chem.h ("two to 1.1e-16 (<= 1 ulp)"); 2^k exact
  hx_div                 1.5 2^-52  relative: 1 ulp of the reciprocal (<= 2^-52) + the product's rounding
  hx_div_cr              0          hx_dev_chem.h ("the quotient is correctly rounded"): bits of ref_hi
  hx_div1                2e-15      relative, hx_dev_chem.h
  pow_m13, pow_m15       2 2^-52    relative, hx_dev_solver.h's own analysis: the seed's error squared /
                                    cubed away (<= 1e-19), two roundings in the last correction, one in the add
  frozen fraction        1.5e-15    absolute, tests/test_erfc_fit.py's bound on the numpy restatement
  chem_constants_fit     5e-16      relative to the formulas as printed, tests/test_chem_fit.py
                                    (max_double_horner_error_rel < 5e-16)
  formula path           8 2^-53 sum|terms| + 2^-52   relative, per point and constant: the forward error
                                    of the argument's eight or so roundings plus the exponential's ulp"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(ROOT, "tests", "golden", "devmath_reference.npz")
HIP_PROBE = os.path.join(HERE, "libhx_devmath.so")
EMUL_PROBE = os.path.join(HERE, "libhx_devmath_emul.so")

EPS = 2.0 ** -52
# hx_exp_batch<1, 3, 8>, hx_exp_chunks<9, 12, 17>; hx_log_batch<1, 2, 4> + hx_log; frozen fraction <1, 4>
EXP_FORMS = (("hx_exp_batch", 1), ("hx_exp_batch", 3), ("hx_exp_batch", 8),
             ("hx_exp_chunks", 9), ("hx_exp_chunks", 12), ("hx_exp_chunks", 17))
LOG_FORMS = (("hx_log_batch", 1), ("hx_log_batch", 2), ("hx_log_batch", 4), ("hx_log", 1))
FF_FORMS = (("hx_frozen_fraction_batch", 1), ("hx_frozen_fraction_batch", 4))
CHEM_NAMES = tuple("%s.%s" % (b, f) for b in ("HL", "LL") for f in ("K0", "Kw", "rKh", "K1", "K2", "Kb"))
LOG_SPECIAL = np.array([0.0, -0.0, -1.0, -2.5e10, -np.inf, np.nan, np.inf, 1.0])
SQRT_SPECIAL = np.array([0.0, -0.0])

_dp = ctypes.POINTER(ctypes.c_double)


def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulp(y):
    return np.spacing(np.abs(y))


def ulps(got, hi, lo):
    """signed error of got in ulps of the correctly rounded result"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (got - hi) / ulp(hi) - lo


def columns(forms):
    """[(form, N, position, column)]"""
    out, col = [], 0
    for name, n in forms:
        for j in range(n):
            out.append((name, n, j, col + j))
        col += n
    return out


class ProbeError(AssertionError):
    pass


class Probe:
    """One probe library.  Every entry point's return value is checked; after the first non-zero one
    nothing is launched any more and every further call fails at once.  A result is computed once."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.devmath_backend.restype = ctypes.c_char_p
        self.lib.devmath_stride.restype = ctypes.c_int
        self.backend = self.lib.devmath_backend().decode()
        self.stride = self.lib.devmath_stride()
        self.failed = None
        self.launches = 0
        self._cache = {}

    def index(self, n, j):
        """the input that position j of a batch holds in thread i"""
        return (np.arange(n) + self.stride * j) % n

    def call(self, name, ncol, a, b=None, table=None):
        key = (name, table, bits(a).tobytes(), None if b is None else bits(b).tobytes())
        if key in self._cache:
            return self._cache[key]
        if self.failed is not None:
            raise ProbeError("devmath_%s returned hipError_t %d earlier: nothing is launched any more" % self.failed)
        a = np.ascontiguousarray(a, dtype=np.float64)
        n = a.size
        out = np.full((ncol, n), np.nan)
        args = [a.ctypes.data_as(_dp)]
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert b.size == n
            args.append(b.ctypes.data_as(_dp))
        args.append(ctypes.c_int(n))
        if table is not None:
            args.append(ctypes.c_int(int(table)))
        args.append(out.ctypes.data_as(_dp))
        fn = getattr(self.lib, "devmath_" + name)
        fn.restype = ctypes.c_int
        self.launches += 1
        rc = fn(*args)
        if rc != 0:
            self.failed = (name, rc)
            raise ProbeError("devmath_%s returned hipError_t %d" % (name, rc))
        self._cache[key] = out
        return out

    # the operations, on the fixture's inputs
    def exp(self, G, table): return self.call("exp", 50, G["exp_x"], table=table)
    def exp1(self, G): return self.call("exp1", 1, np.concatenate([G["exp_x"], G["exp1_extra_x"]]))[0]
    def log(self, G, table): return self.call("log", 8, G["log_x"], table=table)
    def log1(self, G, table): return self.call("log1", 1, np.concatenate([G["log_x"], LOG_SPECIAL]), table=table)[0]
    def sqrt(self, G): return self.call("sqrt", 1, np.concatenate([G["sqrt_x"], SQRT_SPECIAL]))[0]
    def frozen(self, G): return self.call("frozen", 5, G["frozen_d"])
    def div(self, G): return self.call("div", 4, G["div_a"], G["div_b"])
    def pow13(self, G): return self.call("pow13", 1, G["pow13_x"])[0]
    def pow15(self, G): return self.call("pow15", 1, G["pow15_x"])[0]
    def chem_fit(self, G): return self.call("chem_fit", 12, G["chemfit_TcH"], G["chemfit_TcL"])
    def chem_formula(self, G, table):
        return self.call("chem_formula", 12, G["chemform_TcH"], G["chemform_TcL"], table=table)


OPERATIONS = ("exp.literal", "exp.table", "hx_exp", "log.literal", "log.table", "hx_sqrt", "hx_recip", "hx_div",
              "hx_div_cr", "hx_div1", "pow_m13", "pow_m15", "frozen_fraction", "chem_constants_fit",
              "chem_formula.literal", "chem_formula.table")


def measure(p, G, op):
    """-> dict(err=|error| per output, bound=scalar or array like err, unit=..., x=the input behind each
    output, got=the outputs): the error of one operation over its fixture inputs, every form and position."""
    def forms(out, forms_, x, hi, lo):
        err, xs = [], []
        for _, _, j, col in columns(forms_):
            idx = p.index(x.size, j)
            err.append(np.abs(ulps(out[col], hi[idx], lo[idx]))); xs.append(x[idx])
        return np.array(err), np.array(xs)

    def rel(got, hi, lo):
        return np.abs(ulps(got, hi, lo)) * ulp(hi) / np.abs(hi)

    kind, _, variant = op.partition(".")
    table = variant == "table"
    if kind == "exp":
        got = p.exp(G, table)
        err, x = forms(got, EXP_FORMS, G["exp_x"], G["exp_hi"], G["exp_lo"])
        return dict(err=err, bound=1.0, unit="ulp", x=x, got=got)
    if kind == "hx_exp":
        got = p.exp1(G)[:G["exp_x"].size]
        return dict(err=np.abs(ulps(got, G["exp_hi"], G["exp_lo"])), bound=1.0, unit="ulp", x=G["exp_x"], got=got)
    if kind == "log":
        got = p.log(G, table)
        err, x = forms(got, LOG_FORMS, G["log_x"], G["log_hi"], G["log_lo"])
        return dict(err=err, bound=1.0, unit="ulp", x=x, got=got)
    if kind == "hx_sqrt":
        got = p.sqrt(G)[:G["sqrt_x"].size]
        return dict(err=np.abs(ulps(got, G["sqrt_hi"], G["sqrt_lo"])), bound=1.0, unit="ulp", x=G["sqrt_x"], got=got)
    if kind in ("hx_recip", "hx_div", "hx_div_cr", "hx_div1"):
        d = p.div(G)
        x = np.stack([G["div_a"], G["div_b"]], axis=-1)
        if kind == "hx_recip":
            return dict(err=np.abs(ulps(d[0], G["recip_hi"], G["recip_lo"])), bound=1.0, unit="ulp", x=G["div_b"], got=d[0])
        if kind == "hx_div":
            return dict(err=rel(d[1], G["quot_hi"], G["quot_lo"]), bound=1.5 * EPS, unit="relative", x=x, got=d[1])
        if kind == "hx_div_cr":   # distance from the CORRECTLY ROUNDED quotient: must be none
            return dict(err=np.abs(d[2] - G["quot_hi"]) / ulp(G["quot_hi"]), bound=0.0,
                        unit="ulp from the correctly rounded quotient", x=x, got=d[2])
        return dict(err=rel(d[3], G["quot_hi"], G["quot_lo"]), bound=2e-15, unit="relative", x=x, got=d[3])
    if kind in ("pow_m13", "pow_m15"):
        k = kind[-2:]
        got = p.pow13(G) if k == "13" else p.pow15(G)
        return dict(err=rel(got, G["pow%s_hi" % k], G["pow%s_lo" % k]), bound=2 * EPS, unit="relative",
                    x=G["pow%s_x" % k], got=got)
    if kind == "frozen_fraction":
        got = p.frozen(G)
        hi, lo, d = G["frozen_hi"], G["frozen_lo"], G["frozen_d"]
        err, x = [], []
        for _, _, j, col in columns(FF_FORMS):
            idx = p.index(d.size, j)
            err.append(np.abs(ulps(got[col], hi[idx], lo[idx]) * ulp(hi[idx]))); x.append(d[idx])
        return dict(err=np.array(err), bound=1.5e-15, unit="absolute", x=np.array(x), got=got)
    if kind == "chem_constants_fit":
        got = p.chem_fit(G)
        x = np.broadcast_to(np.stack([G["chemfit_TcH"], G["chemfit_TcL"]], axis=-1), (12,) + (G["chemfit_TcH"].size, 2))
        return dict(err=rel(got, G["chemfit_hi"], G["chemfit_lo"]), bound=5e-16, unit="relative", x=x, got=got)
    if kind == "chem_formula":
        got = p.chem_formula(G, table)
        x = np.broadcast_to(np.stack([G["chemform_TcH"], G["chemform_TcL"]], axis=-1), (12,) + (G["chemform_TcH"].size, 2))
        bound = 8 * 2.0 ** -53 * G["chemform_sumabs"].astype(np.float64) + EPS
        return dict(err=rel(got, G["chemform_hi"], G["chemform_lo"]), bound=bound, unit="relative", x=x, got=got)
    raise KeyError(op)


def worst(m):
    """the largest error of a measure, as a share of its bound where the bound varies, and its input"""
    err = np.where(np.isnan(m["err"]), np.inf, m["err"])
    score = err / m["bound"] if np.ndim(m["bound"]) else err
    at = tuple(int(v) for v in np.unravel_index(np.argmax(score), score.shape))
    return float(err[at]), np.atleast_1d(m["x"][at]).tolist(), at


# ---- the checks ---------------------------------------------------------------------------------
def check_bound(p, G, op):
    m = measure(p, G, op)
    w, x, at = worst(m)
    print("%s [%s]: worst %.4g %s at %r (output %r)" % (op, p.backend, w, m["unit"], x, at))
    bad = ~(m["err"] <= m["bound"])
    assert not bad.any(), "%s: %d outputs over the bound; worst %.6g %s at input %r (output %r)" % (
        op, int(bad.sum()), w, m["unit"], x, at)


def exp_mismatches(p, G):
    """outputs of the exp forms whose bits differ from hx_exp_batch<1> (literals) of the same input"""
    lit, tab = p.exp(G, False), p.exp(G, True)
    ref, n = lit[0], G["exp_x"].size
    bad = {}
    for name, N, j, col in columns(EXP_FORMS):
        idx = p.index(n, j)
        for what, out in (("literal", lit), ("table", tab)):
            k = int((bits(out[col]) != bits(ref[idx])).sum())
            if k:
                bad["%s<%d>[%d].%s" % (name, N, j, what)] = k
    k = int((bits(p.exp1(G)[:n]) != bits(ref)).sum())
    if k:
        bad["hx_exp"] = k
    return bad


def log_mismatches(p, G):
    """... of the log forms from hx_log (literals)"""
    lit, tab = p.log(G, False), p.log(G, True)
    ref, n = lit[7], G["log_x"].size
    bad = {}
    for name, N, j, col in columns(LOG_FORMS):
        idx = p.index(n, j)
        for what, out in (("literal", lit), ("table", tab)):
            k = int((bits(out[col]) != bits(ref[idx])).sum())
            if k:
                bad["%s<%d>[%d].%s" % (name, N, j, what)] = k
    for what, table in (("literal", False), ("table", True)):
        k = int((bits(p.log1(G, table)[:n]) != bits(ref)).sum())
        if k:
            bad["hx_log (alone).%s" % what] = k
    return bad


def check_exp_bitwise(p, G):
    """Every position of every batch and chunk size, table and literal, and hx_exp: the bits of
    hx_exp_batch<1>.  Every operation of hx_exp_batch is an explicit fma, rint or ldexp, so the
    equality holds whatever the compiler does with the N chains."""
    assert exp_mismatches(p, G) == {}


def check_log_bitwise(p, G):
    """hx_log_batch<N> positions against hx_log, table forms against literal forms."""
    assert log_mismatches(p, G) == {}


def check_exp_special(p, G):
    n = G["exp_x"].size
    e = p.exp1(G)
    m746, m800, minf = e[n:n + 3]
    assert minf == 0.0 and not np.signbit(minf)                       # exp(-inf) = 0 like libm
    assert bits(m800) == bits(m746) and bits(minf) == bits(m746)      # x <= -746: hx_exp(-746)
    zeros = np.flatnonzero(G["exp_x"] == 0.0)
    assert zeros.size == 2                                            # 0 and -0
    assert (e[zeros] == 1.0).all()
    for table in (False, True):
        out = p.exp(G, table)
        for _, _, j, col in columns(EXP_FORMS):
            idx = p.index(n, j)
            assert (out[col][np.isin(idx, zeros)] == 1.0).all()       # exp(0) = 1 exactly, everywhere


def check_log_special(p, G):
    n = G["log_x"].size
    for table in (False, True):
        out = p.log1(G, table)
        z, mz, neg1, neg2, ninf, nan, pinf, one = out[n:]
        assert z == -np.inf and mz == -np.inf                          # log(0) = log(-0) = -inf
        assert np.isnan([neg1, neg2, ninf, nan]).all()                 # x < 0 and NaN: NaN
        assert pinf == np.inf                                          # log(+inf) = +inf
        assert one == 0.0                                              # log(1) = 0 exactly
        full = p.log(G, table)
        ones = np.flatnonzero(G["log_x"] == 1.0)
        assert ones.size >= 1
        for _, _, j, col in columns(LOG_FORMS):
            assert (full[col][np.isin(p.index(n, j), ones)] == 0.0).all()


def check_sqrt_exact(p, G):
    n = G["sqrt_x"].size
    out = p.sqrt(G)
    ex = G["sqrt_exact"]
    assert ex.sum() == 71 and (G["sqrt_lo"][ex] == 0).all()
    assert (bits(out[:n][ex]) == bits(G["sqrt_hi"][ex])).all()         # m^2 and 4^k: exact
    assert (bits(out[n:]) == bits(SQRT_SPECIAL)).all()                 # sqrt(0) = 0, sqrt(-0) = -0, bitwise


def check_div_exact(p, G):
    d = p.div(G)
    p2, eq = G["div_pow2"], G["div_exactq"]
    assert p2.sum() == 40 and eq.sum() == 100
    assert (G["recip_lo"][p2] == 0).all() and (G["quot_lo"][eq] == 0).all()
    assert (bits(d[0][p2]) == bits(G["recip_hi"][p2])).all()           # 1 / 2^k
    assert (bits(d[2][eq]) == bits(G["quot_hi"][eq])).all()            # a = q b: the quotient itself


def check_frozen_edges(p, G):
    d, out = G["frozen_d"], p.frozen(G)
    for _, _, j, col in columns(FF_FORMS):
        x = d[p.index(d.size, j)]
        assert (x <= -40).sum() == 2 and (x >= 40).sum() == 2
        assert (out[col][x <= -40] == 1.0).all()                       # far below 0 degC: frozen
        assert (out[col][x >= 40] == 0.0).all()                        # far above: thawed
        tiny = np.abs(x) <= 1e-300
        assert tiny.sum() == 4                                         # +-0, +-1e-300
        assert (np.abs(out[col][tiny] - 0.5) <= 1.5e-15).all()


CHECKS = (check_exp_bitwise, check_log_bitwise, check_exp_special, check_log_special, check_sqrt_exact,
          check_div_exact, check_frozen_edges)
