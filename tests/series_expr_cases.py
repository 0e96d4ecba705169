"""hx_series_eval (Core.derive_expr, hector_amd.expr): the bodies and the case table that
tests/test_series_expr.py runs on the host-emulation build and tests/test_gpu_series_expr.py on the
product library.  Not collected itself.

include/hector_amd.h fixes every instruction in IEEE double without fused multiply-add, and
`Program.numpy` restates that table literally on fetchvars output, so everything but LOG and EXP is
compared BIT FOR BIT (`same`: the NaNs in the same places, every other value the same 64 bits, the
sign of zero included).  LOG and EXP are held to np.longdouble results of the same arguments, in
ulps of the double result.

The core: S unsorted, so with member sorting on the lane order is a true permutation; endDate 2300
but run to 1790 -- 46 rows, no multiple of a batch of 4 or 8 rows, and rows behind the valid end
exist.  300 members on the GPU are two 256-lane blocks, the second with 44 real lanes and a partial
last wavefront; the emulation takes 70.
"""
import ctypes

import numpy as np
import pytest

import hector_amd
from hector_amd import expr

E = hector_amd.HectorAmdError
RUN_TO = 1790
OUTPUTS = ("CO2_concentration", "global_tas", "pH", "ocean_tas", "slr", "RF_N2O")
FN = "hx_series_eval"

# The largest LOG / EXP error against np.longdouble, in ulps of the double result, that `_check_log_exp`
# may find.  Host emulation (glibc): 1 -- glibc documents its double exp and log below 1 ulp.  GPU: the
# next whole ulp above what was measured on these very arguments on an MI355X (exp 0.799, log 0.500:
# profiles/post_summaries.md), and never above 3, OpenCL's bound for both functions in double.
LOG_EXP_ULP = {"host-emulation": 1.0, "hip": 1.0}


def params(n):
    k = np.arange(n)
    S = 1.5 + 4.5 * np.fmod(k * 0.6180339887498949, 1.0)          # unsorted
    q10 = 1.0 + 2.0 * np.fmod(k * 0.7548776662466927, 1.0)
    return S, q10


def make_core(n, lib, run_to=RUN_TO, **kw):
    c = hector_amd.Core(n_members=n, lib_path=lib, allow_emulation=True, **kw)
    S, q10 = params(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    c.set_outputs(list(OUTPUTS))
    if run_to:
        c.run(run_to)
    return c


def same(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN pattern", int((gn != rn).sum()))
    g, r = got[~gn].view(np.uint64), ref[~rn].view(np.uint64)
    assert np.array_equal(g, r), (what, int((g != r).sum()), "values differ in their bits")


def fetch(core, names, to=RUN_TO):
    return {v: core.fetchvars(v, (core.strtdate, to)) for v in names}


def run(core, text, bind=None, values=None, name="z", params_=None, to=RUN_TO):
    """derive_expr(text) == Program.numpy of the fetched operands, bit for bit -> the block"""
    p = expr.compile(text, bind)
    if values is None:
        values = fetch(core, sorted({v for v, _ in p.vars}), to)
    ref = p.numpy(values, core.strtdate, params=params_)
    core.derive_expr(name, p)
    got = core.fetchvars(name, (core.strtdate, to))
    same(got, ref, text)
    return got


# Rows behind a series' valid end cannot be fetched: fetchvars refuses a date beyond valid_to, and so
# does every verb.  That they hold NaN is read from the block itself, through the pointer
# hx_device_var returns -- host memory in the emulation, device memory on the GPU, copied by the HIP
# runtime the product library has already brought into the process (tests/test_gpu_quantiles.py
# writes rows the same way).
def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in the process")


def whole_block(core, name):
    """Every row of a series' block, startDate..endDate, valid or not -> [years, n_members]"""
    ptr, npad = core.device_var(name)
    ns = core.enddate - core.strtdate + 1
    buf = np.empty((ns, npad))
    if core.backend == "hip":
        hip = _hip_runtime()
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipMemcpy.restype = ctypes.c_int
        assert hip.hipMemcpy(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), buf.nbytes, 2) == 0
    else:
        ctypes.memmove(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), buf.nbytes)
    return buf[:, core.lane_of_member()]


# ---- 1. the special-value matrix ---------------------------------------------------------------------

TINY = 5e-324
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, TINY, -TINY, 1e308, -1e308, 2.5, 3.0])
UNARY = ("-{a}", "abs({a})", "sqrt({a})")
BINARY = ("{a} + {b}", "{a} - {b}", "{a} * {b}", "{a} / {b}", "minimum({a}, {b})", "maximum({a}, {b})",
          "{a} < {b}", "{a} <= {b}", "{a} > {b}", "{a} >= {b}", "{a} == {b}", "{a} != {b}", "ifnan({a}, {b})",
          "{a} & {b}", "{a} | {b}")
TERNARY = ("where({a}, {b}, {c})", "where({b}, {a}, {c})", "where({c}, {b}, {a})", "where({a}, {b}, nan_)",
           "where({a}, nan_, {b})", "where({a} == {a}, {b}, nan_)")


def special_operands(core):
    """A member vector and a year vector that cycle through SPECIAL with the coprime strides 5 and 7
    of its 13 values: rows 0..12 x members 0..12 already hold every ordered pair.  Held as the series
    mm and yy, so that VAR operands carry them too."""
    n, y0 = core.n_members, core.strtdate
    m = SPECIAL[(5 * np.arange(n)) % 13]
    yv = SPECIAL[(7 * np.arange(RUN_TO - y0 + 1) + 3) % 13]
    bind = {"M": m, "Y": (y0, yv), "nan_": float("nan")}
    tas = fetch(core, ["global_tas"])
    # (global_tas is finite: the condition is 1.0 and WHERE passes its second operand through)
    vals = dict(tas)
    vals["mm"] = run(core, "where(global_tas == global_tas, M, nan_)", bind, tas, name="mm")
    vals["yy"] = run(core, "where(global_tas == global_tas, Y, nan_)", bind, tas, name="yy")
    same(vals["mm"], np.broadcast_to(m[None, :], vals["mm"].shape), "mm")
    same(vals["yy"], np.broadcast_to(yv[:, None], vals["yy"].shape), "yy")
    pairs = {(a.tobytes(), b.tobytes()) for a, b in zip(vals["mm"].ravel().view(np.uint64),
                                                        vals["yy"].ravel().view(np.uint64))}
    assert len(pairs) == 13 * 13      # every ordered pair meets on the grid
    return bind, vals


def check_special_values(core):
    bind, vals = special_operands(core)
    for f in UNARY:
        for a in ("mm", "yy", "lag(mm, 2)"):
            run(core, f.format(a=a), bind, vals)
        run(core, "ifnan(%s, global_tas)" % f.format(a="M"), bind, vals)     # on a MEMBER and a YEARVEC operand
        run(core, "ifnan(%s, global_tas)" % f.format(a="Y"), bind, vals)
    for f in BINARY:
        for a, b in (("mm", "yy"), ("yy", "mm"), ("M", "yy"), ("mm", "Y"), ("Y", "mm"), ("mm", "mm")):
            run(core, f.format(a=a, b=b), bind, vals)
    for f in TERNARY:
        for a, b, c in (("mm", "yy", "global_tas"), ("yy", "mm", "lag(yy, 1)"), ("M", "yy", "Y")):
            run(core, f.format(a=a, b=b, c=c), bind, vals)
    core.drop_series("mm").drop_series("yy").drop_series("z")


def check_log_exp(core):
    """LOG and EXP against np.longdouble (a 64-bit significand) on the arguments of the issue's
    ranges -- exp over +-700, log over 1e-300..1e300, as MEMBER (+ or *) YEARVEC -- in ulps of the
    double result; the special arguments exactly.  -> the largest errors found (exp, log)."""
    assert np.finfo(np.longdouble).nmant >= 63
    n, y0 = core.n_members, core.strtdate
    ny = RUN_TO - y0 + 1
    rng = np.random.default_rng(11)
    tas = fetch(core, ["global_tas"])
    bound = LOG_EXP_ULP[core.backend]
    worst = {}
    for fn, m, yv, text in (("exp", rng.uniform(-650, 650, n), rng.uniform(-50, 50, ny), "exp(M + Y + 0 * global_tas)"),
                            ("log", 10.0 ** rng.uniform(-250, 250, n), 10.0 ** rng.uniform(-50, 50, ny),
                             "log(M * Y + 0 * global_tas)")):
        core.derive_expr("z", text, {"M": m, "Y": (y0, yv)})
        got = core.fetchvars("z", (y0, RUN_TO))
        with np.errstate(all="ignore"):
            x = (m[None, :] + yv[:, None] if fn == "exp" else m[None, :] * yv[:, None]) + 0.0 * tas["global_tas"]
            ref = (np.exp if fn == "exp" else np.log)(x.astype(np.longdouble))
        ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)
        err = float(np.max(np.abs(got.astype(np.longdouble) - ref) / ulp))
        print("series_expr %s: largest error %.3f ulp over %d arguments (%s)" % (fn, err, got.size, core.backend))
        worst[fn] = err
        assert np.isfinite(got).all() and err <= bound, (fn, err, bound)
    bind, vals = special_operands(core)
    with np.errstate(all="ignore"):
        for fn, f in (("exp", np.exp), ("log", np.log)):
            for a in ("mm", "yy"):
                core.derive_expr("z", "%s(%s)" % (fn, a), bind)
                got, x = core.fetchvars("z", (y0, RUN_TO)), vals[a]
                exact = ~np.isfinite(x) | (x <= 0.0) if fn == "log" else ~np.isfinite(x) | (x == 0.0)
                exact |= np.abs(x) == 1e308 if fn == "exp" else x == 1.0       # overflow, underflow; log(1) = 0
                same(got[exact], f(x[exact]), (fn, a, "special arguments"))
                ref = f(x[~exact].astype(np.longdouble))
                ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)
                assert np.max(np.abs(got[~exact].astype(np.longdouble) - ref) / ulp) <= bound, (fn, a)
    core.drop_series("mm").drop_series("yy").drop_series("z")
    return worst["exp"], worst["log"]


# ---- 2. every op on model data, the example's expressions ---------------------------------------------

COMPOUND = "(global_tas >= -0.05) & (pH < 8.2112)"      # the compound event of the example, at this run's scale
OVERSHOOT = "maximum(global_tas + 0.1, 0)"                # its overshoot
MODEL_TEXTS = (
    "-global_tas", "abs(global_tas - 0.02)", "sqrt(CO2_concentration)", "sqrt(global_tas)",
    "CO2_concentration + held", "pH - ocean_tas", "held * ocean_tas", "CO2_concentration / pH",
    "global_tas / (held - held)", "global_tas + slr",
    "minimum(global_tas, ocean_tas)", "maximum(global_tas - 0.01, 0)", "global_tas < ocean_tas", "held <= global_tas",
    "pH > 8.2112", "global_tas >= -0.05", "held == global_tas", "CO2_concentration != 277.15",
    "where(global_tas > -0.05, pH, ocean_tas)", "ifnan(sqrt(global_tas), 0)", "global_tas * year",
    COMPOUND, "(global_tas >= -0.05) | ~(pH < 8.2112)", OVERSHOOT,
    "global_tas / S_", "global_tas ** 2 - offs * ocean_tas ** 3 + CO2_concentration ** 4",
    "(CO2_concentration - 277.15) / CO2_concentration * global_tas",
)


def check_model_data(core):
    y0, n = core.strtdate, core.n_members
    core.hold("held", "CO2_concentration")
    S, _ = params(n)
    bind = {"S_": expr.param("S"), "offs": (y0 + 3, 0.5 + 0.25 * np.arange(30))}
    vals = fetch(core, OUTPUTS + ("held",))
    for text in MODEL_TEXTS:
        z = run(core, text, bind, vals, params_={"S": S})
        assert z.shape == (RUN_TO - y0 + 1, n)
    ind = run(core, COMPOUND, bind, vals, name="both")
    assert set(np.unique(ind)) == {0.0, 1.0} and 0.05 < ind.mean() < 0.95
    over = run(core, OVERSHOOT, bind, vals, name="over")
    core.derive("degyears", "cumsum", "over", years=y0)
    same(core.fetchvars("degyears", (y0, RUN_TO)), np.cumsum(over, axis=0), "degree-years")
    assert (over > 0).any() and (over == 0).any()
    # the core keeps two blocks of derived diagnostics: a third in one expression, and lags of them
    run(core, "pH + ocean_tas + RF_N2O - lag(pH, 2) * lag(RF_N2O, 1)", None, vals)
    assert "z" in core.series()


def check_probabilities_of_an_indicator(core):
    y0 = core.strtdate
    ind = run(core, "where(global_tas >= -0.1, pH < 8.2112, nan_)", {"nan_": float("nan")}, name="ind")
    assert np.isnan(ind).any() and (ind == 1.0).any() and (ind == 0.0).any()
    p, cnt, sums = core.probabilities("ind", [0.5], counts=True, sums=True)
    assert np.array_equal(cnt, (~np.isnan(ind)).sum(axis=1))
    assert np.array_equal(sums[:, 1], (ind == 1.0).sum(axis=1)) and np.array_equal(sums[:, 0], (ind == 0.0).sum(axis=1))
    with np.errstate(invalid="ignore"):
        same(p[:, 1], (ind == 1.0).sum(axis=1) / (~np.isnan(ind)).sum(axis=1).astype(float), "P(event)")


# ---- 3. program edges, lags, validity ------------------------------------------------------------------

def check_program_edges(core):
    vals = fetch(core, OUTPUTS)
    longest = "abs(global_tas" + " + 1" * 31 + ")"
    assert len(expr.compile(longest).ins) == expr.MAX_INS
    run(core, longest, None, vals)
    deepest = "(".join(["global_tas + "] * 7) + "ocean_tas" + ")" * 6
    assert expr.compile(deepest).depth == expr.MAX_STACK
    run(core, deepest, None, vals)
    with pytest.raises(E, match="HX_EX_MAX_INS"):
        expr.compile("-" + longest)
    with pytest.raises(E, match="HX_EX_MAX_STACK"):
        expr.compile("pH + (" + deepest + ")")
    eight = " + ".join("%s * lag(%s, %d)" % (v, v, k + 1) for k, v in enumerate(OUTPUTS[:4]))
    assert len(expr.compile(eight).vars) == expr.MAX_VARS
    run(core, eight, None, vals)
    with pytest.raises(E, match="HX_EX_MAX_VARS"):
        expr.compile(eight + " + lag(pH, 7)")
    four = expr.compile("global_tas ** 4 - global_tas")
    assert four.vars == [("global_tas", 0)] and sum(i[0] == "VAR" for i in four.ins) == 5
    run(core, "global_tas ** 4 - global_tas", None, vals)
    run(core, "lag(global_tas, 3) * 2", None, vals)
    # eight member vectors and eight year vectors at once (the largest kernel flavour)
    n, y0 = core.n_members, core.strtdate
    bind = {"m%d" % k: np.cos(np.arange(n) * (k + 1.0)) for k in range(8)}
    bind.update({"v%d" % k: (y0 + k, np.sin(np.arange(40) + k)) for k in range(8)})
    run(core, " + ".join("m%d * v%d" % (k, k) for k in range(8)) + " + global_tas", bind, vals)


def check_lags(core):
    y0 = core.strtdate
    ny = RUN_TO - y0 + 1
    assert ny == 46
    vals = fetch(core, OUTPUTS)
    for k in (1, 45, 46):
        z = run(core, "lag(CO2_concentration, %d)" % k, None, vals)
        assert np.isnan(z[:k]).all() and np.isfinite(z[k:]).all()
        if k < ny:
            same(z[k:], vals["CO2_concentration"][:ny - k], "the rows moved")
    d = run(core, "global_tas - lag(global_tas, 10)", None, vals)
    core.derive("delta10", "delta", "global_tas", lag=10)
    same(d, core.fetchvars("delta10", (y0, RUN_TO)), "x - lag(x, 10) is DELTA")
    f = run(core, "ifnan(lag(global_tas, 5), global_tas)", None, vals)
    same(f[:5], vals["global_tas"][:5], "the head is filled")
    same(f[5:], vals["global_tas"][:ny - 5], "behind it the lagged rows")


def check_validity(lib, n):
    """One operand held at 1780, the other valid to 1790: valid to 1780, NaN behind."""
    core = make_core(n, lib, run_to=1780)
    core.hold("early", "global_tas")
    core.run(RUN_TO)
    y0 = core.strtdate
    vals = fetch(core, ["early", "CO2_concentration"], to=1780)
    z = run(core, "early * CO2_concentration - lag(CO2_concentration, 2)", None, vals, to=1780)
    assert core.series() == {"early": 1780, "z": 1780}
    with pytest.raises(E, match="1780"):
        core.fetchvars("z", (y0, 1781))
    block = whole_block(core, "z")
    assert block.shape == (core.enddate - y0 + 1, n)
    same(block[:1780 - y0 + 1], z, "the valid rows")
    assert np.isnan(block[1780 - y0 + 1:]).all()
    # a batch that straddles the end of the run, and every batch behind it
    run(core, "CO2_concentration + global_tas", name="late")
    block = whole_block(core, "late")
    assert np.isfinite(block[:RUN_TO - y0 + 1]).all() and np.isnan(block[RUN_TO - y0 + 1:]).all()
    core.shutdown()


# ---- 4. the rules of the store ---------------------------------------------------------------------------

def check_store_rules(core):
    y0, n = core.strtdate, core.n_members
    tas = core.fetchvars("global_tas", (y0, RUN_TO))
    core.hold("x", "global_tas")
    core.derive_expr("x", "x * 2 + 1")
    same(core.fetchvars("x", (y0, RUN_TO)), tas * 2.0 + 1.0, "x = x * 2 + 1")
    w = np.sin(np.arange(n) * 1.0) + 2.0
    core.derive_expr("wx", "x / w - S_", {"w": w, "S_": expr.param("S")})
    S, _ = params(n)
    kept = (tas * 2.0 + 1.0) / w[None, :] - S[None, :]
    same(core.fetchvars("wx", (y0, RUN_TO)), kept, "a MEMBER operand in member order")
    # the result survives reset / run / setvar, and a new lane order
    lanes = core.lane_of_member()
    assert not np.array_equal(lanes, np.arange(n))      # sorted lanes: a true permutation
    core.setvar("S", S[::-1].copy(), "degC")
    core.set_member_sorting(False)
    core.reset(0)
    core.run(RUN_TO)
    assert not np.array_equal(core.lane_of_member(), lanes)
    now = core.fetchvars("global_tas", (y0, RUN_TO))
    assert not np.array_equal(now, tas)
    same(core.fetchvars("wx", (y0, RUN_TO)), kept, "the series means member m after the lanes moved")
    run(core, "wx + global_tas * w_", {"w_": w}, {"wx": kept, "global_tas": now})
    core.drop_series("wx").drop_series("z")
    # the 17th series
    for k in range(15):
        core.derive_expr("n%d" % k, "x + k", {"k": float(k)})
    assert len(core.series()) == 16
    with pytest.raises(E, match=FN + ".*16 series"):
        core.derive_expr("one_too_many", "x + 1")
    core.derive_expr("n3", "n3 * 2")                                # replacing one of the 16 is no 17th
    same(core.fetchvars("n3", (y0, RUN_TO)), (tas * 2.0 + 1.0 + 3.0) * 2.0, "replaced")
    assert len(core.series()) == 16
    for k in range(15):
        core.drop_series("n%d" % k)


def check_equals_derive(core):
    y0 = core.strtdate
    vec = 0.5 + 0.01 * np.arange(30)          # 1750..1779: NaN outside
    for op, sym in (("add", "+"), ("sub", "-"), ("mul", "*"), ("div", "/")):
        for b, text, bind in (("global_tas", "CO2_concentration %s global_tas", None),
                              (1.0 / 3.0, "CO2_concentration %s c", {"c": 1.0 / 3.0}),
                              (vec, "CO2_concentration %s v", {"v": (1750, vec)})):
            core.derive("d", op, "CO2_concentration", b, **({"first_year": 1750} if b is vec else {}))
            core.derive_expr("e", text % sym, bind)
            same(core.fetchvars("e", (y0, RUN_TO)), core.fetchvars("d", (y0, RUN_TO)), (op, text))
    assert np.isnan(core.fetchvars("e", (y0, RUN_TO))[[0, -1]]).all()   # (the vector's span)
    core.drop_series("d").drop_series("e")


def check_shards(one, many):
    n, y0 = one.n_members, one.strtdate
    w = np.cos(np.arange(n) * 0.37)
    bind = {"w": w, "S_": expr.param("S"), "v": (y0 + 2, np.arange(20.0))}
    for text in ("global_tas * w + S_", "where(pH < 8.2112, lag(ocean_tas, 3), w) / (v + CO2_concentration)"):
        for c in (one, many):
            c.derive_expr("z", text, bind)
        assert many.series() == {"z": RUN_TO}
        same(many.fetchvars("z", (y0, RUN_TO)), one.fetchvars("z", (y0, RUN_TO)), text)
    S, _ = params(n)
    same(one.fetchvars("z", (y0, RUN_TO)),
         expr.compile(text, bind).numpy(fetch(one, OUTPUTS), y0, params={"S": S}), "and both the definition")
    with pytest.raises(E, match=FN + ".*variable of the core"):
        many.derive_expr("slr", "global_tas + 1")
    assert many.series() == {"z": RUN_TO}


# ---- 5. refusals, through ctypes with a hand-built hx_expr ------------------------------------------------

def raw_eval(core, name, vars=(), members=(), yearvecs=(), ins=(), over=None):
    """hx_series_eval with the tables as given: vars [(name, lag)], members [ndarray or None],
    yearvecs [(first_year, ndarray)], ins [(op number, arg, value)]; over: fields to overwrite"""
    dp = ctypes.POINTER(ctypes.c_double)
    cv = (expr.HxExprVar * max(1, len(vars)))(*[expr.HxExprVar(v.encode() if v is not None else None, lag, 0)
                                                for v, lag in vars])
    arrays = [None if m is None else np.ascontiguousarray(m, dtype=np.float64) for m in members]
    cm = (dp * max(1, len(arrays)))(*[ctypes.cast(None, dp) if a is None else a.ctypes.data_as(dp) for a in arrays])
    vecs = [np.ascontiguousarray(v, dtype=np.float64) for _, v in yearvecs]
    cy = (expr.HxExprYearvec * max(1, len(vecs)))(*[expr.HxExprYearvec(fy, v.size, v.ctypes.data_as(dp))
                                                    for (fy, _), v in zip(yearvecs, vecs)])
    ci = (expr.HxExprIns * max(1, len(ins)))(*[expr.HxExprIns(*i) for i in ins])
    ex = expr.HxExpr(len(vars), len(arrays), len(vecs), len(ins), cv, cm, cy, ci)
    for k, v in (over or {}).items():
        if k == "reserved":
            ex.reserved[0] = v
        else:
            setattr(ex, k, v)
    core._ck(core._lib.hx_series_eval(core._h, name.encode() if name is not None else None, ctypes.byref(ex)))


def check_refusals(core, fresh):
    O = expr.OPS
    n, y0 = core.n_members, core.strtdate
    ns = core.enddate - y0 + 1
    core.hold("keep", "global_tas")
    kept = core.fetchvars("keep", (y0, RUN_TO))
    T = [("global_tas", 0)]
    V, C, ADD = (O["VAR"], 0, 0.0), (O["CONST"], 0, 1.0), (O["ADD"], 0, 0.0)
    ones = np.ones(n)
    nine = [("global_tas", k) for k in range(9)]
    bad = [
        ("null argument", lambda: core._ck(core._lib.hx_series_eval(core._h, b"z", None))),
        ("null argument", lambda: raw_eval(core, None, T, ins=[V])),
        ("null argument", lambda: raw_eval(core, "z", T, ins=[V], over={"ins": None})),
        ("null argument", lambda: raw_eval(core, "z", T, ins=[V], over={"vars": None})),
        ("null argument", lambda: raw_eval(core, "z", [(None, 0)], ins=[V])),
        ("nins must lie in 1..64", lambda: raw_eval(core, "z", T, ins=[])),
        ("nins must lie in 1..64", lambda: raw_eval(core, "z", T, ins=[V] + [C, ADD] * 32)),          # 65
        ("unknown op 24", lambda: raw_eval(core, "z", T, ins=[V, (24, 0, 0.0)])),
        ("unknown op -1", lambda: raw_eval(core, "z", T, ins=[V, (-1, 0, 0.0)])),
        ("arg 1 is outside the table vars", lambda: raw_eval(core, "z", T, ins=[(O["VAR"], 1, 0.0)])),
        ("arg -1 is outside the table vars", lambda: raw_eval(core, "z", T, ins=[(O["VAR"], -1, 0.0)])),
        ("arg 0 is outside the table members", lambda: raw_eval(core, "z", T, ins=[V, (O["MEMBER"], 0, 0.0), ADD])),
        ("arg 2 is outside the table yearvecs", lambda: raw_eval(core, "z", T, yearvecs=[(y0, ones), (y0, ones)],
                                                                 ins=[V, (O["YEARVEC"], 2, 0.0), ADD])),
        ("stack underflow", lambda: raw_eval(core, "z", T, ins=[V, ADD])),
        ("stack underflow", lambda: raw_eval(core, "z", T, ins=[(O["NEG"], 0, 0.0), V])),
        ("stack underflow", lambda: raw_eval(core, "z", T, ins=[V, V, (O["WHERE"], 0, 0.0)])),
        ("more than 8 values", lambda: raw_eval(core, "z", T, ins=[V] * 9 + [ADD] * 8)),              # depth 9
        ("ends with 2 values", lambda: raw_eval(core, "z", T, ins=[V, V])),
        ("more than 8 distinct", lambda: raw_eval(core, "z", nine, ins=[(O["VAR"], 0, 0.0)] + [
            x for k in range(1, 9) for x in ((O["VAR"], k, 0.0), ADD)])),
        ("more than 8 member vectors", lambda: raw_eval(core, "z", T, members=[ones] * 9, ins=[V])),
        ("more than 8 year vectors", lambda: raw_eval(core, "z", T, yearvecs=[(y0, ones)] * 9, ins=[V])),
        ("no VAR", lambda: raw_eval(core, "z", T, ins=[C, (O["YEAR"], 0, 0.0), ADD])),
        ("lag of global_tas must lie in 0..%d" % (ns - 1), lambda: raw_eval(core, "z", [("global_tas", -1)], ins=[V])),
        ("lag of global_tas must lie in 0..%d" % (ns - 1), lambda: raw_eval(core, "z", [("global_tas", ns)], ins=[V])),
        ("year vector 0 is empty", lambda: raw_eval(core, "z", T, yearvecs=[(y0, np.empty(0))], ins=[V])),
        ("member vector 1 is a null pointer", lambda: raw_eval(core, "z", T, members=[ones, None], ins=[V])),
        ("reserved", lambda: raw_eval(core, "z", T, ins=[V], over={"reserved": 1})),
        ("unknown variable", lambda: core.derive_expr("z", "never_defined + 1")),
        ("not enabled", lambda: core.derive_expr("z", "RF_tot + 1")),
        ("same for every member", lambda: core.derive_expr("z", "global_tas + ffi_emissions")),
        ("variable of the core", lambda: core.derive_expr("global_tas", "keep + 1")),
        ("variable of the core", lambda: core.derive_expr("pH", "keep + 1")),
        ("variable of the core", lambda: core.derive_expr("ffi_emissions", "keep + 1")),
        ("bad series name", lambda: core.derive_expr("9lives", "keep + 1")),
        ("bad series name", lambda: core.derive_expr("x" * 64, "keep + 1")),
    ]
    for text, call in bad:
        with pytest.raises(E, match=FN + ".*" + text):
            call()
        assert core.series() == {"keep": RUN_TO}, text
    # an operand that exists but is not recorded: a diagnostic derived from outputs that were not enabled
    # (the resolver's own text, the one hx_series_define gives)
    with pytest.raises(E, match="variable HL_DIC needs HL_ocean_c: enable it"):
        core.derive_expr("z", "global_tas + HL_DIC")
    assert core.series() == {"keep": RUN_TO}
    # eight lags of one name are eight operands, a ninth table entry that repeats one is not a ninth
    raw_eval(core, "z", nine[:8] + [("global_tas", 3)], ins=[(O["VAR"], 8, 0.0)] + [
        x for k in range(8) for x in ((O["VAR"], k, 0.0), ADD)])
    core.drop_series("z")
    with pytest.raises(E, match=FN + ".*run the core first"):
        fresh.derive_expr("z", "global_tas + 1")
    with pytest.raises(E, match=FN + ".*run the core first"):
        fresh.derive_expr("z", "ocean_tas + pH")
    assert fresh.series() == {}
    with pytest.raises(E, match="n_members"):
        core.derive_expr("z", "keep * w", {"w": np.ones(n + 1)})
    same(core.fetchvars("keep", (y0, RUN_TO)), kept, "kept")
    assert core.series() == {"keep": RUN_TO}
