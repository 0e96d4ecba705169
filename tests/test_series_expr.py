"""hx_series_eval on the host-emulation build (Core.derive_expr), and the parser of hector_amd.expr.

The kernel is lane-local, so the emulation runs its very source one lane at a time; the bodies are
those of tests/series_expr_cases.py, which tests/test_gpu_series_expr.py runs on the product library.
The parser part needs no library at all.
"""
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import expr

import series_expr_cases as sc

E = hector_amd.HectorAmdError
N = 70


@pytest.fixture(scope="module")
def core(emul_lib):
    """One core for the bodies that leave it as they found it (the model runs once)."""
    c = sc.make_core(N, emul_lib)
    assert c.backend == "host-emulation"
    yield c
    c.shutdown()


def test_special_value_matrix_bit_for_bit_emulation(core):
    sc.check_special_values(core)
    assert core.series() == {}


def test_log_exp_within_one_ulp_and_exact_specials_emulation(core):
    sc.check_log_exp(core)
    assert core.series() == {}


def test_every_op_on_model_data_emulation(emul_lib):
    c = sc.make_core(N, emul_lib)
    sc.check_model_data(c)
    c.shutdown()


def test_program_edges_emulation(core):
    sc.check_program_edges(core)
    core.drop_series("z")


def test_lags_emulation(core):
    sc.check_lags(core)
    core.drop_series("z").drop_series("delta10")


def test_validity_and_rows_behind_it_emulation(emul_lib):
    sc.check_validity(emul_lib, N)


def test_store_rules_emulation(emul_lib):
    c = sc.make_core(N, emul_lib)
    sc.check_store_rules(c)
    c.shutdown()


def test_equals_derive_for_the_four_operations_emulation(core):
    sc.check_equals_derive(core)


def test_two_shards_give_the_one_shard_block_emulation(emul_lib):
    n = 2 * N + 3
    one, many = sc.make_core(n, emul_lib), sc.make_core(n, emul_lib, devices=[0, 0])
    sc.check_shards(one, many)
    one.shutdown()
    many.shutdown()


def test_refusals_emulation(emul_lib):
    c, fresh = sc.make_core(N, emul_lib), sc.make_core(N, emul_lib, run_to=0)
    sc.check_refusals(c, fresh)
    c.shutdown()
    fresh.shutdown()


# ---- the parser: text -> program, no library ---------------------------------------------------------

def ops(text, bind=None):
    return [(n, a) if n in ("VAR", "MEMBER", "YEARVEC") else (n, v) if n == "CONST" else n
            for n, a, v in expr.compile(text, bind).ins]


def test_parser_operators_and_functions():
    assert ops("a + b * c - d / e") == [("VAR", 0), ("VAR", 1), ("VAR", 2), "MUL", "ADD", ("VAR", 3), ("VAR", 4),
                                        "DIV", "SUB"]
    assert ops("-a") == [("VAR", 0), "NEG"]
    for sym, op in (("<", "LT"), ("<=", "LE"), (">", "GT"), (">=", "GE"), ("==", "EQ"), ("!=", "NE")):
        assert ops("a %s b" % sym) == [("VAR", 0), ("VAR", 1), op]
    for fn, op in (("abs", "ABS"), ("sqrt", "SQRT"), ("log", "LOG"), ("exp", "EXP")):
        assert ops("%s(a)" % fn) == [("VAR", 0), op]
    for fn, op in (("minimum", "MIN"), ("maximum", "MAX"), ("ifnan", "IFNAN")):
        assert ops("%s(a, b)" % fn) == [("VAR", 0), ("VAR", 1), op]
    assert ops("where(c, a, b)") == [("VAR", 0), ("VAR", 1), ("VAR", 2), "WHERE"]
    assert ops("a * year") == [("VAR", 0), "YEAR", "MUL"]
    p = expr.compile("var('boreal.veg_c') + lag(var('boreal.veg_c'), 2) + lag(x, 0) + x")
    assert p.vars == [("boreal.veg_c", 0), ("boreal.veg_c", 2), ("x", 0)]
    assert [i[:2] for i in p.ins if i[0] == "VAR"] == [("VAR", 0), ("VAR", 1), ("VAR", 2), ("VAR", 2)]
    assert p.depth == 2 and "VAR(0)" in repr(p)


def test_parser_indicator_and_power_translations():
    assert ops("(a < b) & (c > d)") == [("VAR", 0), ("VAR", 1), "LT", ("VAR", 2), ("VAR", 3), "GT", "MUL"]
    assert ops("(a < b) | (c > d)") == [("VAR", 0), ("VAR", 1), "LT", ("VAR", 2), ("VAR", 3), "GT", "MAX"]
    assert ops("~(a < b)") == [("CONST", 1.0), ("VAR", 0), ("VAR", 1), "LT", "SUB"]
    assert ops("a ** 2") == [("VAR", 0), ("VAR", 0), "MUL"]
    assert ops("a ** 4") == [("VAR", 0), ("VAR", 0), "MUL", ("VAR", 0), "MUL", ("VAR", 0), "MUL"]
    assert ops("(a + 1) ** 3") == [("VAR", 0), ("CONST", 1.0), "ADD"] * 1 + [("VAR", 0), ("CONST", 1.0), "ADD", "MUL"] * 2


def test_parser_does_not_fold_constants():
    assert ops("a + 2 * 3") == [("VAR", 0), ("CONST", 2.0), ("CONST", 3.0), "MUL", "ADD"]
    assert ops("a * -2.5") == [("VAR", 0), ("CONST", 2.5), "NEG", "MUL"]
    assert ops("(1 + 1) * a") == [("CONST", 1.0), ("CONST", 1.0), "ADD", ("VAR", 0), "MUL"]


def test_parser_bind_kinds():
    m, v = np.arange(5.0), np.arange(3.0)
    bind = {"m": m, "y": (1900, v), "k": 2.5, "T": "global_tas", "S": expr.param("S"), "i": 3}
    p = expr.compile("T * m + y - k + lag(T, 4) / S + m * i + param('S') + param('q10_rh')", bind)
    assert p.vars == [("global_tas", 0), ("global_tas", 4)]
    assert len(p.members) == 4 and p.members[0] is not None and np.array_equal(p.members[0], m)
    assert [getattr(x, "name", None) for x in p.members[1:]] == ["S", "S", "q10_rh"]
    assert len(p.yearvecs) == 1 and p.yearvecs[0][0] == 1900 and np.array_equal(p.yearvecs[0][1], v)
    got = [(n, a) if n != "CONST" else (n, x) for n, a, x in p.ins if n in ("MEMBER", "YEARVEC", "CONST")]
    assert got == [("MEMBER", 0), ("YEARVEC", 0), ("CONST", 2.5), ("MEMBER", 1), ("MEMBER", 0), ("CONST", 3.0),
                   ("MEMBER", 2), ("MEMBER", 3)]
    # a bound `year` is what it is bound to; an unbound one the calendar year
    assert ops("a + year", {"year": 7}) == [("VAR", 0), ("CONST", 7.0), "ADD"]
    # the numpy restatement takes the same bindings
    vals = {"global_tas": np.arange(12.0).reshape(6, 2)}
    p = expr.compile("where(T > 4, T * m, -y) + S", {"T": "global_tas", "m": np.array([1.0, -1.0]),
                                                      "y": (1901, v), "S": expr.param("S")})
    z = p.numpy(vals, 1900, params={"S": np.array([10.0, 20.0])}, valid_to=1904)
    assert np.isnan(z[0]).all() and np.isnan(z[5]).all()        # no y in 1900; behind valid_to
    assert np.array_equal(z[1:3], [[10.0, 20.0], [9.0, 15.0]]) and np.array_equal(z[3:5], [[16.0, 13.0], [18.0, 11.0]])


@pytest.mark.parametrize("text, piece, why", [
    ("a < b < c", "a < b < c", "chained comparison"),
    ("a + tanh(b)", "tanh(b)", "unknown function tanh"),
    ("lag(a + b, 2)", "lag(a + b, 2)", "lag applies to a variable only"),
    ("lag(year, 2)", "lag(year, 2)", "lag applies to a variable only"),
    ("lag(a, k)", "lag(a, k)", "literal number of years"),
    ("lag(a, -1)", "lag(a, -1)", "literal number of years"),
    ("a ** 5", "a ** 5", "literal exponent 2, 3 or 4"),
    ("a ** b", "a ** b", "literal exponent"),
    ("a ** 2.0", "a ** 2.0", "literal exponent"),
    ("a + np.pi", "np.pi", "unsupported syntax"),
    ("a.real", "a.real", "unsupported syntax"),
    ("minimum(a, b=c)", "minimum(a, b=c)", "keyword arguments"),
    ("np.sqrt(a)", "np.sqrt(a)", "plain function names"),
    ("a if b else c", "a if b else c", "unsupported syntax"),
    ("a and b", "a and b", "unsupported syntax"),
    ("not a", "not a", "unsupported unary"),
    ("a % b", "a % b", "unsupported operator"),
    ("a // b", "a // b", "unsupported operator"),
    ("a in b", "a in b", "unsupported comparison"),
    ("a + 'x'", "'x'", "not a number"),
    ("a + True", "True", "not a number"),
    ("a[0]", "a[0]", "unsupported syntax"),
    ("sqrt(a, b)", "sqrt(a, b)", "sqrt takes 1 argument"),
    ("where(a, b)", "where(a, b)", "where takes 3 arguments"),
    ("var(a)", "var(a)", "one literal variable name"),
])
def test_parser_rejections_quote_the_text(text, piece, why):
    with pytest.raises(E, match=re.escape(why)) as e:
        expr.compile("1 + (" + text + ")" if "if" not in text and " and " not in text else text)
    assert repr(piece) in str(e.value), str(e.value)


def test_parser_other_rejections():
    with pytest.raises(E, match="not an expression"):
        expr.compile("a +")
    with pytest.raises(E, match="non-empty string"):
        expr.compile("  ")
    with pytest.raises(E, match="names no per-member variable"):
        expr.compile("1 + year")
    with pytest.raises(E, match="bound to dict"):
        expr.compile("a + b", {"b": {}})
    with pytest.raises(E, match="HX_EX_MAX_MEMBERS"):
        expr.compile("a + " + " + ".join("param('p%d')" % k for k in range(9)))
    with pytest.raises(E, match="HX_EX_MAX_YEARVECS"):
        expr.compile("a + " + " + ".join("v%d" % k for k in range(9)), {"v%d" % k: (1900, np.ones(2)) for k in range(9)})
    p = expr.compile("a + 1")
    assert expr.compile(p) is p


# ---- the header pin --------------------------------------------------------------------------------------

def test_header_states_the_abi_and_its_semantics():
    import os
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hector_amd.h")).read()
    assert "int hx_series_eval(hx_core *core, const char *name, const hx_expr *expr);" in h
    for name, number in expr.OPS.items():
        assert re.search(r"#define HX_EX_%s %d\n" % (name, number), h), name
    assert "#define HX_EX_NOPS %d\n" % len(expr.OPS) in h
    for name, value in (("INS", expr.MAX_INS), ("VARS", expr.MAX_VARS), ("MEMBERS", expr.MAX_MEMBERS),
                        ("YEARVECS", expr.MAX_YEARVECS), ("STACK", expr.MAX_STACK)):
        assert "#define HX_EX_MAX_%s %d\n" % (name, value) in h
    flat = " ".join(h.split()).replace(" * ", " ")
    for words in ("(a < b || a != a) ? a : b", "(a > b || a != a) ? a : b", "NaN if either operand is NaN, else 1.0 or 0.0",
                  "NaN if c is NaN; a if c != 0; otherwise b", "The branch not taken does not matter, NaN included",
                  "b if a is NaN, else a", "NaN if that year is before startDate (such a row is not loaded)",
                  "sign-bit operations", "at +-0 ties the second operand", "log(0) = -inf, log(<0) = NaN, exp(-inf) = 0",
                  "A (name, lag) pair that occurs twice is ONE operand", "permutes them to lane order",
                  "NaN outside the span", "(double) calendar year", "contraction off",
                  "valid to the smallest valid end over its VAR operands", "At least one VAR is required",
                  "every message names hx_series_eval; a refused call changes nothing"):
        assert words in flat, words
    for field in ("hx_expr_var", "hx_expr_yearvec", "hx_expr_ins", "} hx_expr;", "int reserved[2];"):
        assert field in h
    assert "hx_series_eval" in hector_amd._lib.ABI_SYMBOLS
