"""Expressions over per-member variables for Core.derive_expr (hx_series_eval in
include/hector_amd.h): text -> a postfix Program, with the standard `ast` module and nothing else.

    compile("(global_tas >= 2.0) & (pH < 8.0)")
    compile("maximum(T - 1.5, 0)", bind={"T": "global_tas"})
    compile("dT / S", bind={"S": param("S")})          # a parameter of the members, through getvar
    compile("log(var('CO2_concentration') / c0)", bind={"c0": 277.15})
    compile("ifnan(lag(x, 5), x)", bind={"x": "global_tas"})

Identifiers are core variables (recorded outputs, derived diagnostics, combinations, series);
var("boreal.veg_c") serves names that are not identifiers; the bare name `year` is the calendar year.
`bind` is consulted first: an n_members array is a MEMBER operand, param("S") one that derive_expr
fills from getvar("S"), (first_year, values) a YEARVEC (NaN outside its span), a number a CONST, a
string an alias for a variable name.
Operators: + - * / and unary -; single comparisons < <= > >= == != (1.0 / 0.0, NaN if either side is);
a ** k for a literal k in 2..4, as left-to-right products; on indicators & is MUL, | is MAX and ~x is
1 - x.  Functions: abs sqrt log exp minimum maximum where(c, a, b) ifnan(a, b) lag(x, k) -- lag takes a
variable and a literal k >= 0 years.  Literal constant sub-expressions are NOT folded: the program is
what the text says.  Anything else is a HectorAmdError that quotes the offending piece of text.

Program.numpy restates the instruction table of hx_series_eval on fetchvars-shaped arrays: the
documentation of the semantics, and the tests' checker (as ensemble.midpit is for the ranks)."""
import ast
import ctypes

import numpy as np

from ._lib import HectorAmdError

# HX_EX_* of include/hector_amd.h
OPS = {"VAR": 0, "MEMBER": 1, "YEARVEC": 2, "CONST": 3, "YEAR": 4, "NEG": 5, "ABS": 6, "SQRT": 7, "LOG": 8,
       "EXP": 9, "ADD": 10, "SUB": 11, "MUL": 12, "DIV": 13, "MIN": 14, "MAX": 15, "LT": 16, "LE": 17, "GT": 18,
       "GE": 19, "EQ": 20, "NE": 21, "WHERE": 22, "IFNAN": 23}
OP_NAMES = {v: k for k, v in OPS.items()}
MAX_INS, MAX_VARS, MAX_MEMBERS, MAX_YEARVECS, MAX_STACK = 64, 8, 8, 8, 8   # HX_EX_MAX_*
_POPS = {op: 0 for op in ("VAR", "MEMBER", "YEARVEC", "CONST", "YEAR")}
_POPS.update({op: 1 for op in ("NEG", "ABS", "SQRT", "LOG", "EXP")})
_POPS.update({op: 2 for op in ("ADD", "SUB", "MUL", "DIV", "MIN", "MAX", "LT", "LE", "GT", "GE", "EQ", "NE",
                               "IFNAN")})
_POPS["WHERE"] = 3


class HxExprVar(ctypes.Structure):   # hx_expr_var
    _fields_ = [("name", ctypes.c_char_p), ("lag", ctypes.c_int), ("reserved", ctypes.c_int)]


class HxExprYearvec(ctypes.Structure):   # hx_expr_yearvec
    _fields_ = [("first_year", ctypes.c_int), ("n", ctypes.c_int), ("values", ctypes.POINTER(ctypes.c_double))]


class HxExprIns(ctypes.Structure):   # hx_expr_ins
    _fields_ = [("op", ctypes.c_int), ("arg", ctypes.c_int), ("value", ctypes.c_double)]


class HxExpr(ctypes.Structure):   # hx_expr
    _fields_ = [("nvars", ctypes.c_int), ("nmem", ctypes.c_int), ("nvec", ctypes.c_int), ("nins", ctypes.c_int),
                ("vars", ctypes.POINTER(HxExprVar)), ("members", ctypes.POINTER(ctypes.POINTER(ctypes.c_double))),
                ("yearvecs", ctypes.POINTER(HxExprYearvec)), ("ins", ctypes.POINTER(HxExprIns)),
                ("reserved", ctypes.c_int * 2)]


class param:
    """A MEMBER operand that Core.derive_expr fills from getvar(name): bind={"S": param("S")}."""

    def __init__(self, name):
        if not isinstance(name, str) or not name:
            raise HectorAmdError("expr.param: a parameter name is a non-empty string")
        self.name = name

    def __repr__(self):
        return "param(%r)" % self.name


class Program:
    """A postfix program and its operand tables:
    ins       [(op name, arg, value)], arg an index into vars / members / yearvecs, value of a CONST
    vars      [(name, lag)], distinct
    members   [ndarray [n_members] or param], MEMBER order
    yearvecs  [(first_year, ndarray)]"""

    def __init__(self, ins, vars, members, yearvecs, text=None):
        self.ins, self.vars, self.members, self.yearvecs, self.text = list(ins), list(vars), list(members), \
            list(yearvecs), text
        self.depth = _check(self, text if text is not None else "the program")

    def __repr__(self):
        return "Program(%s)" % " ".join(
            n if _POPS[n] or n == "YEAR" else "%s(%s)" % (n, repr(v) if n == "CONST" else a) for n, a, v in self.ins)

    def numpy(self, values, y0, params=None, valid_to=None):
        """The instruction table of hx_series_eval, literally, on fetchvars-shaped arrays.
        values: {variable name: ndarray [years, members]}, row 0 the year y0 (startDate, for a result
        that compares with the library's); params: {name: ndarray [n_members]} for param operands;
        valid_to: rows behind that calendar year are NaN.  -> ndarray [years, members]."""
        first = np.asarray(values[self.vars[0][0]], dtype=np.float64)
        ny, shape = first.shape[0], first.shape
        years = np.arange(y0, y0 + ny)
        stack = []
        with np.errstate(all="ignore"):
            for name, arg, value in self.ins:
                if name == "VAR":
                    var, lag = self.vars[arg]
                    x = np.asarray(values[var], dtype=np.float64)
                    r = np.full(shape, np.nan)
                    r[lag:] = x[:ny - lag]      # year y - lag; NaN where that is before row 0
                elif name == "MEMBER":
                    m = self.members[arg]
                    m = np.asarray(params[m.name] if isinstance(m, param) else m, dtype=np.float64)
                    r = np.broadcast_to(m[None, :], shape)
                elif name == "YEARVEC":
                    fy, v = self.yearvecs[arg]
                    col = np.full(ny, np.nan)
                    k = years - fy
                    on = (k >= 0) & (k < len(v))
                    col[on] = np.asarray(v, dtype=np.float64)[k[on]]
                    r = np.broadcast_to(col[:, None], shape)
                elif name == "CONST":
                    r = np.full(shape, np.float64(value))
                elif name == "YEAR":
                    r = np.broadcast_to(years.astype(np.float64)[:, None], shape)
                elif _POPS[name] == 1:
                    a = stack.pop()
                    r = {"NEG": np.negative, "ABS": np.fabs, "SQRT": np.sqrt, "LOG": np.log, "EXP": np.exp}[name](a)
                elif name == "WHERE":
                    b, a, c = stack.pop(), stack.pop(), stack.pop()
                    r = np.where(c != c, np.nan, np.where(c != 0.0, a, b))
                else:
                    b, a = stack.pop(), stack.pop()
                    nan2 = (a != a) | (b != b)
                    if name == "ADD":
                        r = a + b
                    elif name == "SUB":
                        r = a - b
                    elif name == "MUL":
                        r = a * b
                    elif name == "DIV":
                        r = a / b
                    elif name == "MIN":
                        r = np.where((a < b) | (a != a), a, b)
                    elif name == "MAX":
                        r = np.where((a > b) | (a != a), a, b)
                    elif name == "IFNAN":
                        r = np.where(a != a, b, a)
                    else:
                        cmp = {"LT": np.less, "LE": np.less_equal, "GT": np.greater, "GE": np.greater_equal,
                               "EQ": np.equal, "NE": np.not_equal}[name](a, b)
                        r = np.where(nan2, np.nan, np.where(cmp, 1.0, 0.0))
                stack.append(np.asarray(r, dtype=np.float64))
        out = np.array(stack.pop(), dtype=np.float64)
        if valid_to is not None:
            out[years > valid_to] = np.nan
        return out

    def _c(self, n_members, getvar):
        """-> (HxExpr, what must stay alive during the call)"""
        dp = ctypes.POINTER(ctypes.c_double)
        cv = (HxExprVar * max(1, len(self.vars)))(*[HxExprVar(n.encode(), int(lag), 0) for n, lag in self.vars])
        arrays = []
        for m in self.members:
            v = np.ascontiguousarray(getvar(m.name) if isinstance(m, param) else m, dtype=np.float64)
            if v.shape != (n_members,):
                raise HectorAmdError("hx_series_eval: a member operand of %s must have n_members = %d values"
                                     % (self.text or "the program", n_members))
            arrays.append(v)
        cm = (dp * max(1, len(arrays)))(*[a.ctypes.data_as(dp) for a in arrays])
        vecs = [np.ascontiguousarray(v, dtype=np.float64).ravel() for _, v in self.yearvecs]
        cy = (HxExprYearvec * max(1, len(vecs)))(*[HxExprYearvec(int(fy), int(v.size), v.ctypes.data_as(dp))
                                                   for (fy, _), v in zip(self.yearvecs, vecs)])
        ci = (HxExprIns * len(self.ins))(*[HxExprIns(OPS[n], int(a), float(v)) for n, a, v in self.ins])
        ex = HxExpr(len(self.vars), len(arrays), len(vecs), len(self.ins), cv, cm, cy, ci)
        return ex, (cv, arrays, cm, vecs, cy, ci)


def _check(p, what):
    """The limits and the stack discipline of hx_series_eval -> the depth the program reaches."""
    if not 1 <= len(p.ins) <= MAX_INS:
        raise HectorAmdError("expr: %s takes %d instructions; a program holds 1..%d (HX_EX_MAX_INS)"
                             % (what, len(p.ins), MAX_INS))
    for table, limit, name in ((p.vars, MAX_VARS, "distinct (variable, lag) operands (HX_EX_MAX_VARS)"),
                               (p.members, MAX_MEMBERS, "member operands (HX_EX_MAX_MEMBERS)"),
                               (p.yearvecs, MAX_YEARVECS, "year vectors (HX_EX_MAX_YEARVECS)")):
        if len(table) > limit:
            raise HectorAmdError("expr: %s uses %d %s; at most %d" % (what, len(table), name, limit))
    depth = top = 0
    for n, _, _ in p.ins:
        if n not in OPS:
            raise HectorAmdError("expr: unknown op %r in %s" % (n, what))
        if depth < _POPS[n]:
            raise HectorAmdError("expr: stack underflow at %s in %s" % (n, what))
        depth += 1 - _POPS[n]
        top = max(top, depth)
    if top > MAX_STACK:
        raise HectorAmdError("expr: %s needs an evaluation stack of %d values; at most %d (HX_EX_MAX_STACK)"
                             % (what, top, MAX_STACK))
    if depth != 1:
        raise HectorAmdError("expr: %s ends with %d values, not one" % (what, depth))
    if not any(n == "VAR" for n, _, _ in p.ins):
        raise HectorAmdError("expr: %s names no per-member variable; a series needs one" % what)
    return top


_BIN = {ast.Add: "ADD", ast.Sub: "SUB", ast.Mult: "MUL", ast.Div: "DIV", ast.BitAnd: "MUL", ast.BitOr: "MAX"}
_CMP = {ast.Lt: "LT", ast.LtE: "LE", ast.Gt: "GT", ast.GtE: "GE", ast.Eq: "EQ", ast.NotEq: "NE"}
_FUNCS = {"abs": ("ABS", 1), "sqrt": ("SQRT", 1), "log": ("LOG", 1), "exp": ("EXP", 1), "minimum": ("MIN", 2),
          "maximum": ("MAX", 2), "where": ("WHERE", 3), "ifnan": ("IFNAN", 2)}


class _Compiler:
    def __init__(self, text, bind):
        self.text, self.bind = text, dict(bind or {})
        self.ins, self.vars, self.members, self.yearvecs = [], [], [], []
        self._member_of, self._vec_of = {}, {}

    def bad(self, node, why):
        piece = ast.get_source_segment(self.text, node) if hasattr(node, "col_offset") else None
        raise HectorAmdError("expr: %s: %r in %r" % (why, piece if piece is not None else self.text, self.text))

    def emit(self, op, arg=0, value=0.0):
        self.ins.append((op, arg, value))

    def emit_var(self, name, lag):
        if (name, lag) not in self.vars:
            self.vars.append((name, lag))
        self.emit("VAR", self.vars.index((name, lag)))

    def variable(self, node):
        """-> the variable name a node stands for, or None: an identifier (bound to a string, or not
        bound and not `year`) or var("name")."""
        if isinstance(node, ast.Name):
            b = self.bind.get(node.id)
            if isinstance(b, str):
                return b
            if node.id not in self.bind and node.id != "year":
                return node.id
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "var":
            if node.keywords or len(node.args) != 1 or not isinstance(node.args[0], ast.Constant) or \
                    not isinstance(node.args[0].value, str) or not node.args[0].value:
                self.bad(node, "var() takes one literal variable name")
            return node.args[0].value
        return None

    def name(self, node):
        key = node.id
        if key not in self.bind:
            return self.emit("YEAR")   # (`year`: every other unbound identifier is a variable)
        b = self.bind[key]
        if isinstance(b, bool):
            self.bad(node, "a bound bool is not a number")
        if isinstance(b, (int, float, np.integer, np.floating)):
            return self.emit("CONST", 0, float(b))
        if isinstance(b, tuple) and len(b) == 2 and np.ndim(b[0]) == 0 and np.ndim(b[1]) == 1:
            if key not in self._vec_of:
                v = np.asarray(b[1], dtype=np.float64)
                if v.size < 1:
                    self.bad(node, "a bound year vector is empty")
                self._vec_of[key] = len(self.yearvecs)
                self.yearvecs.append((int(b[0]), v))
            return self.emit("YEARVEC", self._vec_of[key])
        if isinstance(b, param) or (not isinstance(b, tuple) and np.ndim(b) == 1):
            if key not in self._member_of:
                self._member_of[key] = len(self.members)
                self.members.append(b if isinstance(b, param) else np.asarray(b, dtype=np.float64))
            return self.emit("MEMBER", self._member_of[key])
        self.bad(node, "bound to %s, which is not a member array, param(), (first_year, values), a number or "
                       "a variable name" % type(b).__name__)

    def visit(self, node):
        v = self.variable(node)
        if v is not None:
            return self.emit_var(v, 0)
        if isinstance(node, ast.Name):
            return self.name(node)
        if isinstance(node, ast.Constant):
            if isinstance(node.value, bool) or not isinstance(node.value, (int, float)):
                self.bad(node, "not a number")
            return self.emit("CONST", 0, float(node.value))
        if isinstance(node, ast.UnaryOp):
            if isinstance(node.op, ast.USub):
                self.visit(node.operand)
                return self.emit("NEG")
            if isinstance(node.op, ast.Invert):   # ~x on an indicator: 1 - x
                self.emit("CONST", 0, 1.0)
                self.visit(node.operand)
                return self.emit("SUB")
            self.bad(node, "unsupported unary operator")
        if isinstance(node, ast.BinOp):
            if isinstance(node.op, ast.Pow):
                k = node.right
                if not (isinstance(k, ast.Constant) and type(k.value) is int and 2 <= k.value <= 4):
                    self.bad(node, "** takes a literal exponent 2, 3 or 4")
                self.visit(node.left)
                for _ in range(k.value - 1):   # ((x * x) * x) * x
                    self.visit(node.left)
                    self.emit("MUL")
                return None
            if type(node.op) not in _BIN:
                self.bad(node, "unsupported operator")
            self.visit(node.left)
            self.visit(node.right)
            return self.emit(_BIN[type(node.op)])
        if isinstance(node, ast.Compare):
            if len(node.ops) != 1:
                self.bad(node, "a chained comparison (write (a < b) & (b < c))")
            if type(node.ops[0]) not in _CMP:
                self.bad(node, "unsupported comparison")
            self.visit(node.left)
            self.visit(node.comparators[0])
            return self.emit(_CMP[type(node.ops[0])])
        if isinstance(node, ast.Call):
            if not isinstance(node.func, ast.Name):
                self.bad(node, "only plain function names can be called")
            fn = node.func.id
            if node.keywords:
                self.bad(node, "keyword arguments are not supported")
            if any(isinstance(a, ast.Starred) for a in node.args):
                self.bad(node, "starred arguments are not supported")
            if fn == "lag":
                if len(node.args) != 2:
                    self.bad(node, "lag takes (variable, years)")
                v = self.variable(node.args[0])
                if v is None:
                    self.bad(node, "lag applies to a variable only")
                k = node.args[1]
                if not (isinstance(k, ast.Constant) and type(k.value) is int and k.value >= 0):
                    self.bad(node, "the lag must be a literal number of years >= 0")
                return self.emit_var(v, k.value)
            if fn == "param":
                if len(node.args) != 1 or not isinstance(node.args[0], ast.Constant) or \
                        not isinstance(node.args[0].value, str) or not node.args[0].value:
                    self.bad(node, "param() takes one literal parameter name")
                key = ("param", node.args[0].value)
                if key not in self._member_of:
                    self._member_of[key] = len(self.members)
                    self.members.append(param(node.args[0].value))
                return self.emit("MEMBER", self._member_of[key])
            if fn not in _FUNCS:
                self.bad(node, "unknown function %s (one of %s, lag, var, param)" % (fn, ", ".join(_FUNCS)))
            op, nargs = _FUNCS[fn]
            if len(node.args) != nargs:
                self.bad(node, "%s takes %d argument%s" % (fn, nargs, "" if nargs == 1 else "s"))
            for a in node.args:
                self.visit(a)
            return self.emit(op)
        self.bad(node, "unsupported syntax (%s)" % type(node).__name__)


def compile(text, bind=None):   # noqa: A001 (the name the issue of this module gives it)
    """text -> Program (the module's docstring has the grammar)."""
    if isinstance(text, Program):
        return text
    if not isinstance(text, str) or not text.strip():
        raise HectorAmdError("expr: an expression is a non-empty string")
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except SyntaxError as e:
        raise HectorAmdError("expr: not an expression: %r (%s)" % (text, e.msg)) from None
    c = _Compiler(text.strip(), bind)
    c.visit(tree.body)
    return Program(c.ins, c.vars, c.members, c.yearvecs, text=repr(text.strip()))
