"""hx_member_pair_metrics and its siblings (Core.pair_metrics, hector_amd.PairMetric): the parts that
need no GPU and no run -- the header documents the four symbols and both libraries export them,
PairMetric validates its arguments, and a spy in the symbols' place shows what a call hands over.
"""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import hector_amd
from hector_amd import PairMetric
from hector_amd.core import PAIR_METRIC_OPS, _HxPairMetric
from conftest import ROOT, SCENARIO

E = hector_amd.HectorAmdError
SYMBOLS = ("hx_member_pair_metrics", "hx_pair_metric_quantiles", "hx_pair_metric_probabilities",
           "hx_pair_metric_moments")
LEAD = (r"\(hx_core \*core, const char \*cap_a, const char \*cap_b, const double \*b_vec,\s+int b_year0, "
        r"int b_year1, const hx_pair_metric \*specs, int nspecs,\s+")


def test_the_header_documents_the_symbols_and_the_libraries_export_them(emul_lib, hip_lib):
    from hector_amd import _lib
    text = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    assert re.search(r"typedef struct \{\s+int op, year0, year1;\s+int base_a0, base_a1;[^\n]*\n\s+int base_b0, base_b1;"
                     r"[^\n]*\n\s+int reserved;\s+double threshold;\s+\} hx_pair_metric;", text)
    assert re.search(r"\bint hx_member_pair_metrics" + LEAD + r"double \*out\);", text)
    assert re.search(r"\bint hx_pair_metric_quantiles" + LEAD + r"const double \*weights, const double \*probs, "
                     r"int nprobs, double \*out,\s+long long \*n_part\);", text)
    assert re.search(r"\bint hx_pair_metric_probabilities" + LEAD + r"const double \*weights, const double \*edges, "
                     r"int nedges, double \*prob,\s+unsigned long long \*sums, long long \*n_part\);", text)
    assert re.search(r"\bint hx_pair_metric_moments" + LEAD + r"const double \*weights, const double \*predictors, "
                     r"int npred, double \*shift,\s+double \*sums, unsigned long long \*wsum, long long \*n_part\);", text)
    for name, value in PAIR_METRIC_OPS.items():
        assert re.search(r"^#define HX_PMET_%s %d\b" % (name.upper(), value), text, re.M), name
    assert re.search(r"^#define HX_PMET_NOPS 8$", text, re.M) and re.search(r"^#define HX_PMET_MAX_SPECS 32$", text, re.M)
    doc = text[text.index("Two series of the same member"):text.index("int hx_pair_metric_moments(")]
    for phrase in ("base_a0 > base_a1: none", "EXACTLY ONE", "b_vec[y - b_year0]", "names\n *     the year",
                   "without fused multiply-add", "s = 0.0; for y = base_a0..base_a1: s = s + xa_y;  base_a = s / count",
                   "ma = sa / n;  mb = sb / n", "sab = sab + (db * da);  sbb = sbb + (db * db)", "saa = saa + (da * da)",
                   "every product rounded before its sum", "SLOPE = sab / sbb;  INTERCEPT = ma - (SLOPE * mb);  "
                   "R2 = (sab * sab) / (sbb * saa)", "0 / 0 = NaN", "no special case and no sqrt",
                   "first year with b_y >= threshold; NaN if there is none", "only on strict > / <",
                   "divided by\n *     their count as a double", "(a_year1 - a_year0) / (b_year1 - b_year0)",
                   "reads only the two end rows", "NaN rule", "no grouping", "eight rows of each operand",
                   "not prepared, spun up or dirtied", "every message names the function", "a refused call changes nothing",
                   "both or neither of cap_b / b_vec", "never reaches\n * the host", "does not take part",
                   "communicator of several processes is refused", "refused after the argument checks"):
        assert phrase in doc, phrase
    abi = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_abi.cpp")).read()
    post = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_post.h")).read()
    assert re.search(r"^#define HXP_BATCH 8\b", post, re.M)
    kernel = post[post.index("void hx_pair_metric_kernel("):post.index("hipError_t hx_launch_pair_metric(")]
    assert "#pragma clang fp contract(off)" in kernel and "__shared__" not in kernel and "atomic" not in kernel
    lib = _lib.load(emul_lib, allow_emulation=True)
    assert os.path.exists(hip_lib)
    product = ctypes.CDLL(hip_lib)
    dp = ctypes.POINTER(ctypes.c_double)
    lead = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, dp, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    assert lib.hx_member_pair_metrics.argtypes == lead + [dp]
    for fn in SYMBOLS:
        assert fn in _lib.ABI_SYMBOLS
        assert "int %s(" % fn in abi and "%s: null argument" % fn in abi
        assert getattr(lib, fn).argtypes[:8] == lead
        getattr(product, fn)
    assert ctypes.sizeof(_HxPairMetric) == 40 and _HxPairMetric.threshold.offset == 32


def test_pair_metric_validates_its_arguments():
    assert hector_amd.PairMetric is PairMetric
    assert tuple(PAIR_METRIC_OPS) == ("slope", "intercept", "r2", "at_first_ge", "at_max", "at_min", "mean_where_ge",
                                      "end_ratio")
    for op in ("median", "first_ge", "", None):
        with pytest.raises(E, match="PairMetric: unknown op"):
            PairMetric(op, 1900)
    with pytest.raises(E, match="PairMetric: years must be a year or"):
        PairMetric("slope", [])
    with pytest.raises(E, match="PairMetric: baseline must be"):
        PairMetric("slope", 1900, baseline=(1900, 1850))
    with pytest.raises(E, match="PairMetric: baseline_b must be"):
        PairMetric("slope", 1900, baseline_b=(1850,))
    m = PairMetric("at_first_ge", (2100, 1850), baseline=(1850, 1900), baseline_b=[1860, 1870], threshold=1.5)
    assert m.years == (1850, 2100) and m.baseline == (1850, 1900) and m.baseline_b == (1860, 1870) and m.threshold == 1.5
    c = m._c()
    assert (c.op, c.year0, c.year1, c.base_a0, c.base_a1, c.base_b0, c.base_b1, c.reserved, c.threshold) == \
        (3, 1850, 2100, 1850, 1900, 1860, 1870, 0, 1.5)
    c = PairMetric("end_ratio", 2000)._c()
    assert (c.op, c.year0, c.year1) == (7, 2000, 2000) and c.base_a0 > c.base_a1 and c.base_b0 > c.base_b1
    assert c.threshold != c.threshold
    assert repr(m) == "PairMetric('at_first_ge', (1850, 2100), baseline=(1850, 1900), baseline_b=(1860, 1870), threshold=1.5)"


class _Spy:
    """Stands in for a symbol of the library: records the leading arguments it is handed."""

    def __init__(self, fill):
        self.calls, self.fill = [], fill

    def __call__(self, h, cap_a, cap_b, b_vec, b_year0, b_year1, specs, nspecs, *rest):
        vec = None if not b_vec else np.ctypeslib.as_array(b_vec, (b_year1 - b_year0 + 1,)).copy()
        recs = ctypes.cast(specs, ctypes.POINTER(_HxPairMetric))
        ops = [(recs[i].op, recs[i].year0, recs[i].year1) for i in range(nspecs)]
        self.calls.append((cap_a, cap_b, vec, b_year0, b_year1, ops, nspecs, len(rest)))
        self.fill(nspecs, rest)
        return 0


def test_the_binding_hands_over_what_it_was_given(emul_lib, monkeypatch):
    c = hector_amd.Core(SCENARIO, 4, lib_path=emul_lib, allow_emulation=True)

    def fill_members(nspecs, rest):
        np.ctypeslib.as_array(rest[0], (nspecs, 4))[:] = np.arange(1.0, nspecs + 1.0)[:, None]

    spies = {"hx_member_pair_metrics": _Spy(fill_members)}
    for fn in SYMBOLS[1:]:
        spies[fn] = _Spy(lambda nspecs, rest: None)

    class Lib:       # the loaded library with the four symbols replaced
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return spies[name] if name in spies else getattr(self._lib, name)

    monkeypatch.setattr(c, "_lib", Lib(c._lib))
    specs = [PairMetric("slope", (1850, 1900)), PairMetric("at_max", 1870), PairMetric("end_ratio", (1800, 1801))]
    ops = [(0, 1850, 1900), (4, 1870, 1870), (7, 1800, 1801)]
    # what the binding refuses itself: nothing reaches the library
    for b, s, text in (("global_tas", ["slope"], "pair_metrics: specs must be hector_amd.PairMetric objects"),
                       ("global_tas", [hector_amd.Metric("slope", 1900)], "specs must be hector_amd.PairMetric objects"),
                       (7, specs, r"pair_metrics: b is a variable name or a \(years, values\) pair"),
                       (([1850, 1851], [1.0]), specs, "pair_metrics: the vector b needs one value per year"),
                       (([], []), specs, "pair_metrics: the vector b needs one value per year"),
                       (([1850, 1852], [1.0, 2.0]), specs, "the years of the vector b must be consecutive and ascending"),
                       (([1851, 1850], [1.0, 2.0]), specs, "the years of the vector b must be consecutive and ascending")):
        with pytest.raises(E, match=text):
            c.pair_metrics("CO2_concentration", b, s)
    with pytest.raises(E, match="pair_metric_quantiles: weights must have n_members"):
        c.pair_metric_quantiles("CO2_concentration", "global_tas", specs, [0.5], weights=np.ones(3))
    with pytest.raises(E, match="pair_metric_probabilities: edges must be one-dimensional"):
        c.pair_metric_probabilities("CO2_concentration", "global_tas", specs, [[0.0, 1.0]])
    with pytest.raises(E, match="pair_metric_moments: at most 8 entries in against"):
        c.pair_metric_moments("CO2_concentration", "global_tas", specs, against=[np.ones(4)] * 9)
    assert all(s.calls == [] for s in spies.values())
    # a variable b
    out = c.pair_metrics("CO2_concentration", "global_tas", specs)
    (cap_a, cap_b, vec, y0, y1, got_ops, ns, nrest), = spies["hx_member_pair_metrics"].calls
    assert (cap_a, cap_b, vec, ns, nrest) == (b"CO2_concentration", b"global_tas", None, 3, 1) and got_ops == ops
    assert out.shape == (3, 4) and np.array_equal(out, np.arange(1.0, 4.0)[:, None] * np.ones(4))
    # a vector b (a strided view, integer values), one bare specification
    spies["hx_member_pair_metrics"].calls.clear()
    years, values = np.arange(1850, 1861), np.arange(22)[::2]
    out = c.pair_metrics("global_tas", (years, values), specs[1])
    (cap_a, cap_b, vec, y0, y1, got_ops, ns, nrest), = spies["hx_member_pair_metrics"].calls
    assert (cap_a, cap_b, y0, y1, ns) == (b"global_tas", None, 1850, 1860, 1) and got_ops == ops[1:2]
    assert vec.dtype == np.float64 and np.array_equal(vec, np.arange(0.0, 22.0, 2.0)) and out.shape == (1, 4)
    # the ensemble-wide verbs hand over the same leading arguments, then their counterparts' own
    c.pair_metric_quantiles("CO2_concentration", (years, values), specs, [0.1, 0.9], weights=np.ones(4))
    c.pair_metric_probabilities("CO2_concentration", "global_tas", specs, [0.0, 1.0])
    c.pair_metric_moments("CO2_concentration", "global_tas", specs, against=[np.ones(4)])
    for fn, nrest, b in (("hx_pair_metric_quantiles", 5, None), ("hx_pair_metric_probabilities", 6, b"global_tas"),
                         ("hx_pair_metric_moments", 7, b"global_tas")):
        (cap_a, cap_b, vec, y0, y1, got_ops, ns, n), = spies[fn].calls
        assert (cap_a, cap_b, ns, n) == (b"CO2_concentration", b, 3, nrest) and got_ops == ops, fn
        assert (vec is None) == (b is not None)
    # a triple in against= goes through pair_metrics
    spies["hx_member_pair_metrics"].calls.clear()
    c.pair_metric_moments("CO2_concentration", "global_tas", specs, against=[("global_tas", (years, values), specs[0])])
    (cap_a, cap_b, vec, y0, y1, got_ops, ns, nrest), = spies["hx_member_pair_metrics"].calls
    assert (cap_a, cap_b, y0, y1, ns) == (b"global_tas", None, 1850, 1860, 1) and got_ops == ops[:1]
    c.shutdown()


def test_the_carbon_budget_example_imports():
    spec = importlib.util.spec_from_file_location("example_carbon_budget", os.path.join(ROOT, "examples", "carbon_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.LEVELS == (1.5, 2.0)
