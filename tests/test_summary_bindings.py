"""The summary verbs of Core as calls of the C ABI: which hx_* function every (verb, kind of rows,
grouped) form calls, with which leading arguments and which output buffers, and the argument errors
that every form shares.  No GPU: a recorder stands in for the library.

The host-emulation build refuses the summary functions by name, so their results cannot be compared
here (the GPU tests do that); the calls can.  `Recorder` wraps the emulation's library of a small core
that has run: the functions of ANSWERED are logged and forwarded (the dates, parameters and
lane-local per-member metrics that the verbs read on their way), every other function is logged and
answered with 0.  SIG restates the argument lists of include/hector_amd.h by hand ('>' marks an
output: its shape and dtype are logged, not its bytes, which are whatever np.empty left there); the
expectations below are written against those names, not taken from hector_amd/core.py.
"""
import ctypes

import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, PairMetric, Moments, GroupedMoments, Sobol
from conftest import SCENARIO

E = hector_amd.HectorAmdError
N, RUN_TO, START = 7, 1760, 1745

SIG = {   # include/hector_amd.h, after the handle
    "hx_ensemble_quantiles": "capability year0 year1 weights probs nprobs >out >n_part",
    "hx_metric_quantiles": "capability specs nspecs weights probs nprobs >out >n_part",
    "hx_pair_metric_quantiles": "cap_a cap_b b_vec b_year0 b_year1 specs nspecs weights probs nprobs >out >n_part",
    "hx_group_quantiles": "capability year0 year1 specs nspecs labels ngroups weights probs nprobs >out >n_part",
    "hx_ensemble_probabilities": "capability year0 year1 weights edges nedges >prob >sums >n_part",
    "hx_metric_probabilities": "capability specs nspecs weights edges nedges >prob >sums >n_part",
    "hx_pair_metric_probabilities":
        "cap_a cap_b b_vec b_year0 b_year1 specs nspecs weights edges nedges >prob >sums >n_part",
    "hx_group_probabilities":
        "capability year0 year1 specs nspecs labels ngroups weights edges nedges >prob >sums >n_part",
    "hx_ensemble_moments": "capability year0 year1 weights predictors npred >shift >sums >wsum >n_part",
    "hx_metric_moments": "capability specs nspecs weights predictors npred >shift >sums >wsum >n_part",
    "hx_pair_metric_moments":
        "cap_a cap_b b_vec b_year0 b_year1 specs nspecs weights predictors npred >shift >sums >wsum >n_part",
    "hx_group_moments": "capability year0 year1 specs nspecs labels ngroups weights predictors npred "
                        ">shift >pshift >sums >wsum >n_part",
    "hx_ensemble_sobol": "capability year0 year1 k n_base use >shift >sums >n_part",
    "hx_metric_sobol": "capability specs nspecs k n_base use >shift >sums >n_part",
    "hx_member_metrics": "capability specs nspecs >out",
    "hx_member_pair_metrics": "cap_a cap_b b_vec b_year0 b_year1 specs nspecs >out",
    "hx_metric_ranks": "capability specs nspecs weights kind >out",
    "hx_series_rank": "name capability year0 year1 weights kind",
}
ANSWERED = ("hx_dates", "hx_getvar", "hx_member_metrics", "hx_member_pair_metrics", "hx_series_list",
            "hx_last_error")


def decode(a, output=False):
    """One argument of a call as plain data: a scalar as given; a pointer into a numpy array, a
    ctypes array or a byref of one as (dtype or type name, shape, bytes) -- bytes None for an output."""
    arr = getattr(a, "_arr", None)              # ndarray.ctypes.data_as keeps its array there
    if isinstance(arr, np.ndarray):
        assert arr.flags["C_CONTIGUOUS"]
        return (str(arr.dtype), arr.shape, None if output else arr.tobytes())
    obj = getattr(a, "_obj", a)                 # ctypes.byref keeps its object there
    if isinstance(obj, (ctypes.Array, ctypes.Structure, ctypes._SimpleCData)) and not isinstance(obj, ctypes.c_void_p):
        shape = (len(obj),) if isinstance(obj, ctypes.Array) else ()
        return (type(obj).__name__, shape, None if output else bytes(obj))
    if isinstance(obj, ctypes._Pointer):        # (a pointer the library sets: hx_series_list)
        return type(obj).__name__
    return a.value if isinstance(a, ctypes.c_void_p) else a


class Recorder:
    def __init__(self, lib):
        self.lib, self.log = lib, []

    def __getattr__(self, fn):
        if not fn.startswith("hx_"):
            raise AttributeError(fn)
        names = SIG.get(fn, "").split()

        def call(handle, *args):
            outs = [n.startswith(">") for n in names] if names else [False] * len(args)
            assert len(outs) == len(args), (fn, len(args))
            if fn in ANSWERED:   # (before logging: the outputs of a forwarded call do not enter the log either)
                rc = getattr(self.lib, fn)(handle, *args)
            else:
                rc = 0
            self.log.append((fn, [decode(a, o) for a, o in zip(args, outs)]))
            return rc
        if fn == "hx_last_error":
            return self.lib.hx_last_error
        return call

    def named(self, i=-1):
        """Call i of the log -> (function, {argument name: decoded value})."""
        fn, args = self.log[i]
        return fn, dict(zip([n.lstrip(">") for n in SIG[fn].split()], args))


@pytest.fixture(scope="module")
def rec(emul_lib):
    c = hector_amd.Core(SCENARIO, N, lib_path=emul_lib, allow_emulation=True)
    c.setvar("S", np.linspace(2.0, 4.5, N), "degC")
    c.run(RUN_TO)
    c._lib = r = Recorder(c._lib)
    yield c, r
    c._lib = r.lib
    c.shutdown()


VAR = "global_tas"
SPECS = [Metric("mean", (1750, 1760)), Metric("max", (1746, 1755), baseline=(1745, 1750))]
PSPECS = [PairMetric("slope", (1750, 1760))]
BVEC = (np.arange(1750, 1761), np.linspace(0.0, 1.0, 11))
LAB = np.array([0, 1, 2, -1, 0, 1, 2])
W = np.linspace(0.5, 2.0, N)
PROBS, EDGES = [0.1, 0.5, 0.9], [0.0, 0.5]


def spec_bytes(specs):
    return b"".join(bytes(s._c()) for s in specs)


def f64(a):
    return ("float64", np.shape(a), np.asarray(a, dtype=np.float64).tobytes())


# kind of rows -> (the arguments in front of the verb's own in the public call, its dates= if any, the
# leading arguments of the ungrouped function, those of the grouped function, the number of rows)
ROWS = {
    "window": (lambda name: (VAR,), dict(dates=(1750, 1755)),
               dict(capability=VAR.encode(), year0=1750, year1=1755),
               dict(capability=VAR.encode(), year0=1750, year1=1755, specs=None, nspecs=0), 6),
    "window, all years": (lambda name: (VAR,), {},
                          dict(capability=VAR.encode(), year0=START, year1=RUN_TO),
                          dict(capability=VAR.encode(), year0=START, year1=RUN_TO, specs=None, nspecs=0),
                          RUN_TO - START + 1),
    "metric": (lambda name: (VAR, SPECS), {},
               dict(capability=VAR.encode(), specs=("_HxMetric_Array_2", (2,), spec_bytes(SPECS)), nspecs=2),
               dict(capability=VAR.encode(), year0=0, year1=0,
                    specs=("_HxMetric_Array_2", (2,), spec_bytes(SPECS)), nspecs=2), 2),
    "pair, b a name": (lambda name: (VAR, "CO2_concentration", PSPECS), {},
                       dict(cap_a=VAR.encode(), cap_b=b"CO2_concentration", b_vec=None, b_year0=0, b_year1=0,
                            specs=("_HxPairMetric_Array_1", (1,), spec_bytes(PSPECS)), nspecs=1), None, 1),
    "pair, b a vector": (lambda name: (VAR, BVEC, PSPECS), {},
                         dict(cap_a=VAR.encode(), cap_b=None, b_vec=f64(BVEC[1]), b_year0=1750, b_year1=1760,
                              specs=("_HxPairMetric_Array_1", (1,), spec_bytes(PSPECS)), nspecs=1), None, 1),
}
PREFIX = {"window": "", "window, all years": "", "metric": "metric_", "pair, b a name": "pair_metric_",
          "pair, b a vector": "pair_metric_"}
STEM = {"window": "hx_ensemble_", "window, all years": "hx_ensemble_", "metric": "hx_metric_",
        "pair, b a name": "hx_pair_metric_", "pair, b a vector": "hx_pair_metric_"}
GROUPS = {None: None, "labels": LAB, "(labels, G)": (LAB, 4)}


def forms():
    for kind in ROWS:
        for verb in ("quantiles", "probabilities", "moments"):
            for grouped in GROUPS:
                if grouped is None or not kind.startswith("pair"):
                    yield verb, kind, grouped
        if not kind.startswith("pair"):
            yield "sobol", kind, None


@pytest.mark.parametrize("verb,kind,grouped", list(forms()))
def test_the_function_its_leading_arguments_and_its_output_buffers(rec, verb, kind, grouped):
    c, r = rec
    front, dates, lead, group_lead, nrows = ROWS[kind]
    name = PREFIX[kind] + verb
    kw = dict(dates)
    G = 0
    if grouped is not None:
        kw["groups"] = GROUPS[grouped]
        G = 3 if grouped == "labels" else 4
        lead = dict(group_lead, labels=("int32", (N,), LAB.astype(np.int32).tobytes()), ngroups=G)
    g = (G,) if G else ()
    if verb == "quantiles":
        got = getattr(c, name)(*front(name), PROBS, weights=W, counts=True, **kw)
        own = dict(weights=f64(W), probs=f64(PROBS), nprobs=3)
        outs = dict(out=("float64", g + (nrows, 3), None), n_part=("int64", g + (nrows,), None))
        assert [(a.dtype, a.shape) for a in got] == [(np.float64, g + (nrows, 3)), (np.int64, g + (nrows,))]
    elif verb == "probabilities":
        got = getattr(c, name)(*front(name), EDGES, counts=True, sums=True, **kw)
        own = dict(weights=None, edges=f64(EDGES), nedges=2)
        outs = dict(prob=("float64", g + (nrows, 3), None), sums=("uint64", g + (nrows, 3), None),
                    n_part=("int64", g + (nrows,), None))
        assert [(a.dtype, a.shape) for a in got] == [(np.float64, g + (nrows, 3)), (np.int64, g + (nrows,)),
                                                     (np.uint64, g + (nrows, 3))]
    elif verb == "moments":
        pred = np.stack([np.linspace(2.0, 4.5, N), np.arange(N, dtype=np.float64)])
        got = getattr(c, name)(*front(name), weights=W, against=["S", pred[1]], **kw)
        own = dict(weights=f64(W), predictors=f64(pred), npred=2)
        outs = dict(shift=("float64", g + (nrows,), None), sums=("float64", g + (nrows, 8), None),
                    wsum=("uint64", g + (nrows,), None), n_part=("int64", g + (nrows,), None))
        if G:
            outs["pshift"] = ("float64", (G, 2), None)
        assert type(got) is (GroupedMoments if G else Moments)
        assert (got.shift.shape, got.sums.shape, got.wsum.shape, got.n_part.shape, got.pshift.shape) == \
            (g + (nrows,), g + (nrows, 8), g + (nrows,), g + (nrows,), g + (2,))
        assert (got.sums.dtype, got.wsum.dtype, got.n_part.dtype) == (np.float64, np.uint64, np.int64)
        assert got.names == ["S", "against[1]"]
        if G:
            assert len(got) == G and got[0].shift.shape == (nrows,)
    else:
        use = np.array([1, 0])
        got = getattr(c, name)(*front(name), ["a", "b"] if kind == "metric" else 1, n_base=2, use=use, **kw)
        k = 2 if kind == "metric" else 1
        own = dict(k=k, n_base=2, use=("uint8", (2,), bytes([1, 0])))
        outs = dict(shift=("float64", (nrows,), None), sums=("float64", (nrows, 4 + 4 * k), None),
                    n_part=("int64", (nrows,), None))
        assert type(got) is Sobol and got.sums.shape == (nrows, 4 + 4 * k) and got.n_part.dtype == np.int64
    fn, args = r.named()
    assert fn == ("hx_group_" if G else STEM[kind]) + verb
    want = dict(lead, **own, **outs)
    assert list(args) == SIG[fn].replace(">", "").split() and set(args) == set(want)   # (position by position)
    for key in want:
        assert args[key] == want[key], (fn, key)


def test_member_metrics_ranks_and_defaults(rec):
    c, r = rec
    out = c.metrics(VAR, SPECS)
    fn, a = r.named()
    assert fn == "hx_member_metrics" and out.shape == (2, N) and a["out"] == ("float64", (2, N), None)
    assert a["specs"][2] == spec_bytes(SPECS) and a["nspecs"] == 2
    out = c.pair_metrics(VAR, BVEC, PSPECS[0])
    fn, a = r.named()
    assert fn == "hx_member_pair_metrics" and out.shape == (1, N) and a["out"] == ("float64", (1, N), None)
    assert (a["cap_b"], a["b_vec"], a["b_year0"], a["b_year1"], a["nspecs"]) == (None, f64(BVEC[1]), 1750, 1760, 1)
    out = c.metric_ranks(VAR, SPECS[0], weights=W, kind="numerator")
    fn, a = r.named()
    assert fn == "hx_metric_ranks" and out.shape == (1, N)
    assert (a["nspecs"], a["weights"], a["kind"], a["out"]) == (1, f64(W), 1, ("float64", (1, N), None))
    assert c.rank_series("r", VAR, (1751, 1753)) is c
    assert r.named() == ("hx_series_rank", dict(name=b"r", capability=VAR.encode(), year0=1751, year1=1753,
                                                weights=None, kind=0))
    c.rank_series("r", VAR)
    assert r.named()[1]["year0"] == START and r.named()[1]["year1"] == RUN_TO
    # no weights, no counts, one probability, no use: NULL, the bare array, n_base from the members
    q = c.quantiles(VAR, 0.5, (1750, 1751))
    a = r.named()[1]
    assert q.shape == (2, 1) and a["weights"] is None and a["nprobs"] == 1
    p = c.metric_probabilities(VAR, SPECS, 0.0, sums=True)
    assert isinstance(p, tuple) and len(p) == 2 and p[1].dtype == np.uint64
    s = c.sobol(VAR, 3, (1750, 1750))
    a = r.named()[1]
    assert (a["k"], a["n_base"], a["use"]) == (3, N // 5, None) and s.names == ["factor[0]", "factor[1]", "factor[2]"]
    m = c.moments(VAR, (1750, 1751))
    a = r.named()[1]
    assert (a["weights"], a["predictors"], a["npred"]) == (None, None, 0) and m.sums.shape == (2, 2)


def test_against_takes_each_kind_of_entry_through_one_call_each(rec):
    c, r = rec
    r.log.clear()
    m = c.metric_moments(VAR, SPECS, against=["S", (VAR, SPECS[0]), (VAR, "CO2_concentration", PSPECS[0]),
                                               np.arange(N)])
    assert [fn for fn, _ in r.log] == ["hx_getvar", "hx_member_metrics", "hx_member_pair_metrics", "hx_metric_moments"]
    a = r.named()[1]
    assert a["npred"] == 4 and a["predictors"][:2] == ("float64", (4, N)) and m.sums.shape == (2, 14)
    pred = np.frombuffer(a["predictors"][2]).reshape(4, N)
    assert np.array_equal(pred[0], np.linspace(2.0, 4.5, N)) and np.array_equal(pred[3], np.arange(N))
    assert np.isfinite(pred).all()   # (the metrics are the emulation's own)


VERBS = [   # (public name, a call with the keyword arguments of the case; takes groups, probs / edges)
    ("quantiles", lambda c, **kw: c.quantiles(VAR, kw.pop("probs", 0.5), **kw), True, "probs"),
    ("metric_quantiles", lambda c, **kw: c.metric_quantiles(VAR, kw.pop("specs", SPECS), kw.pop("probs", 0.5), **kw),
     True, "probs"),
    ("pair_metric_quantiles",
     lambda c, **kw: c.pair_metric_quantiles(VAR, "CO2_concentration", kw.pop("specs", PSPECS), kw.pop("probs", 0.5), **kw),
     False, "probs"),
    ("probabilities", lambda c, **kw: c.probabilities(VAR, kw.pop("edges", [0.0]), **kw), True, "edges"),
    ("metric_probabilities",
     lambda c, **kw: c.metric_probabilities(VAR, kw.pop("specs", SPECS), kw.pop("edges", [0.0]), **kw), True, "edges"),
    ("pair_metric_probabilities",
     lambda c, **kw: c.pair_metric_probabilities(VAR, BVEC, kw.pop("specs", PSPECS), kw.pop("edges", [0.0]), **kw),
     False, "edges"),
    ("moments", lambda c, **kw: c.moments(VAR, **kw), True, None),
    ("metric_moments", lambda c, **kw: c.metric_moments(VAR, kw.pop("specs", SPECS), **kw), True, None),
    ("pair_metric_moments",
     lambda c, **kw: c.pair_metric_moments(VAR, "CO2_concentration", kw.pop("specs", PSPECS), **kw), False, None),
    ("sobol", lambda c, **kw: c.sobol(VAR, 1, **kw), False, None),
    ("metric_sobol", lambda c, **kw: c.metric_sobol(VAR, kw.pop("specs", SPECS), 1, **kw), False, None),
]


@pytest.mark.parametrize("name,call,has_groups,axis", VERBS, ids=[v[0] for v in VERBS])
def test_every_form_raises_the_shared_argument_errors_under_its_own_name(rec, name, call, has_groups, axis):
    c, r = rec
    r.log.clear()
    good = np.arange(N) % 2
    for groups in ((None, good) if has_groups else (None,)):
        kw = {} if groups is None else {"groups": groups}
        if "sobol" not in name:
            with pytest.raises(E, match="^%s: weights must have n_members entries$" % name):
                call(c, weights=np.ones(N + 1), **kw)
            with pytest.raises(E, match="^%s: weights must have n_members entries$" % name):
                call(c, weights=np.ones((N, 1)), **kw)
        else:
            with pytest.raises(E, match="^%s: use must have n_base entries$" % name):
                call(c, use=np.ones(3), **kw)
            with pytest.raises(E, match="^%s: at most 16 factors$" % name):
                (c.sobol(VAR, 17) if name == "sobol" else c.metric_sobol(VAR, SPECS, 17))
        if axis:   # (ungrouped quantiles() included: it used to flatten a two-dimensional probs)
            with pytest.raises(E, match="^%s: %s must be one-dimensional$" % (name, axis)):
                call(c, **{axis: np.full((2, 2), 0.5)}, **kw)
        if "metric" in name:
            of = "PairMetric" if name.startswith("pair") else "Metric"
            for bad in (["mean"], PSPECS if of == "Metric" else SPECS):
                with pytest.raises(E, match="^%s: specs must be hector_amd.%s objects$" % (name, of)):
                    call(c, specs=bad, **kw)
    if has_groups:
        for bad, text in ((np.zeros(N), "the labels of groups must be integers \\(dtype float64\\)"),
                          (good.astype(bool), "the labels of groups must be integers \\(dtype bool\\)"),
                          (np.zeros(N - 1, dtype=np.int64), "groups must have n_members labels"),
                          (np.zeros((N, 1), dtype=np.int64), "groups must have n_members labels"),
                          ((good, 17), "the number of groups must lie in 1..16 \\(it is 17\\)"),
                          ((good, 0), "the number of groups must lie in 1..16 \\(it is 0\\)"),
                          (np.full(N, -1), "the number of groups must lie in 1..16 \\(it is 0\\)"),
                          ((good, 2.0), "the number of groups must be an integer"),
                          ((np.where(np.arange(N) == 3, 5, good), 3), "label 5 lies outside -1..2"),
                          (np.where(np.arange(N) == 3, -2, good), "label -2 lies outside -1..1")):
            with pytest.raises(E, match="^%s: %s$" % (name, text)):
                call(c, groups=bad)
    if name.startswith("pair"):
        with pytest.raises(E, match="^%s: b is a variable name or a \\(years, values\\) pair$" % name):
            getattr(c, name)(VAR, 3, PSPECS, *([[0.5]] if axis else []))
        with pytest.raises(E, match="^%s: the vector b needs one value per year$" % name):
            getattr(c, name)(VAR, ([1750, 1751], [1.0]), PSPECS, *([[0.5]] if axis else []))
        with pytest.raises(E, match="^%s: the years of the vector b must be consecutive and ascending$" % name):
            getattr(c, name)(VAR, ([1750, 1752], [1.0, 2.0]), PSPECS, *([[0.5]] if axis else []))
    assert not [fn for fn, _ in r.log if fn in SIG and fn not in ANSWERED]   # none of them reached a verb's call
