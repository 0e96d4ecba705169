"""The verbs' device scratch grows, is reused and is released with the layout: a result must not
depend on what the buffer held or how large it was before (EnsembleCore::Scratch in
ensemble_core.hpp; the verbs in ensemble_post.cpp).

One core of 130 members (a ragged last wavefront), run 1745-1760.  Every scratch-owning family makes
the same call at a small shape, at a larger one that forces a regrow, and at the small one again;
then the core lays out its device memory anew (set_outputs with a different list and a run, twice,
so that it ends on the first list) and the small call is made once more.  Every result must equal,
bit for bit, the same call made FIRST on a fresh core.  Reuse-invariance only: parity with the
definitions is held by the other test_gpu_* files.

small: 1 year, 1 probability, 1 edge, 1 specification; large: 5 years, 3 probabilities, 4 edges,
9 specifications.  Sobol: the smallest valid Saltelli design (one factor, one group of three
members), then three factors in 26 groups.  The whitened score pads its matrix to 64, 128, 192 or
256 observations, so 1 and 5 years share one size of scratch: "score_whitened_wide" goes from 1 to 70
observations (the run's sixteen years, repeated), which does regrow.
"""
import numpy as np
import pytest

import hector_amd
from hector_amd import Metric, PairMetric, ensemble
from conftest import SCENARIO

pytestmark = pytest.mark.gpu

N, Y0, Y1 = 130, 1745, 1760
VAR, VAR_B = "global_tas", "CO2_concentration"
OUTPUTS = [VAR, VAR_B]
OPS = ("mean", "min", "max", "year_of_min", "year_of_max", "first_ge", "count_ge", "slope", "mean")
PAIR_OPS = ("slope", "intercept", "r2", "at_first_ge", "at_max", "at_min", "mean_where_ge", "end_ratio", "slope")


def _shape(large):
    ny, nprobs, nedges, nspecs = (5, 3, 4, 9) if large else (1, 1, 1, 1)
    years = np.arange(1750, 1750 + ny)
    specs = [Metric(OPS[i], (1746 + i % 3, 1760 - i % 4), baseline=(1745, 1747) if i % 2 else None,
                    threshold=0.02 * i) for i in range(nspecs)]
    pspecs = [PairMetric(PAIR_OPS[i], (1746 + i % 3, 1760 - i % 4), baseline=(1745, 1747) if i % 2 else None,
                         threshold=277.0 + 0.1 * i) for i in range(nspecs)]
    return dict(ny=ny, years=years, dates=(int(years[0]), int(years[-1])),
                probs=np.linspace(0.1, 0.9, nprobs) if large else np.array([0.5]),
                edges=np.linspace(-0.1, 0.2, nedges) if large else np.array([0.0]),
                specs=specs, pspecs=pspecs, obs=0.01 * np.arange(ny), nspecs=nspecs,
                sobol=(3, 26) if large else (1, 1),
                wide_years=Y0 + np.arange(70) % (Y1 - Y0 + 1) if large else years)


def _whiten(n):
    w = np.tril(0.1 * np.ones((n, n))) + np.eye(n)
    return w


FAMILIES = {
    "quantiles": lambda c, s: c.quantiles(VAR, s["probs"], s["dates"], counts=True),
    "metric_quantiles": lambda c, s: c.metric_quantiles(VAR, s["specs"], s["probs"], counts=True),
    "probabilities": lambda c, s: c.probabilities(VAR, s["edges"], s["dates"], counts=True, sums=True),
    "metrics": lambda c, s: c.metrics(VAR, s["specs"]),
    "pair_metrics": lambda c, s: c.pair_metrics(VAR, VAR_B, s["pspecs"]),
    "moments": lambda c, s: c.moments(VAR, s["dates"], against=["S"]),
    "group_quantiles": lambda c, s: c.quantiles(VAR, s["probs"], s["dates"], counts=True,
                                                groups=(np.arange(N) % 3, 3)),
    "sobol": lambda c, s: c.sobol(VAR, s["sobol"][0], s["dates"], n_base=s["sobol"][1]),
    "comoments": lambda c, s: c.comoments(VAR, s["dates"]),
    "score_whitened": lambda c, s: c.score(VAR, s["years"], s["obs"], whiten=_whiten(s["ny"])),
    "score_whitened_wide": lambda c, s: c.score(VAR, s["wide_years"], 0.002 * np.arange(len(s["wide_years"])),
                                                whiten=_whiten(len(s["wide_years"]))),
    "project": lambda c, s: c.project(VAR, s["years"], np.cos(np.arange(s["nspecs"] * s["ny"], dtype=float))
                                      .reshape(s["nspecs"], s["ny"])),
    "metric_ranks": lambda c, s: c.metric_ranks(VAR, s["specs"]),
    "crps": lambda c, s: c.crps(VAR, s["years"], s["obs"], return_pit=True, counts=True),
}
RAW = ("shift", "sums", "wsum", "n_part", "shift_a", "sums_a", "shift_b", "sums_b", "cross")
STAGES = ("small", "large", "small again", "small after a new layout")


def _arrays(res):
    """A verb's result as a tuple of arrays: its raw fields, for the result classes."""
    if isinstance(res, np.ndarray):
        return (res,)
    if isinstance(res, tuple):
        return tuple(a for r in res for a in _arrays(r))
    got = tuple(np.asarray(getattr(res, f)) for f in RAW if getattr(res, f, None) is not None)
    assert got, "no raw fields in %r" % (res,)
    return got


def _core(hip_lib):
    c = hector_amd.Core(SCENARIO, N, lib_path=hip_lib)
    S, q10 = ensemble.ecs_q10(N)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    c.set_outputs(OUTPUTS)
    c.run(Y1)
    return c


@pytest.fixture(scope="module")
def results(hip_lib):
    """-> (fresh, reused): fresh[(family, large)] from a core whose first verb call it is,
    reused[(family, stage)] from the one core that makes every call."""
    fresh, reused = {}, {}
    for name, call in FAMILIES.items():
        for large in (False, True):
            c = _core(hip_lib)
            fresh[(name, large)] = _arrays(call(c, _shape(large)))
            c.shutdown()
    c = _core(hip_lib)
    for name, call in FAMILIES.items():
        for stage, large in zip(STAGES[:3], (False, True, False)):
            reused[(name, stage)] = _arrays(call(c, _shape(large)))
    c.set_outputs(OUTPUTS + ["RF_tot"])
    c.run(Y1)
    c.set_outputs(OUTPUTS)
    c.run(Y1)
    for name, call in FAMILIES.items():
        reused[(name, STAGES[3])] = _arrays(call(c, _shape(False)))
    c.shutdown()
    return fresh, reused


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_result_does_not_depend_on_the_scratch_before(results, family, stage):
    fresh, reused = results
    want, got = fresh[(family, stage == "large")], reused[(family, stage)]
    assert len(want) == len(got)
    for w, g in zip(want, got):
        assert w.shape == g.shape and w.dtype == g.dtype
        assert w.tobytes() == g.tobytes(), (family, stage, w, g)


def test_the_shapes_differ_and_hold_values(results):
    """The larger call is another call (a whitened score is one number per member at any shape, so
    this compares the results, not their sizes), and both return numbers, not NaN throughout."""
    fresh, _ = results
    for name in FAMILIES:
        small, large = fresh[(name, False)], fresh[(name, True)]
        assert [a.tobytes() for a in large] != [a.tobytes() for a in small], name
        for res in (small, large):
            assert any(np.isfinite(a.astype(np.float64)).any() for a in res), name
