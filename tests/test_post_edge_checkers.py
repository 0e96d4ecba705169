"""The checkers that tests/test_gpu_post_edges.py trusts, held to brute force on the rows it uses
(tests/post_edge_cases.py).  No GPU: the quantile checker against an expansion (every value repeated
q times, sorted) and numpy's inverted_cdf, `bin_reference` against a Python loop, the moments checker
against fractions.Fraction sums, and the condition under which the moments bound holds -- every term
of the sums exactly 0 or a normal double -- on the generated rows of every size.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import post_edge_cases as pe
from test_gpu_quantiles import checker as quantile_checker, quantise
from test_gpu_metrics_probabilities import bin_reference
from test_gpu_moments import checker as moments_checker

LD = np.longdouble
SMALL = (1, 63, 65, 257)


def test_generators_cover_what_the_gpu_tests_assert():
    pads = [pe.npad_of(n) - n for n in pe.SIZES]
    assert any(p > 0 for p in pads) and any(p == 0 for p in pads)
    assert {pe.nprobs_of(n) for n in pe.SIZES} == set(range(1, 17))
    assert {k for n in pe.SIZES for k in pe.npred_for(n)} == set(range(9))
    assert len(pe.ALL_ROWS) <= pe.RUN_TO - pe.FIRST_ROW_YEAR + 1
    for n in pe.SIZES + pe.HOSTILE_SIZES:
        r = pe.rows(n)
        assert tuple(r) == pe.ALL_ROWS and all(v.shape == (n,) and v.dtype == np.float64 for v in r.values())
        beg, end = pe.last_chunk(n)
        assert 0 <= beg < end == n and end - beg <= pe.CHUNK and beg % pe.CHUNK == 0
        assert not np.isnan(r["only the last member"][n - 1]) and np.isnan(r["only the last member"][:n - 1]).all()
        assert not np.isnan(r["only member 0"][0]) and np.isnan(r["only member 0"][1:]).all()
        ws = pe.weight_settings(n)
        assert ws["none"] is None and np.count_nonzero(ws["one"]) == 1 and ws["one"][n - 1] > 0
        if n > 1:
            assert (quantise(ws["wide"]) == 0).any() and (quantise(ws["wide"]) > 0).any()
            lace = np.isnan(r["NaN in the last chunk"])
            if beg and end - beg >= 64:
                assert lace[beg:].mean() > 4 * lace[:beg].mean()      # concentrated in the last chunk
        if n >= 63:
            x = pe.matrix(r, pe.ALL_ROWS)
            assert all(np.isin(x, e).any() for e in pe.EDGE_SETS)      # members exactly on edges
    for n in pe.SERIES_SIZES:
        a, b = pe.hostile_block(n, 11), pe.hostile_block(n, 12)
        for special in (np.inf, -np.inf, 0.0, pe.TINY, 1e300):
            assert (a == special).any() and (b == special).any()
        assert (np.signbit(b) & (b == 0)).any() and np.isnan(a).any()
        assert (np.isinf(a) & np.isinf(b) & (a == b)).any()
        assert ((b == 0) & (a == 0)).any() and ((b == 0) & (a != 0) & ~np.isnan(a)).any()


@pytest.mark.parametrize("n", SMALL)
def test_quantile_checker_against_an_expansion(n):
    r = pe.rows(n)
    rng = np.random.default_rng(n)
    probs = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
    for name in pe.ALL_ROWS:
        x = r[name]
        for q in (np.ones(n, dtype=np.uint64), rng.integers(0, 4, n).astype(np.uint64)):
            got, cnt = quantile_checker(x, q, probs)
            part = ~np.isnan(x) & (q > 0)
            assert cnt == int(part.sum())
            if cnt == 0:
                assert np.isnan(got).all()
                continue
            flat = np.sort(np.repeat(x[part], q[part].astype(np.int64)))
            W = flat.size
            ref = np.array([flat[max(1, math.ceil(p * float(W))) - 1] for p in probs])
            assert (got == ref).all(), (n, name, got, ref)
            # p n is no integer for these sizes and probabilities: numpy's index is the same one
            if np.__version__ >= "2.0" and (q == 1).all() and part.all() and n > 1:
                assert (got[1:-1] == np.quantile(x, probs[1:-1], method="inverted_cdf")).all(), (n, name)
                assert got[0] == x.min() and got[-1] == x.max()


@pytest.mark.parametrize("n", SMALL)
def test_bin_reference_against_a_loop(n):
    r = pe.rows(n)
    rng = np.random.default_rng(n)
    for name in pe.ALL_ROWS:
        x = r[name]
        for q in (np.ones(n, dtype=np.uint64), pe.q_of(n, pe.weight_settings(n)["wide"]),
                  rng.integers(0, 3, n).astype(np.uint64)):
            for edges in pe.EDGE_SETS:
                sums, cnt = bin_reference(x, q, edges)
                ref, members = [0] * (len(edges) + 1), 0
                for v, w in zip(x.tolist(), q.tolist()):
                    if v != v or w == 0:
                        continue
                    ref[sum(1 for e in edges.tolist() if e <= v)] += w      # on an edge: the upper bin
                    members += 1
                assert [int(s) for s in sums] == ref and cnt == members, (n, name)


def _exact(v):
    """A longdouble with a 64-bit significand as an exact Fraction: two doubles hold it."""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - LD(hi)))


def test_moments_checker_against_fractions():
    n = 40
    r = pe.rows(63)
    names = [k for k in pe.MOMENT_ROWS]
    x = np.stack([r[k][:n] for k in names])
    pred = pe.predictors(63)[:3, :n]
    eps = float(np.finfo(LD).eps)
    for q in (np.ones(n, dtype=np.uint64), pe.q_of(n, pe.weight_settings(63)["wide"][:n])):
        ref = moments_checker(x, q, pred)
        ok = [m for m in range(n) if q[m] > 0 and all(math.isfinite(pred[j, m]) for j in range(3))]
        assert list(np.flatnonzero(ref["ok"])) == ok
        for j in range(3):
            assert ref["pshift"][j] == min(pred[j, m] for m in ok)
        for y in range(x.shape[0]):
            part = [m for m in ok if x[y, m] == x[y, m]]
            assert ref["n_part"][y] == len(part)
            if not part:
                assert np.isnan(ref["shift"][y]) and ref["wsum"][y] == 0 and (ref["sums"][y] == 0).all()
                continue
            c = min(x[y, m] for m in part)
            assert ref["shift"][y] == c and int(ref["wsum"][y]) == sum(int(q[m]) for m in part)
            d = {m: Fraction(float(np.float64(x[y, m]) - np.float64(c))) for m in part}          # one IEEE subtraction
            e = [{m: Fraction(float(np.float64(pred[j, m]) - np.float64(ref["pshift"][j]))) for m in part}
                 for j in range(3)]
            w = {m: int(q[m]) for m in part}
            exact = [sum(w[m] * d[m] for m in part), sum(w[m] * d[m] * d[m] for m in part)]
            for j in range(3):
                exact += [sum(w[m] * e[j][m] for m in part), sum(w[m] * e[j][m] ** 2 for m in part),
                          sum(w[m] * d[m] * e[j][m] for m in part)]
            for k, s in enumerate(exact):
                got = _exact(ref["sums"][y, k])
                assert abs(got - s) <= Fraction((len(part) + 3) * eps) * s, (names[y], k, float(got), float(s))


@pytest.mark.parametrize("n", sorted(set(pe.SIZES + pe.HOSTILE_SIZES)))
def test_every_term_of_the_moment_sums_is_zero_or_normal(n):
    """The condition of the moments bound, on the rows the GPU tests give the moments kernel."""
    r = pe.rows(n)
    x = pe.matrix(r, pe.MOMENT_ROWS)
    allp = pe.predictors(n)
    seen = 0
    for w in pe.weight_settings(n).values():
        q = pe.q_of(n, w)
        for k in (0, 8):
            ref = moments_checker(x, q, allp[:k])
            seen += pe.terms_zero_or_normal(x, q, allp[:k], ref)
    assert seen > 0
    # ... and it does tell: a denormal spread or an overflowing square is refused
    for name in ("denormals", "full range"):
        if n < 63:
            continue
        bad = r[name][None, :]
        q = pe.q_of(n, None)
        with pytest.raises(AssertionError):
            pe.terms_zero_or_normal(bad, q, allp[:0], moments_checker(bad, q, allp[:0]))
