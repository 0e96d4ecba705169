"""Rows, weights, predictors and edges for the chunk, batch and template edges of the summary kernels
(hector_amd/csrc/hx_dev_post.h).  No tests here: tests/test_gpu_post_edges.py writes these rows into a
core and holds the kernels to the project's checkers; tests/test_post_edge_checkers.py holds the
checkers to brute force on the same rows.

The sizes come from the kernel constants: a workgroup takes HXQ_CHUNK = 256 x 32 = 8192 members of a
row, a lane 32 strided elements of them (i = beg + e 256 + tid), and the moments kernel goes through
those 32 in register batches of 32 (no predictors), 16 (1..3) or 8 (4..8), so that a chunk's
remainder of 2048 / 4096 / 6144 members is where a batch ends exactly.
"""
import numpy as np

CHUNK = 8192
SIZES = (1, 63, 64, 65, 255, 256, 257, 2048, 2049, 4097, 6145, 8191, 8192, 8193, 10240, 12289, 16384,
         16385, 24575)            # 10240 = 8192 + 2048, 12289 = 8192 + 4097, 24575 = 3 * 8192 - 1
HOSTILE_SIZES = (777, 12289)      # the moments on hostile rows
AB_SIZES = (257, 8193, 24575, 777)
METRIC_SIZES = (8193, 12289, 24575)
ALL_PREDICTOR_SIZES = (6145, 12289)
FIRST_ROW_YEAR = 1750             # the rows below go to the years 1750, 1751, ... of a core run to 1790
RUN_TO = 1790
TINY = 5e-324
DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308


def npad_of(n):
    return (n + 63) // 64 * 64


def last_chunk(n):
    """Index range of the last workgroup chunk of a row of n members."""
    beg = (n - 1) // CHUNK * CHUNK
    return beg, n


def rows(n):
    """name -> values[n], in the order in which they are written from FIRST_ROW_YEAR on.  Member
    order; the cores of the GPU tests run without member sorting, so it is the lane order too and
    'the last chunk' means the last workgroup's."""
    rng = np.random.default_rng(1000 + n)
    beg, _ = last_chunk(n)
    i = np.arange(n)
    in_last = i >= beg
    r = {}
    # --- part 1: every verb
    r["all equal"] = np.full(n, 3.25)
    r["two adjacent doubles"] = np.where(rng.random(n) < 0.3, 1.0, 1.0 + 2.0 ** -52)
    r["ties"] = np.round(rng.normal(0, 3, n))
    r["NaN in the last chunk"] = np.where(rng.random(n) < np.where(in_last, 0.7, 0.02), np.nan, rng.normal(0, 1, n))
    r["only the last member"] = np.where(i == n - 1, -7.0, np.nan)
    r["only member 0"] = np.where(i == 0, 2.5, np.nan)
    r["wide range"] = rng.normal(0, 1, n) * 10.0 ** rng.integers(-100, 101, n)
    # --- part 2: hostile rows the moments still take (every term of the sums 0 or a normal double)
    r["both zeros"] = rng.choice([-2.5, -1.0, -0.0, 0.0, 1.0], n)
    r["negatives"] = -rng.lognormal(0, 2, n)
    r["one value among NaN"] = np.where(i == (2 * n) // 3, -7.0, np.nan)
    r["all NaN"] = np.full(n, np.nan)
    r["NaN-laced"] = np.where(rng.random(n) < 0.4, np.nan, rng.normal(0, 1, n))
    r["1e-100 .. 1e100"] = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-100, 100, n)
    # --- integer arithmetic only (quantiles, bins): the hostile rows of tests/test_gpu_quantiles.py
    r["full range"] = rng.normal(0, 1, n) * 10.0 ** rng.integers(-300, 300, n)
    r["denormals"] = rng.integers(-40, 40, n) * TINY
    r["infinities"] = rng.choice([-np.inf, np.inf, 0.0, 1.0, -1.0], n)
    r["zeros and 1e-300"] = rng.choice([-2.5, -1.0, -0.0, 0.0, 1.0, -1e-300, 1e-300], n)
    return r


PART1_ROWS = ("all equal", "two adjacent doubles", "ties", "NaN in the last chunk", "only the last member",
              "only member 0", "wide range")
HOSTILE_MOMENT_ROWS = ("both zeros", "negatives", "one value among NaN", "all NaN", "NaN-laced", "1e-100 .. 1e100")
MOMENT_ROWS = PART1_ROWS + HOSTILE_MOMENT_ROWS
INTEGER_ONLY_ROWS = ("full range", "denormals", "infinities", "zeros and 1e-300")
ALL_ROWS = MOMENT_ROWS + INTEGER_ONLY_ROWS


def year_of(name):
    return FIRST_ROW_YEAR + ALL_ROWS.index(name)


def pad_value(k):
    """Poison of the padding lanes n..npad-1 of the k-th row: a read past n shows up in the answer."""
    return -1e300 if k % 2 else np.nan


def matrix(r, names):
    return np.stack([r[k] for k in names])


def weight_settings(n):
    """name -> weights[n] or None: no weights; a wide vector of which entries quantise to 0 (from
    n = 2 on: with one member its weight is the maximum); one weight, on the last member."""
    rng = np.random.default_rng(2000 + n)
    wide = 2.0 ** -rng.uniform(0, 40, n)
    wide[n // 2] = 1.0
    if n > 1:
        wide[0] = 2.0 ** -40          # rint(2^-8) = 0
    one = np.zeros(n)
    one[n - 1] = 0.7
    return {"none": None, "wide": wide, "one": one}


def probs_for(k):
    """k probabilities, 0 and 1 among them from two on."""
    return (0.5,) if k == 1 else tuple(np.linspace(0.0, 1.0, k))


def nprobs_of(n):
    """Every count 1..16 over SIZES: the select's pick kernel runs 64 threads a probability."""
    return SIZES.index(n) % 16 + 1 if n in SIZES else 9


EDGE_SETS = (np.array([3.25]),                                                  # the all-equal row sits on it
             np.array([-2.0, -1.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 2.0, 3.25]),     # both adjacent doubles are edges
             np.arange(-15.0, 16.0))                                            # 31: HX_BIN_MAX_EDGES


def predictors(n):
    """[8, n] finite per-member predictors, but for member n // 3 of the first (NaN) and member
    n // 5 of the fifth (inf) from n = 8 on: those members take no part when their row is used."""
    rng = np.random.default_rng(3000 + n)
    i = np.arange(n)
    p = np.stack([np.fmod(i * 0.6180339887498949, 1.0), np.cos(i * 0.001) * 3.0 - 40.0, (i % 97).astype(np.float64),
                  rng.normal(0, 1, n), (i + 0.5) / n, rng.lognormal(0, 1, n), -(i % 13).astype(np.float64),
                  rng.uniform(-1e3, 1e3, n)])
    if n >= 8:
        p[0, n // 3] = np.nan
        p[4, n // 5] = np.inf
    return p


def npred_for(n):
    """The predictor counts of a size: all nine at ALL_PREDICTOR_SIZES, elsewhere one of each batch
    size (32: none; 16: 1..3; 8: 4..8), moving with the size."""
    if n in ALL_PREDICTOR_SIZES:
        return tuple(range(9))
    k = SIZES.index(n) if n in SIZES else 0
    return (0, 1 + k % 3, 4 + k % 5)


def quantise(w):
    return np.rint(w / w.max() * 2.0 ** 32).astype(np.uint64)


def q_of(n, weights):
    return np.ones(n, dtype=np.uint64) if weights is None else quantise(np.asarray(weights, dtype=np.float64))


def terms_zero_or_normal(x, q, pred, ref):
    """The condition under which the bound (n_part + 8) 2^-53 of the sums holds: no term underflows
    or overflows.  ref: the record of the moments checker of tests/test_gpu_moments.py for
    (x[ny, n], q, pred[K, n]); its own d = x - shift and e = p - pshift (float64) and q give the
    terms q d, q d d, q e, q e e, q d e, formed here in longdouble (no underflow there): every one must
    be exactly 0 or a normal double.  -> the number of terms looked at."""
    LD = np.longdouble
    idx = np.flatnonzero(ref["ok"])
    wl = q[idx].astype(LD)
    seen = 0

    def good(t):
        a = np.abs(t)
        return bool(((a == 0) | ((a >= LD(DBL_MIN)) & (a <= LD(DBL_MAX)))).all())

    es = [(pred[j, idx] - ref["pshift"][j]).astype(LD) for j in range(pred.shape[0])]
    for e in es:
        assert good(wl * e) and good(wl * e * e)
        seen += 2 * e.size
    for y in range(x.shape[0]):
        xv = x[y, idx]
        part = ~np.isnan(xv)
        if not part.any():
            continue
        d = (xv[part] - ref["shift"][y]).astype(LD)
        w = wl[part]
        assert good(w * d) and good(w * d * d), y
        seen += 2 * d.size
        for e in es:
            assert good(w * d * e[part]), y
            seen += d.size
    return seen


# ---- the series, score and metric kernels on hostile content -------------------------------------

SERIES_SIZES = (200, 257)     # npad 256 and 320
HOSTILE_POOL = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, TINY, -TINY, 3 * TINY, -17 * TINY, 1e300, -1e300,
                         1e-300, -1e-300])


def hostile_block(n, seed, ny=RUN_TO - 1745 + 1):
    """[ny, n]: two thirds ordinary values, one third drawn from HOSTILE_POOL."""
    rng = np.random.default_rng(seed + n)
    x = rng.normal(0, 2, (ny, n))
    return np.where(rng.random((ny, n)) < 1.0 / 3.0, HOSTILE_POOL[rng.integers(0, HOSTILE_POOL.size, (ny, n))], x)


def hostile_vector(ny, seed):
    """A per-year operand: ordinary values with +-0.0, +-inf, NaN and denormals among them."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 2, ny)
    v[::5] = HOSTILE_POOL[rng.integers(0, HOSTILE_POOL.size, v[::5].size)]
    v[1], v[2] = 0.0, -0.0
    return v


def same_bits(got, ref, what):
    """The NaN masks equal, and the bit patterns equal elsewhere: a zero of the wrong sign or a
    flushed denormal fails."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN masks", np.argwhere(gn != rn)[:5])
    g, r = np.where(gn, 0.0, got).view(np.uint64), np.where(rn, 0.0, ref).view(np.uint64)
    bad = np.argwhere(g != r)
    assert bad.size == 0, (what, bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])
