"""Synthetic perturbed-parameter ensembles: counter-based, so
member i gets the same parameters on any rank / any shard layout."""
import numpy as np

SEED = 20260928


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform01(member_index, stream, seed=SEED):
    """U[0,1) for (member, stream) pairs; member_index: int array."""
    with np.errstate(over="ignore"):
        i = np.asarray(member_index, dtype=np.uint64)
        k = _splitmix64(np.uint64(seed) + i * np.uint64(0x632BE59BD9B4E019) +
                        np.uint64(stream) * np.uint64(0xD1B54A32D192ED03))
        k = _splitmix64(k)
    return (k >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def ecs_q10(n, offset=0, seed=SEED):
    """BASELINE configs 2-4: S ~ U(1.5, 6.0) degC, q10_rh ~ U(1.0, 3.0)."""
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    S = 1.5 + 4.5 * uniform01(idx, 0, seed)
    q10 = 1.0 + 2.0 * uniform01(idx, 1, seed)
    return S, q10


def biome4(n, offset=0, seed=SEED, wf_base=1.0):
    """BASELINE config 5: 4 equal biomes, warmingfactor = wf*(1+0.5b),
    q10_rh ~ U(1,3) per biome, S ~ U(1.5,6)."""
    idx = np.arange(offset, offset + n, dtype=np.uint64)
    S = 1.5 + 4.5 * uniform01(idx, 0, seed)
    q10 = [1.0 + 2.0 * uniform01(idx, 10 + b, seed) for b in range(4)]
    wf = [np.full(n, wf_base * (1 + 0.5 * b)) for b in range(4)]
    return S, q10, wf


def saltelli(n_base, k, offset=0, seed=SEED):
    """A Saltelli (A, B, AB_i) design for variance-based sensitivity indices -> U[(k + 2) * n_base, k]
    in [0, 1), in the interleaved layout Core.sobol reads: the group of base point j is the k + 2
    consecutive rows j * (k + 2) + r, with r = 0 the point A_j, r = 1 the point B_j and r = 2 + i the
    point A_j with column i taken from B_j.  Counter-based like ecs_q10: base point offset + j has
    A[:, i] = uniform01(offset + j, i) and B[:, i] = uniform01(offset + j, k + i), so a larger call
    or another offset gives the same rows.  The caller maps the columns to parameter ranges."""
    n_base, k = int(n_base), int(k)
    if n_base < 1 or k < 1:
        raise ValueError("saltelli: n_base and k must be at least 1")
    idx = np.arange(offset, offset + n_base, dtype=np.uint64)
    A = np.stack([uniform01(idx, i, seed) for i in range(k)], axis=1)
    B = np.stack([uniform01(idx, k + i, seed) for i in range(k)], axis=1)
    U = np.repeat(A[:, None, :], k + 2, axis=1)          # [n_base, k + 2, k]
    U[:, 1, :] = B
    for i in range(k):
        U[:, 2 + i, i] = B[:, i]
    return U.reshape(n_base * (k + 2), k)


def quantise(weights, n):
    """The integer weights every weighted summary verb uses (include/hector_amd.h): q = rint(w / wmax *
    2^32) as uint64 [n]; None: every member 1."""
    if weights is None:
        return np.ones(int(n), dtype=np.uint64)
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (int(n),):
        raise ValueError("weights must have one entry per member")
    if not (np.isfinite(w).all() and (w >= 0).all() and w.max() > 0):
        raise ValueError("weights must be finite, not negative and not all zero")
    return np.rint(w / w.max() * 2.0 ** 32).astype(np.uint64)


def _midpit_row(x, q, kind):
    x = x + 0.0                                   # -0.0 and +0.0 tie
    part = ~np.isnan(x)
    out = np.full(x.shape, np.nan)
    W = int(q[part].sum(dtype=np.uint64))
    if W == 0:
        return out
    xs = x[part]
    order = np.argsort(xs, kind="stable")
    v = xs[order]
    cum = np.cumsum(q[part][order], dtype=np.uint64)
    lo = np.searchsorted(v, xs, side="left")
    hi = np.searchsorted(v, xs, side="right")
    L = np.where(lo > 0, cum[np.maximum(lo, 1) - 1], np.uint64(0)).astype(np.uint64)
    num = (L + cum[hi - 1]).astype(np.float64)    # 2 L + E: an integer <= 2 W <= 2^53, exact in double
    out[part] = num / np.float64(2 * W) if kind == "pit" else num
    return out


def midpit(values, weights=None, kind="pit"):
    """Every member's weighted mid-rank within its row, as hx_series_rank defines it
    (include/hector_amd.h): with q the integer weights, L_i = sum of q_j with x_j < x_i, E_i = sum of
    q_j with x_j == x_i and W = sum q over the values that are not NaN, kind "pit" gives
    (2 L_i + E_i) / (2 W) -- one double division of two exact integers -- and kind "numerator" gives
    2 L_i + E_i.  NaN stays NaN; a row with W = 0 is all NaN.  values: [n] or [rows, n] -> the same
    shape.  With weights=None this is (average rank - 0.5) / n, and what Core.rank_series,
    Core.metric_ranks and Core.spearman hold on the device, bit for bit."""
    if kind not in ("pit", "numerator"):
        raise ValueError("midpit: kind must be 'pit' or 'numerator'")
    x = np.asarray(values, dtype=np.float64)
    if x.ndim not in (1, 2):
        raise ValueError("midpit: values must be [n] or [rows, n]")
    q = quantise(weights, x.shape[-1])
    if x.ndim == 1:
        return _midpit_row(x, q, kind)
    return np.stack([_midpit_row(r, q, kind) for r in x]) if x.shape[0] else np.empty_like(x)


def _crps_row(x, y, q, dt):
    nan = (dt(np.nan), np.nan, 0, 0)
    x = x + 0.0
    y = np.float64(y) + 0.0
    part = ~np.isnan(x) & (q > 0)
    if np.isnan(y) or not part.any():
        return nan
    v, inv = np.unique(x[part], return_inverse=True)
    c = np.zeros(v.size, dtype=np.uint64)
    np.add.at(c, inv.ravel(), q[part])
    C = np.cumsum(c, dtype=np.uint64)
    W = C[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        F = C[:-1].astype(dt) / dt(W)
        G = (W - C[:-1]).astype(dt) / dt(W)
        FF, GG = F * F, G * G
        a, b, yy = v[:-1].astype(dt), v[1:].astype(dt), dt(y)
        inside = (yy > a) & (yy < b)
        first = np.where(yy <= a, (b - a) * GG, np.where(yy >= b, (b - a) * FF, (yy - a) * FF))
        second = (b - yy)[inside] * GG[inside]
        terms = [first, second]
        if y < v[0]:
            terms.append(np.array([dt(v[0]) - yy]))
        if y > v[-1]:
            terms.append(np.array([yy - dt(v[-1])]))
        total = np.concatenate(terms).sum(dtype=dt)
    lt = int(q[part][x[part] < y].sum(dtype=np.uint64))
    eq = int(q[part][x[part] == y].sum(dtype=np.uint64))
    pit = np.float64(2 * lt + eq) / np.float64(2 * int(W))
    return total, pit, int(part.sum()), int(v.size)


def crps(values, obs, weights=None, dtype=np.float64, full=False):
    """The continuous ranked probability score of a weighted ensemble row against an observation, as
    hx_ensemble_crps defines it (include/hector_amd.h): over the distinct values v_1 < ... < v_m of the
    members with q > 0 and a value that is not NaN, with C_k the running integer sum of q, F_k = C_k / W
    and G_k = (W - C_k) / W, the sum of (v_(k+1) - v_k) G_k^2 left of the observation, (v_(k+1) - v_k)
    F_k^2 right of it, the two parts of the gap that holds it, and the distance to the nearest value
    if it lies outside them all.  values [n] with a scalar obs, or [rows, n] with obs[rows].  dtype:
    the type the terms and their sum are evaluated in (np.longdouble for a reference).  full=True:
    -> (crps, pit_obs, n_part, m): also the observation's own mid-PIT, the members that took part and
    the number of distinct values (the error bound of the double sum is (m + 8) 2^-53, relatively)."""
    x = np.asarray(values, dtype=np.float64)
    if x.ndim not in (1, 2):
        raise ValueError("crps: values must be [n] or [rows, n]")
    q = quantise(weights, x.shape[-1])
    if x.ndim == 1:
        r = _crps_row(x, obs, q, dtype)
        return r if full else r[0]
    y = np.asarray(obs, dtype=np.float64)
    if y.shape != (x.shape[0],):
        raise ValueError("crps: one observation per row")
    rows = [_crps_row(x[i], y[i], q, dtype) for i in range(x.shape[0])]
    out = (np.array([r[0] for r in rows], dtype=dtype), np.array([r[1] for r in rows], dtype=np.float64),
           np.array([r[2] for r in rows], dtype=np.int64), np.array([r[3] for r in rows], dtype=np.int64))
    return out if full else out[0]
