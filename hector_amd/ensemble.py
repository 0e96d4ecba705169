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
