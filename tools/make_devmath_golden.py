#!/usr/bin/env python3
"""Reference values for the device-math probe (tests/devmath/, tests/devmath/devmath_checks.py).

    python tools/make_devmath_golden.py      ->  tests/golden/devmath_reference.npz

For every operation of the probe the file holds the inputs (float64, from a fixed seed, plus the
structured points: reduction boundaries, powers of two, exact cases, the ends of each contract) and
the MATHEMATICAL result at 200 bits (mpmath), split as

    ref_hi  float64   the exact result, correctly rounded
    ref_lo  float32   (exact - ref_hi) / ulp(ref_hi), in [-0.5, 0.5]

so that a test measures an error in ulps as (got - ref_hi) / ulp(ref_hi) - ref_lo, good to ~1e-7
ulp, without mpmath or long double at test time.  ulp(y) = 2^(e - 52) for 2^e <= |y| < 2^(e+1).

The references are the functions themselves, no implementation: exp, log, sqrt, 1/b, a/b,
min(x, 1e30)^(-1/3), x^(-1/5), 1 - erfc(-d)/2, and the six T-only equilibrium constants of
src/ocean_csys.cpp:205-287 at S = 34.5 (K0, Kw, 1/Kh, K1, K2, Kb) -- the latter twice:

  chemfit_*   the formulas with their constants as printed (decimal, sqrt(34.5) exact): what
              tools/make_chem_fit.py fitted and profiles/chem_fit_report.json measures against;
              the reference of chem_constants_fit.
  chemform_*  the formulas with every constant taken as the DOUBLE the kernels hold
              (hx_fill_chem_table: 273.15, 0.01, the literal ln 100, the literal sqrt(34.5), products
              like 0.01615 * S folded in double): the reference of the formula path, whose bound
              counts roundings of the evaluation only.  With it, per point and constant, `sumabs`:
              the sum of the absolute values of the terms of the exponential's argument.
  The two differ by up to a few 1e-15 relative (Kb: the literal sqrt(34.5) and 8966.90 as doubles,
  multiplied by terms of magnitude 10 ... 60), which is why they are kept apart."""
import os

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "devmath_reference.npz")
SEED = 20260511
PREC = 200
M = mp.mpf


def rnd(x):
    """The double nearest to x (ties to even)."""
    x = M(x)
    if x == 0:
        return 0.0
    with mp.workprec(53):
        return float(+x)


def ulp(y):
    return np.spacing(np.abs(np.asarray(y, dtype=np.float64)))


def split(exact):
    """[mpf] -> ref_hi (float64), ref_lo (float32, in ulps of ref_hi)."""
    hi = np.array([rnd(v) for v in exact], dtype=np.float64)
    u = ulp(hi)
    lo = np.array([float((v - M(h)) / M(uu)) for v, h, uu in zip(exact, hi, u)], dtype=np.float32)
    return hi, lo


def neighbours(v):
    """The two doubles around the real number v."""
    d = rnd(v)
    return (d, float(np.nextafter(d, np.inf))) if M(d) <= v else (float(np.nextafter(d, -np.inf)), d)


def mp_exp_of(u):
    return np.array([rnd(mp.exp(M(float(x)))) for x in u])


# ---- the carbonate constants --------------------------------------------------------------------
def chem_decimal(Tc):
    """src/ocean_csys.cpp:205-287 at S = 34.5, constants as printed (tools/make_chem_fit.py)."""
    S = M("34.5"); sqrtS = mp.sqrt(S); S15 = S ** M("1.5")
    Tk = Tc + M("273.15"); lnTk = mp.log(Tk); lnTk100 = mp.log(Tk / 100); T100 = Tk / 100
    K0 = mp.exp(M("-58.0931") + M("90.5069") * (100 / Tk) + M("22.2940") * lnTk100 +
                S * (M("0.027766") - M("0.025888") * T100 + M("0.0050578") * T100 * T100))
    Kw = mp.exp(M("-13847.26") / Tk + M("148.96502") - M("23.6521") * lnTk +
                (M("118.67") / Tk - M("5.977") + M("1.0495") * lnTk) * sqrtS - M("0.01615") * S)
    Kh = mp.exp(M("9345.17") / Tk - M("60.2409") + M("23.3585") * lnTk100 +
                S * (M("0.023517") - M("0.00023656") * Tk + M("0.0047036e-4") * Tk * Tk))
    pK1 = M("3633.86") / Tk - M("61.2172") + M("9.6777") * lnTk - M("0.011555") * S + M("0.0001152") * S * S
    pK2 = M("471.78") / Tk + M("25.9290") - M("3.16967") * lnTk - M("0.01781") * S + M("0.0001122") * S * S
    Kb = mp.exp((M("-8966.90") - M("2890.53") * sqrtS - M("77.942") * S + M("1.728") * S15 - M("0.0996") * S * S) / Tk +
                M("148.0248") + M("137.1942") * sqrtS + M("1.62142") * S +
                (M("-24.4344") - M("25.085") * sqrtS - M("0.2474") * S) * lnTk + M("0.053105") * sqrtS * Tk)
    return [K0, Kw, 1 / Kh, M(10) ** (-pK1), M(10) ** (-pK2), Kb]


def chem_table():
    """hx_fill_chem_table (hx_dev_chem.h): the same expressions in IEEE double."""
    S = 34.5
    sqrtS = 5.873670062235365; S15 = 202.64161714712009; LN10 = 2.302585092994045684
    return [273.15, 0.01, 4.605170185988092, -58.0931, 9050.69, 22.2940, S, 0.027766, 0.025888,
            0.0050578, -13847.26, 148.96502, 23.6521, 118.67, 5.977, 1.0495, sqrtS, 0.01615 * S,
            9345.17, 60.2409, 23.3585, 0.023517, 0.00023656, 0.0047036e-4, 3633.86, 61.2172, 9.6777,
            0.011555 * S, 0.0001152 * S * S, LN10, 471.78, 25.9290, 3.16967, 0.01781 * S,
            0.0001122 * S * S,
            (-8966.90 - 2890.53 * sqrtS - 77.942 * S + 1.728 * S15 - 0.0996 * S * S),
            +148.0248 + 137.1942 * sqrtS + 1.62142 * S,
            +(-24.4344 - 25.085 * sqrtS - 0.2474 * S), 0.053105 * sqrtS]


def chem_doubles(Tc):
    """The six constants with chem_exponents' constants as the doubles of hx_fill_chem_table, exact
    arithmetic otherwise; and the sum of |terms| of each exponential's argument."""
    c = [M(v) for v in chem_table()]
    Tk = M(Tc) + c[0]; r = 1 / Tk; ln = mp.log(Tk); T100 = Tk * c[1]; S = c[6]
    terms = [
        [c[3], c[4] * r, c[5] * ln, -c[5] * c[2], S * c[7], -S * c[8] * T100, S * c[9] * T100 * T100],
        [c[10] * r, c[11], -c[12] * ln, c[13] * r * c[16], -c[14] * c[16], c[15] * ln * c[16], -c[17]],
        [-c[18] * r, c[19], -c[20] * ln, c[20] * c[2], -S * c[21], S * c[22] * Tk, -S * c[23] * Tk * Tk],
        [-c[24] * r * c[29], c[25] * c[29], -c[26] * ln * c[29], c[27] * c[29], -c[28] * c[29]],
        [-c[30] * r * c[29], -c[31] * c[29], c[32] * ln * c[29], c[33] * c[29], -c[34] * c[29]],
        [c[35] * r, c[36], c[37] * ln, c[38] * Tk],
    ]
    return [mp.exp(mp.fsum(t)) for t in terms], [mp.fsum(abs(x) for x in t) for t in terms]


# ---- inputs -------------------------------------------------------------------------------------
def inputs():
    rng = np.random.default_rng(SEED)
    ln2 = mp.ln2
    g = {}
    bnd = [x for k in (-1000, -1, 0, 1, 1000) for x in neighbours((k + M(1) / 2) * ln2)]
    g["exp_x"] = np.concatenate([rng.uniform(-700, 700, 500), rng.uniform(-1, 1, 500), bnd,
                                 [0.0, -0.0, rnd(ln2 / 2), -rnd(ln2 / 2), 699.9, -699.9]])
    g["exp1_extra_x"] = np.array([-746.0, -800.0, -np.inf])
    s12 = neighbours(mp.sqrt(M(1) / 2))
    g["log_x"] = np.concatenate([
        mp_exp_of(rng.uniform(-700, 700, 400)), rng.uniform(0.5, 2, 300),
        1 + rng.uniform(0, 1e-6, 150), 1 - rng.uniform(0, 1e-6, 150), s12,
        [float(np.nextafter(1.0, 0.0)), 1.0, float(np.nextafter(1.0, 2.0))],
        [2.0 ** k for k in (-1022, -1, 0, 1, 1023)],
        [np.finfo(np.float64).tiny, np.finfo(np.float64).max]])
    m = np.concatenate([rng.integers(1, 2 ** 26, 62), [2 ** 26 - 1, 1]]).astype(np.float64)
    p4 = [4.0 ** k for k in (-511, -100, -1, 0, 1, 100, 511)]
    # (the two lowest binades: normal arguments whose Newton residuals x - g^2 are SUBNORMAL, a few bits
    # each -- where a refinement step less, or a flushed residual, would show first.  Their own
    # generator: the points were added after the rest of the file had been measured on the device.)
    low = np.finfo(np.float64).tiny * np.random.default_rng(SEED + 1).uniform(1, 4, 64)
    g["sqrt_x"] = np.concatenate([mp_exp_of(rng.uniform(-700, 700, 500)), rng.uniform(1, 4, 400), m * m, p4,
                                  [np.finfo(np.float64).tiny, np.finfo(np.float64).max], low])
    exact = np.zeros(g["sqrt_x"].size, dtype=bool)
    exact[900:900 + 64 + 7] = True
    g["sqrt_exact"] = exact
    # divisions: b = +-exp(U[-600, 600]) | U[1, 2] | 2^k | U[1, 2] on 24 bits with a = q b
    b1 = mp_exp_of(rng.uniform(-600, 600, 400)) * rng.choice([-1.0, 1.0], 400)
    b2 = rng.uniform(1, 2, 300)
    b3 = np.array([2.0 ** int(k) for k in rng.integers(-600, 601, 38)] + [1.0, -2.0])
    b4 = rng.uniform(1, 2, 100).astype(np.float32).astype(np.float64) * rng.choice([-1.0, 1.0], 100)
    q = rng.integers(1, 30, 100).astype(np.float64) * rng.choice([-1.0, 1.0], 100)
    g["div_b"] = np.concatenate([b1, b2, b3, b4])
    g["div_a"] = np.concatenate([rng.uniform(-10, 10, 740), q * b4])
    g["div_pow2"] = np.concatenate([np.zeros(700, bool), np.ones(40, bool), np.zeros(100, bool)])
    g["div_exactq"] = np.concatenate([np.zeros(740, bool), np.ones(100, bool)])
    g["pow13_x"] = np.concatenate([mp_exp_of(rng.uniform(0, 69, 800)), [1.0, 1e30, 1e40]])
    lo15 = float(mp.log(M(3.2e-4)))
    g["pow15_x"] = np.concatenate([np.clip(mp_exp_of(rng.uniform(lo15, 0, 800)), 3.2e-4, 1.0), [1.0, 3.2e-4]])
    g["frozen_d"] = np.concatenate([rng.uniform(-27, 27, 600), rng.uniform(-1, 1, 300),
                                    [0.0, -0.0, 1e-300, -1e-300, 40.0, -40.0, 1e3, -1e3]])
    # the fit's interval, both ends exactly
    uH, uL = rng.uniform(-1, 1, 400), rng.uniform(-1, 1, 400)
    g["chemfit_TcH"] = np.concatenate([6.6 + 8 * uH, [6.6 - 8.0, 6.6 + 8.0, 6.6 - 8.0, 6.6 + 8.0]])
    g["chemfit_TcL"] = np.concatenate([25.9 + 8 * uL, [25.9 - 8.0, 25.9 + 8.0, 25.9 + 8.0, 25.9 - 8.0]])
    # ... and what the formulas see: the interval again, and everything an ocean box can hold
    uH, uL = rng.uniform(-1, 1, 200), rng.uniform(-1, 1, 200)
    g["chemform_TcH"] = np.concatenate([6.6 + 8 * uH, rng.uniform(-2, 45, 300), [6.6 - 8.0, 6.6 + 8.0, -2.0, 45.0]])
    g["chemform_TcL"] = np.concatenate([25.9 + 8 * uL, rng.uniform(-2, 45, 300), [25.9 - 8.0, 25.9 + 8.0, 45.0, -2.0]])
    return g


def frozen_exact(d):
    d = M(float(d))
    return mp.erfc(d) / 2 if d > 0 else 1 - mp.erfc(-d) / 2


def generate():
    with mp.workprec(PREC):
        return _generate()


def _generate():
    g = inputs()
    F = lambda a: [M(float(v)) for v in a]
    g["exp_hi"], g["exp_lo"] = split([mp.exp(x) for x in F(g["exp_x"])])
    g["log_hi"], g["log_lo"] = split([mp.log(x) for x in F(g["log_x"])])
    g["sqrt_hi"], g["sqrt_lo"] = split([mp.sqrt(x) for x in F(g["sqrt_x"])])
    g["recip_hi"], g["recip_lo"] = split([1 / b for b in F(g["div_b"])])
    g["quot_hi"], g["quot_lo"] = split([a / b for a, b in zip(F(g["div_a"]), F(g["div_b"]))])
    third, fifth, cap = M(1) / 3, M(1) / 5, M(1e30)
    g["pow13_hi"], g["pow13_lo"] = split([min(x, cap) ** (-third) for x in F(g["pow13_x"])])
    g["pow15_hi"], g["pow15_lo"] = split([x ** (-fifth) for x in F(g["pow15_x"])])
    g["frozen_hi"], g["frozen_lo"] = split([frozen_exact(d) for d in g["frozen_d"]])
    hi, lo = [], []
    for TcH, TcL in zip(F(g["chemfit_TcH"]), F(g["chemfit_TcL"])):
        h, l = split(chem_decimal(TcH) + chem_decimal(TcL))
        hi.append(h); lo.append(l)
    g["chemfit_hi"], g["chemfit_lo"] = np.array(hi).T.copy(), np.array(lo).T.copy()     # [12][n]
    hi, lo, sa = [], [], []
    for TcH, TcL in zip(F(g["chemform_TcH"]), F(g["chemform_TcL"])):
        (vH, sH), (vL, sL) = chem_doubles(TcH), chem_doubles(TcL)
        h, l = split(vH + vL)
        hi.append(h); lo.append(l); sa.append([float(x) for x in sH + sL])
    g["chemform_hi"], g["chemform_lo"] = np.array(hi).T.copy(), np.array(lo).T.copy()
    g["chemform_sumabs"] = np.array(sa, dtype=np.float32).T.copy()
    return g


def main(path=OUT):
    g = generate()
    np.savez(path, **g)
    print("%s: %d arrays, %d bytes" % (os.path.relpath(path, ROOT), len(g), os.path.getsize(path)))


if __name__ == "__main__":
    main()
