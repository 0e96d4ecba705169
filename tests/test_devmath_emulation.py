"""The hand-written fp64 device math (hx_dev_math.h, hx_dev_chem.h, hx_dev_solver.h) function by
function, in the HOST build of the probe (tests/devmath/devmath_probe.hip through tests/emul/shim),
against the 200-bit references of tests/golden/devmath_reference.npz.

The bounds and their sources stand in tests/devmath/devmath_checks.py; the same checks run on the
device in tests/test_gpu_devmath.py.  The host build's v_rcp_f64 / v_rsq_f64 stand-ins are exact
(1.0 / x, 1.0 / sqrt(x)), so what this module says about hx_sqrt, hx_recip and hx_div_cr holds for
the refinement's arithmetic only: the seeds are the GPU module's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "devmath"))
import devmath_checks as dm  # noqa: E402


@pytest.fixture(scope="module")
def probe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "devmath"), "libhx_devmath_emul.so"])
    p = dm.Probe(dm.EMUL_PROBE)
    assert p.backend == "host-emulation"
    return p


@pytest.fixture(scope="module")
def G():
    return dm.golden()


@pytest.mark.parametrize("op", dm.OPERATIONS)
def test_error_bound(probe, G, op):
    dm.check_bound(probe, G, op)


@pytest.mark.parametrize("check", dm.CHECKS, ids=lambda f: f.__name__[6:])
def test_property(probe, G, check):
    check(probe, G)


def test_fixture_shapes(G):
    """Every grid is a few wavefronts with a partial last one; ref_lo is a fraction of an ulp."""
    for k in ("exp_x", "log_x", "sqrt_x", "div_b", "pow13_x", "pow15_x", "frozen_d", "chemfit_TcH", "chemform_TcH"):
        assert 128 < G[k].size <= 1100 and G[k].size % 64 != 0, k
    for k in G:
        if k.endswith("_lo"):
            assert G[k].dtype == np.float32 and (np.abs(G[k]) <= 0.5).all(), k
    assert os.path.getsize(dm.GOLDEN) < 628474      # tests/golden/stash_control_parent.npz, the largest so far


def test_exp_and_log_constants_in_the_source():
    """A wrong low digit in a coefficient of exp or log moves a result by 1e-20 or less: no error bound
    can see it.  So the constants themselves, read from the source text: the table hx_fill_math_table
    fills is the literals of hx_dev_math.h, double for double; 1/k! to an ulp (the exact rational
    rounded once: <= 1/2 ulp, and 1/9!, 1/10! stand one ulp off that); log2 e and sqrt(1/2) correctly
    rounded; LN2_HI with 21 trailing zero bits (k LN2_HI exact for |k| < 2^21) and LN2_LO the rounded
    rest of ln 2; Lg1..Lg7 the words of fdlibm's e_log.c."""
    import math
    import re
    import struct
    from decimal import Decimal
    from fractions import Fraction
    num = r"(-?[\d.]+(?:e[+-]?\d+)?)"
    src = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_dev_math.h")).read()
    lay = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_layout.h")).read()
    floats = lambda body: [float(x) for x in body.replace("\n", " ").split(",") if x.strip()]
    table = floats(re.search(r"const double v\[26\] = \{([^}]*)\}", lay).group(1))
    c = floats(re.search(r"constexpr double c\[12\] = \{([^}]*)\}", src).group(1))
    log2e, ln2hi, ln2lo = (float(x) for x in re.search(
        r"LOG2E = %s, LN2_HI = %s,\s*LN2_LO = %s;" % (num, num, num), src).groups())
    lit = {int(i): float(v) for i, v in re.findall(r"T\[(\d+)\] : %s" % num, src)}
    assert len(table) == 26 and len(c) == 12 and sorted(lit) == list(range(16, 26))
    word = lambda v: struct.unpack("<Q", struct.pack("<d", v))[0]
    want = c + [log2e, -ln2hi, -ln2lo, 0.0] + [lit[i] for i in range(16, 26)]
    assert [word(v) for v in table] == [word(v) for v in want]
    assert (lit[23], lit[24]) == (ln2hi, ln2lo)
    for k, v in zip(range(13, 1, -1), c):
        exact = Fraction(1, math.factorial(k))
        assert abs(Fraction(v) - exact) <= Fraction(math.ulp(v)), k
    ln2 = Fraction(Decimal("0.6931471805599453094172321214581765680755001343602552541206800094933936"))
    assert word(ln2hi) & ((1 << 21) - 1) == 0 and abs(Fraction(ln2hi) - ln2) < Fraction(1, 2 ** 31)
    assert ln2lo == float(ln2 - Fraction(ln2hi))
    assert log2e == float(Fraction(Decimal("1.4426950408889634073599246810018921374266459541529859341354494069")))
    assert lit[25] == float(Fraction(Decimal("0.70710678118654752440084436210484903928483593768847403658833987")))
    assert [word(lit[i]) for i in range(16, 23)] == [
        0x3FE5555555555593, 0x3FD999999997FA04, 0x3FD2492494229359, 0x3FCC71C51D8E78AF,
        0x3FC7466496CB03DE, 0x3FC39A09D078C69F, 0x3FC2F112DF3E5244]


def test_committed_fixture_is_what_the_generator_produces():
    """... and, with the same tool at hand, hx_chem_fit.inc is what tools/make_chem_fit.py fits: a
    changed digit in a mid-degree coefficient moves a constant by 1e-21, far below any error bound."""
    import importlib.util
    mp = pytest.importorskip("mpmath")

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    new, old = load("make_devmath_golden").generate(), dm.golden()
    assert sorted(new) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
    dps = mp.mp.dps
    try:
        fit = load("make_chem_fit")          # (sets its own 60 digits)
        txt = open(os.path.join(ROOT, "hector_amd", "csrc", "hx_chem_fit.inc")).read()
        body = txt[txt.index("{", txt.index("hx_chem_fit_table")) + 1:txt.rindex("}")]
        tab = np.array([float.fromhex(x.strip()) for x in body.replace("\n", " ").split(",") if x.strip()])
        tab = tab.reshape(fit.DEGREE + 1, 12)
        for b, (_, centre) in enumerate(fit.BOXES):
            for f, name in enumerate(fit.NAMES):
                mono = [float(x) for x in fit.fit(lambda T: fit.constants(T)[name], centre)]
                assert mono[::-1] == tab[:, b * 6 + f].tolist(), (b, name)
    finally:
        mp.mp.dps = dps
