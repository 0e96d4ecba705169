"""The hand-written fp64 device math function by function ON THE DEVICE: the gfx950 build of the probe
(tests/devmath/devmath_probe.hip: the product's device headers unchanged, the product's compiler
flags) against the 200-bit references of tests/golden/devmath_reference.npz.

What only exists here, and no host build can stand in for: the v_rcp_f64 / v_rsq_f64 seeds behind
hx_recip, hx_sqrt and the logarithm's division, the v_log_f32 / v_exp_f32 seeds of pow_m13 /
pow_m15, the inline-asm v_fma_f64 chains of hx_frozen_fraction_batch and chem_constants_fit, frexp /
ldexp / rint as the device compiler lowers them, and the constants read as data through
HxConst::mtab / ctab / kfit.  Bounds and their sources: tests/devmath/devmath_checks.py.

The probe owns every allocation it touches and needs no torch.  Every entry point must return 0;
after the first one that does not, the remaining tests fail without launching anything.  The grids
are 7 to 16 wavefronts with a partial last one."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "devmath"))
import devmath_checks as dm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(dm.HIP_PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "devmath"), "libhx_devmath.so"])
    p = dm.Probe(dm.HIP_PROBE)
    assert p.backend == "hip"       # never the emulation
    return p


@pytest.fixture(scope="module")
def G():
    return dm.golden()


@pytest.mark.parametrize("op", dm.OPERATIONS)
def test_error_bound_on_gpu(probe, G, op):
    dm.check_bound(probe, G, op)


@pytest.mark.parametrize("check", dm.CHECKS, ids=lambda f: f.__name__[6:])
def test_property_on_gpu(probe, G, check):
    check(probe, G)


def test_every_entry_point_returned_zero(probe, G):
    """(last in the module: by now every operation has been asked for)"""
    for op in dm.OPERATIONS:
        dm.measure(probe, G, op)
    probe.log1(G, False), probe.log1(G, True)
    assert probe.failed is None and probe.launches == 15
