"""hx_ensemble_comoments on the GPU, beside tests/test_gpu_comoments.py: windows far outside the
scenario through the C ABI itself (they must be refused by name before the library sizes anything
from them), and examples/emergent_constraint.py end to end on a small ensemble -- its main() goes
through derive, score, comoments (cross and symmetric, with and without weights) and CoMoments.pca,
so a drift in any of those signatures fails here."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import hector_amd
from hector_amd import ensemble
from conftest import ROOT, SCENARIO

pytestmark = pytest.mark.gpu


def test_absurd_windows_are_refused_by_name_through_the_c_abi(hip_lib):
    n = 64
    c = hector_amd.Core(SCENARIO, n, lib_path=hip_lib)
    S, q10 = ensemble.ecs_q10(n)
    c.setvar("S", S, "degC").setvar("q10_rh", q10)
    c.run(1760)
    good = c.comoments("global_tas", (1750, 1760))
    dp = ctypes.POINTER(ctypes.c_double)
    buf = np.full(64, 7.0)          # (far too small for the windows below: a refused call writes nothing)
    p = buf.ctypes.data_as(dp)
    imax, imin = 2 ** 31 - 1, -2 ** 31
    for a, b in (((0, 10 ** 9), None), ((imin, imax), None), ((1745, imax), None), ((imin, 1760), None),
                 ((1750, 1760), (0, 10 ** 9)), ((1750, 1760), (imin, imax)), ((imin, imax), (imin, imax))):
        vb, b0, b1 = (None, 0, 0) if b is None else (b"global_tas", b[0], b[1])
        rc = c._lib.hx_ensemble_comoments(c._h, b"global_tas", a[0], a[1], vb, b0, b1, None, p, p, p, p, p, None, None)
        assert rc != 0
        msg = c._lib.hx_last_error().decode()
        assert msg.startswith("hx_ensemble_comoments: dates must lie between"), msg
        assert (buf == 7.0).all()
    again = c.comoments("global_tas", (1750, 1760))
    assert np.array_equal(good.cross, again.cross) and good.wsum == again.wsum and good.n_part == again.n_part
    c.shutdown()


def test_the_emergent_constraint_example_runs(hip_lib, capsys):
    spec = importlib.util.spec_from_file_location(
        "example_emergent_constraint", os.path.join(ROOT, "examples", "emergent_constraint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 192
    prior, post = mod.main(n, lib_path=hip_lib)
    out = capsys.readouterr().out
    assert "score-weighted corr" in out and out.count("EOFs of global_tas 1850-2100: variance shares") == 2
    for cm in (prior, post):
        assert cm.cross.shape == (41, 1) and not cm.symmetric
        assert np.array_equal(cm.years_a, np.arange(1980, 2021)) and np.array_equal(cm.years_b, [2100])
        assert np.isfinite(cm.corr).all() and (np.abs(cm.corr) <= 1.0 + 1e-12).all()
    assert 0 < post.n_part < prior.n_part <= n      # (the held-out member carries no weight)
