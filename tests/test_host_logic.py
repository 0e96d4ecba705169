"""CPU tests of host-side logic: scenario pack, ensemble generator, sharding,
ABI surface of the HIP library (no compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENARIO, HIP_LIB


def test_abi_library_loads_and_exports_every_declared_symbol(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "hector_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(hx_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) >= 20
    lib = ctypes.CDLL(hip_lib)
    for sym in declared:
        assert hasattr(lib, sym), sym
    lib.hx_backend.restype = ctypes.c_char_p
    assert lib.hx_backend() == b"hip"
    from hector_amd import _lib
    assert sorted(_lib.ABI_SYMBOLS) == declared
    # the toolchain pairing behind a run's figures (no device needed to ask)
    lib.hx_build_info.restype = ctypes.c_char_p
    info = lib.hx_build_info().decode()
    assert re.match(r"built with HIP \d+\.\d+\.\d+ \(.*\), gfx950, product build: .*; runtime -?\d+, driver -?\d+$", info), info


def test_product_fails_loudly_without_gpu(hip_lib):
    """No CPU fallback: creating a core on a box without a HIP device is an error."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import hector_amd
    with pytest.raises(hector_amd.HectorAmdError):
        hector_amd.Core(n_members=4)


def test_loader_refuses_emulation_as_product(emul_lib):
    import hector_amd
    from hector_amd import _lib
    with pytest.raises(hector_amd.HectorAmdError):
        _lib.load(emul_lib)
    assert _lib.load(emul_lib, allow_emulation=True).hx_backend() == b"host-emulation"
    # ... and only from where the tests build it: a copy elsewhere is refused even on request
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        other = shutil.copy(emul_lib, d)
        with pytest.raises(_lib.HectorAmdError):
            _lib.load(other, allow_emulation=True)


def test_ensemble_generator_is_counter_based():
    from hector_amd import ensemble
    S, q = ensemble.ecs_q10(1000)
    S2, q2 = ensemble.ecs_q10(300, offset=500)
    assert np.array_equal(S[500:800], S2) and np.array_equal(q[500:800], q2)
    assert 1.5 <= S.min() and S.max() < 6.0 and 1.0 <= q.min() and q.max() < 3.0
    assert abs(S.mean() - 3.75) < 0.15 and abs(q.mean() - 2.0) < 0.07


def test_shard_ranges_partition_exactly():
    from hector_amd.distributed import shard_range
    for n, w in [(1048576, 8), (65536, 3), (10, 4), (7, 8)]:
        spans = [shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and sum(c for _, c in spans) == n
        for (o0, c0), (o1, _) in zip(spans, spans[1:]):
            assert o0 + c0 == o1


def test_scenario_pack_matches_reference_inputs_when_available(tmp_path, reference_input):
    """The committed pack is regenerated from the reference INI/CSV and must be identical."""
    ini = os.path.join(reference_input, "hector_ssp245.ini")
    import subprocess, sys
    out = tmp_path / "x.hxs"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "import_scenario.py"),
                           ini, str(out)])
    assert open(out).read() == open(SCENARIO).read()


def test_ini_reader_equals_pack(emul_lib, reference_input):
    """The C++ INI/CSV front end (hx_scenario.cpp) on the reference's own INI gives
    the same core as the committed dense pack."""
    ini = os.path.join(reference_input, "hector_ssp245.ini")
    import hector_amd
    a = hector_amd.Core(SCENARIO, 1, lib_path=emul_lib, allow_emulation=True).run(1800)
    b = hector_amd.Core(ini, 1, lib_path=emul_lib, allow_emulation=True).run(1800)
    for v in ("CO2_concentration", "global_tas"):
        assert np.array_equal(a.fetchvars(v), b.fetchvars(v))


def test_example_script_runs(emul_lib, capsys):
    """examples/ensemble_ecs_q10.py end to end (its main() on the emulation build here)."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location(
        "example_ecs_q10", os.path.join(ROOT, "examples", "ensemble_ecs_q10.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tas, tas2 = mod.main(8, lib_path=emul_lib, allow_emulation=True)
    assert (tas2 < tas).all()
    out = capsys.readouterr().out
    assert "2100 warming" in out and "halved fossil emissions" in out


RUNAWAY = {"S": 7.4981, "diff": 0.55557, "aero_scalar": 1.6819, "vol_scalar": 0.33619, "C0": 313.54,
           "tt": 41731000.0, "tu": 47115000.0, "twi": 11610000.0, "tid": 232640000.0,
           "beta": 0.46336, "q10_rh": 3.5869, "warmingfactor": 2.1026, "f_nppv": 0.29871,
           "f_nppd": 0.48862, "f_litterd": 0.93955, "rh_ch4_frac": 0.023349, "pf_mu": 0.88199,
           "pf_sigma": 1.3919, "fpf_static": 0.36564}


def runaway_member_checks(lib, **kw):
    """A member whose carbon cycle runs away (SSP1-1.9 with S = 7.5, Q10 = 3.6, warming factor
    2.1: a negative pool around 2130, CO2 beyond 1e12 ppm a few years later in an implementation
    that carries on) must raise its flag and stop -- not drive the step size to zero and hang the
    launch -- while its neighbours are unaffected."""
    import os
    import hector_amd
    from conftest import ROOT
    path = os.path.join(ROOT, "hector_amd", "data", "ssp119.hxs")
    c = hector_amd.Core(path, 3, lib_path=lib, **kw)
    d = hector_amd.Core(path, 1, lib_path=lib, **kw)
    for k, v in RUNAWAY.items():
        base = c.getvar(k)[0]
        c.setvar(k, [base, v, base])
    c.set_outputs(["CO2_concentration"]); d.set_outputs(["CO2_concentration"])
    # (c's members differ in `diff` -> per-member DOECLIM table, d's lone member uses the shared one:
    # two instantiations of the small-ensemble kernel; the bitwise comparison below is between
    # run kernels, whose history pass sums in the same order either way)
    c.set_pair_kernel_limit(0); d.set_pair_kernel_limit(0)
    c.run(2300); d.run(2300)
    st = c.status()
    assert st[0] == 0 and st[2] == 0 and st[1] & 4          # HX_ERR_NEGPOOL
    co2 = c.fetchvars("CO2_concentration", (1745, 2300))
    assert np.isfinite(co2).all() and co2[:, 1].max() < 5000.0   # frozen at the error, no blow-up
    assert np.array_equal(co2[:, 0], d.fetchvars("CO2_concentration", (1745, 2300))[:, 0])
    assert np.array_equal(co2[:, 2], co2[:, 0])


@pytest.mark.timeout(120)
def test_runaway_member_is_flagged_and_does_not_hang(emul_lib):
    runaway_member_checks(emul_lib, allow_emulation=True)


def test_run_to_an_earlier_date_is_an_error_in_the_r_style_api(emul_lib):
    """rcpp_hector.cpp:168-175 (the C ABI keeps Core::run's silent return, core.cpp:454-458)."""
    import hector_amd
    c = hector_amd.Core(SCENARIO, 1, lib_path=emul_lib, allow_emulation=True)
    c.run(1800)
    with pytest.raises(hector_amd.HectorAmdError, match="prior to the current date of 1800"):
        c.run(1790)
    c.run(1800)                      # the current date itself: nothing to do, no error
    assert c.current_date == 1800
    c.setvar_dated("ffi_emissions", [1780], [0.5], "Pg C/yr")   # pending auto-reset to 1779
    c.run(1790)                      # fine: the core goes back first
    assert c.current_date == 1790


def test_lane_calibration_reorders_lanes_and_keeps_results(emul_lib):
    """Measured-cost lane order (hx_set_lane_calibration) on the host build: adopted at the first
    reset(startDate) after a COMPLETE run, costliest members first, results bit for bit."""
    import hector_amd
    from hector_amd import ensemble
    n = 130
    S, q = ensemble.ecs_q10(n)
    c = hector_amd.Core(n_members=n, lib_path=emul_lib, allow_emulation=True)
    c.setvar("S", S).setvar("q10_rh", q)
    c.set_outputs(["global_tas", "solver_steps", "timesteps"])
    c.run(1900)
    c.reset(1745)
    assert not c.lanes_calibrated()            # a partial run measures nothing
    c.run(2300)
    lane0 = c.lane_of_member().copy()
    tas = c.fetchvars("global_tas").copy()
    cost = 4 * c.fetchvars("solver_steps", (1746, 2300)).sum(0) + 5 * c.fetchvars("timesteps", (1746, 2300)).sum(0)
    c.reset(1745)
    assert c.lanes_calibrated()
    lane1 = c.lane_of_member()
    assert sorted(lane1) == list(range(n)) and not np.array_equal(lane0, lane1)
    assert (np.diff(cost[np.argsort(lane1)]) <= 0).all()
    c.run(2300)
    assert np.array_equal(c.fetchvars("global_tas"), tas)
    off = hector_amd.Core(n_members=n, lib_path=emul_lib, allow_emulation=True)
    off.set_lane_calibration(False).setvar("S", S).setvar("q10_rh", q)
    off.run(2300); off.reset(1745)
    assert not off.lanes_calibrated()
    c.shutdown(); off.shutdown()


def test_cost_model_orders_the_first_run_of_a_later_core(emul_lib, monkeypatch):
    """A core's measured costs make a model (cost ~ quadratic in the varying parameter rows, filed
    under scenario table / biomes / varying rows); a LATER core of the same study orders its lanes
    by the predicted cost from its first run on -- where the order matters, more wavefronts than
    SIMDs (HECTOR_AMD_SIMDS: the logic of a small GPU).  Results do not depend on it, bit for bit."""
    import hector_amd
    from hector_amd import ensemble
    monkeypatch.setenv("HECTOR_AMD_SIMDS", "2")
    kw = dict(lib_path=emul_lib, allow_emulation=True)
    n = 512
    S, q = ensemble.ecs_q10(n)
    a = hector_amd.Core(n_members=n, **kw)
    a.setvar("S", S).setvar("q10_rh", q)
    a.status()
    assert a.lane_order_source() == "parameter key"        # nothing measured anywhere yet
    a.run(2300); a.reset(1745)
    assert a.lane_order_source() == "measured cost" and a.lanes_calibrated()
    # another ensemble of the same study: other members, another size
    m = 768
    S2, q2 = ensemble.ecs_q10(m, offset=5000)
    b = hector_amd.Core(n_members=m, **kw)
    b.setvar("S", S2).setvar("q10_rh", q2)
    b.set_outputs(["global_tas", "CO2_concentration", "solver_steps", "timesteps"])
    b.status()
    assert b.lane_order_source() == "cost model" and not b.lanes_calibrated()
    b.run(2300)
    cost = 4 * b.fetchvars("solver_steps", (1746, 2300)).sum(0) + 5 * b.fetchvars("timesteps", (1746, 2300)).sum(0)
    by_lane = cost[np.argsort(b.lane_of_member())]
    q4 = m // 4
    assert by_lane[:q4].mean() > by_lane[q4:2 * q4].mean() > by_lane[-q4:].mean()    # costliest lanes first
    rank = np.argsort(np.argsort(-by_lane))
    assert np.corrcoef(rank, np.arange(m))[0, 1] > 0.8
    # the same members without the model: other lanes, the same results
    off = hector_amd.Core(n_members=m, **kw)
    off.set_cost_model(False).setvar("S", S2).setvar("q10_rh", q2)
    off.run(2300)
    assert off.lane_order_source() == "parameter key"
    assert not np.array_equal(off.lane_of_member(), b.lane_of_member())
    for v in ("global_tas", "CO2_concentration"):
        assert np.array_equal(off.fetchvars(v), b.fetchvars(v)), v
    # a parameter change keeps the model's order (the measured one is void until the next complete run)
    b.reset(1745)
    assert b.lane_order_source() == "measured cost"
    b.setvar("S", S2[::-1].copy()); b.status()
    assert b.lane_order_source() == "cost model"
    # other varying rows: another key, no model
    d = hector_amd.Core(n_members=m, **kw)
    d.setvar("S", S2).setvar("beta", 0.3 + 0.2 * ensemble.uniform01(np.arange(m, dtype=np.uint64), 7))
    d.status()
    assert d.lane_order_source() == "parameter key"
    for c in (a, b, off, d):
        c.shutdown()


def test_hip_runtime_preload_checks_the_soname(hip_lib, monkeypatch, capsys):
    """PyTorch's bundled HIP runtime is preloaded only if it is the runtime the library
    was linked against (its SONAME among the library's DT_NEEDED), and not at all with
    HECTOR_AMD_NO_TORCH_HIP=1."""
    from hector_amd import _lib
    needed = _lib._elf_dynamic_strings(hip_lib, (1,))[1]
    assert any(n.startswith("libamdhip64.so") for n in needed)
    assert _lib._elf_dynamic_strings(__file__, (1,)) == {}        # not an ELF file
    loaded = []
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path, mode=0: loaded.append(path))
    monkeypatch.setenv("HECTOR_AMD_NO_TORCH_HIP", "1")
    _lib._share_torch_hip_runtime(hip_lib)
    assert loaded == []
    monkeypatch.delenv("HECTOR_AMD_NO_TORCH_HIP")
    monkeypatch.setattr(_lib, "_elf_dynamic_strings",
                        lambda path, tags: {14: ["libamdhip64.so.6"]} if 14 in tags else {1: needed})
    _lib._share_torch_hip_runtime(hip_lib)
    assert loaded == [] and "not preloading" in capsys.readouterr().err


def test_cost_models_persist_across_processes(emul_lib, tmp_path):
    """VERDICT r5 item 2 / ADVICE r5: a genuine one-shot run -- a FRESH process, one core -- orders
    its lanes by a cost model read from a file (hx_cost_models_export / $HECTOR_AMD_COST_MODELS,
    by default the models shipped in hector_amd/data/cost_models.txt), not only by a model some
    earlier core of the same process happened to fit.  And the key now holds the uniform rows'
    values: the same scenario with another beta is another workload, no model."""
    import subprocess
    import sys
    path = str(tmp_path / "models.txt")
    prog = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import hector_amd
from hector_amd import ensemble, core as core_mod
kw = dict(lib_path=%(lib)r, allow_emulation=True)
mode = sys.argv[1]
if mode == "fit":
    S, q = ensemble.ecs_q10(512)
    a = hector_amd.Core(n_members=512, **kw)
    a.setvar("S", S).setvar("q10_rh", q)
    a.status()
    assert a.lane_order_source() == "parameter key", a.lane_order_source()
    a.run(2300); a.reset(1745)
    assert core_mod.cost_models_export(%(path)r, **kw) == 1
    print("fitted")
else:
    S, q = ensemble.ecs_q10(768, offset=9000)
    b = hector_amd.Core(n_members=768, **kw)
    b.setvar("S", S).setvar("q10_rh", q)
    b.status()
    print("first order:", b.lane_order_source())
    d = hector_amd.Core(n_members=768, **kw)
    d.setvar("S", S).setvar("q10_rh", q).setvar("beta", np.full(768, 0.5))
    d.status()
    print("other beta:", d.lane_order_source())
    if mode == "load":       # the explicit call instead of the environment
        assert core_mod.cost_models_load(%(path)r, **kw) == 1
        e = hector_amd.Core(n_members=768, **kw)
        e.setvar("S", S).setvar("q10_rh", q); e.status()
        print("after load:", e.lane_order_source())
''' % {"root": ROOT, "lib": emul_lib, "path": path}
    env = dict(os.environ, HECTOR_AMD_SIMDS="2", HECTOR_AMD_COST_MODELS="")

    def run(mode, **extra):
        r = subprocess.run([sys.executable, "-c", prog, mode], env=dict(env, **extra), capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    assert "fitted" in run("fit")
    text = open(path).read()
    assert text.count("\nmodel ") == 1 and " | rows " in text and " | beta " in text
    out = run("fresh", HECTOR_AMD_COST_MODELS=path)       # a fresh process, its first core
    assert "first order: cost model" in out and "other beta: parameter key" in out
    out = run("load")                                     # no file named: nothing until the explicit load
    assert "first order: parameter key" in out and "after load: cost model" in out
    # a damaged file is ignored, not fatal
    open(path, "w").write("model zzzz 2 1 | rows 0 1 | mean 1 2\n")
    assert "first order: parameter key" in run("fresh", HECTOR_AMD_COST_MODELS=path)
