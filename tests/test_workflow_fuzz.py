"""Randomised workflows on one core -- run in pieces, reset to any date, edit emissions and
parameters in between (R/messages.R:107-140 auto-reset; core.cpp:511-549 reset) -- must end on
exactly what a fresh run with the final inputs gives: the oracle reading the final scenario."""
import os

import numpy as np
import pytest

import hector_amd
from conftest import ROOT, edited_pack


def pack_series(path, section, key):
    with open(path) as f:
        for line in f:
            p = line.split()
            if len(p) > 5 and p[0] == "series" and p[1] == section and p[2] == key:
                return int(p[3]), np.array([float(x) for x in p[5:5 + int(p[4])]])
    raise KeyError(key)


def workflow_fuzz(lib, seed, rounds, tmpdir, n=3, **kw):
    import oracle_binding
    rng = np.random.default_rng(seed)
    names = ["ssp119", "ssp245", "ssp370", "ssp585"]
    worst = 0.0
    for rd in range(rounds):
        name = names[rng.integers(len(names))]
        path = os.path.join(ROOT, "hector_amd", "data", name + ".hxs")
        B = int(rng.choice([1, 2, 4]))
        c = hector_amd.Core(path, n, lib_path=lib, **kw)
        c.enable_history(True)
        if B > 1:
            c.split_biome(["b%d" % b for b in range(B)])
        S = rng.uniform(2.0, 5.0, n); q10 = rng.uniform(1.2, 2.8, (B, n))
        c.setvar("S", S, "degC")
        for b in range(B):
            c.setvar(("b%d." % b if B > 1 else "") + "q10_rh", q10[b])
        outs = ["CO2_concentration", "global_tas", "veg_c", "timesteps"]
        c.set_outputs(outs)
        y0s, ffi = pack_series(path, "simpleNbox", "ffi_emissions")
        _, luc = pack_series(path, "simpleNbox", "luc_emissions")
        log = []
        for op in range(int(rng.integers(3, 7))):
            kind = rng.choice(["run", "reset", "ffi", "luc", "param"])
            if kind == "run":
                y = int(rng.integers(max(c.current_date, 1746), 2301))
                c.run(y); log.append(("run", y))
            elif kind == "reset":
                if c.current_date <= 1746:
                    continue
                y = int(rng.integers(1745, c.current_date + 1))
                c.reset(y); log.append(("reset", y))
            elif kind in ("ffi", "luc"):
                a = int(rng.integers(1760, 2250)); b_ = a + int(rng.integers(1, 50))
                yrs = np.arange(a, b_ + 1)
                ser = ffi if kind == "ffi" else luc
                ser[yrs - y0s] = ser[yrs - y0s] * rng.uniform(0.5, 1.5) + rng.uniform(0, 0.2)
                c.setvar_dated(kind + "_emissions", yrs, ser[yrs - y0s], "Pg C/yr")
                log.append((kind, a, b_))
            else:   # a parameter change invalidates everything (reset to 0 + spinup)
                S = rng.uniform(2.0, 5.0, n)
                c.setvar("S", S, "degC"); log.append(("S",))
        c.run(2300)
        assert (c.status() == 0).all(), log
        allyears = np.arange(y0s, y0s + ffi.size)
        p1 = edited_pack(os.path.join(str(tmpdir), "wf_%d_%d_a.hxs" % (seed, rd)), "simpleNbox",
                         "ffi_emissions", allyears, ffi, base=path)
        p2 = edited_pack(os.path.join(str(tmpdir), "wf_%d_%d_b.hxs" % (seed, rd)), "simpleNbox",
                         "luc_emissions", allyears, luc, base=p1)
        o = oracle_binding.Oracle(p2)
        for i in range(n):
            p = o.default_params()
            if B > 1:
                p = o.split_equal(p, B)
            p.S = S[i]
            for b in range(B):
                p.q10_rh[b] = q10[b][i]
            r, err, _ = o.run(p)
            assert err == 0
            for v in ("CO2_concentration", "global_tas", "veg_c"):
                d = np.abs(c.fetchvars(v, (1745, 2300))[:, i] - r[v]).max() / max(1.0, np.abs(r[v]).max())
                worst = max(worst, d)
                assert d < 2e-8, (name, B, log, i, v, d)
            assert np.array_equal(c.fetchvars("timesteps", (1746, 2300))[:, i], r["timesteps"][1:]), log
    return worst


def test_workflow_fuzz(emul_lib, tmp_path):
    workflow_fuzz(emul_lib, seed=5, rounds=8, tmpdir=tmp_path, allow_emulation=True)


@pytest.mark.gpu
def test_workflow_fuzz_on_gpu(hip_lib, tmp_path):
    print("worst relative deviation:", workflow_fuzz(hip_lib, seed=6, rounds=12, tmpdir=tmp_path, n=70, device=0))


def param_workflow_fuzz(lib, seed, rounds, biomes=(1, 2), n=8, run_to=2300, **kw):
    """Random edits of any parameter row (per member, uniform, back to uniform; the ocean
    diffusivity among them: shared <-> per-member DOECLIM tables), kernel selections switched
    (run / run2 / pair), runs in pieces, resets through the state history -- on one core, which must
    end where a fresh core given the final inputs does: bit for bit when every piece since the
    last invalidation ran the fresh core's kernel, else against the oracle for a few probes.
    (With more than 64 members the lanes are sorted and, after a complete run and a reset to the
    start, re-ordered by measured cost: the partial upload then runs with a changed lane order.)"""
    import oracle_binding
    from test_one_factor import PARAMS, EDGES, DEFAULTS, ORACLE_SCALARS, check_vs_oracle
    from test_random_sweep import check_member
    rng = np.random.default_rng(seed)
    names = list(PARAMS)
    o = oracle_binding.Oracle(os.path.join(ROOT, "hector_amd", "data", "ssp245.hxs"))
    outs = ["CO2_concentration", "global_tas", "timesteps", "veg_c", "ocean_c"]
    stats = {"bitwise": 0, "oracle": 0, "measured order": 0}
    for rd in range(rounds):
        B = int(rng.choice(biomes))
        c = hector_amd.Core(os.path.join(ROOT, "hector_amd", "data", "ssp245.hxs"), n, lib_path=lib, **kw)
        c.enable_history(True)
        if B > 1:
            c.split_biome(["b%d" % b for b in range(B)])
        c.set_outputs(outs)
        sel = {"pair": int(rng.choice([0, 32768])), "w2": int(rng.choice([0, 1]))}
        c.set_pair_kernel_limit(sel["pair"]).set_two_wave_from(sel["w2"])
        vals = {}    # (name, biome or None) -> values[n]
        used, log = set(), []
        for op in range(int(rng.integers(5, 10))):
            kind = rng.choice(["run", "run", "reset", "param", "param", "diff", "select", "complete"])
            if kind == "complete":   # a complete run and a reset to the start: lanes by measured cost
                c.run(run_to); used.add((c.last_run_kernel(), c.last_run_variant()))
                c.reset(1745); log.append(("complete",))
                stats["measured order"] += c.lane_order_source() == "measured cost"
            elif kind == "run":
                y = int(rng.integers(max(c.current_date, 1746), run_to + 1))
                c.run(y); used.add((c.last_run_kernel(), c.last_run_variant())); log.append(("run", y))
            elif kind == "reset":
                if c.current_date <= 1746:
                    continue
                y = int(rng.choice([1745, int(rng.integers(1745, c.current_date + 1))]))
                c.reset(y); log.append(("reset", y))
            elif kind == "select":
                sel = {"pair": int(rng.choice([0, 32768])), "w2": int(rng.choice([0, 1]))}
                c.set_pair_kernel_limit(sel["pair"]).set_two_wave_from(sel["w2"]); log.append(("select", sel))
            else:
                name = "diff" if kind == "diff" else names[rng.integers(len(names))]
                lo, hi, unit, per_biome = PARAMS[name][:4]
                b = int(rng.integers(B)) if per_biome else None
                how = rng.choice(["member", "uniform", "default"])
                v = {"member": lambda: rng.uniform(lo, hi, n), "uniform": lambda: np.full(n, rng.uniform(lo, hi)),
                     "default": lambda: np.full(n, DEFAULTS[name])}[how]()
                if name in EDGES and how == "member":
                    v[rng.integers(n)] = EDGES[name][0]
                if per_biome and name in ("npp_flux0", "veg_c", "detritus_c", "soil_c", "permafrost_c"):
                    v = v / B
                cap = "b%d.%s" % (b, name) if per_biome and B > 1 else name
                c.setvar(cap, v, unit); vals[(name, b if per_biome else None)] = v
                used = set(); log.append((cap, how))   # (a parameter change: reset to 0 + spinup)
        c.run(run_to); used.add((c.last_run_kernel(), c.last_run_variant()))
        f = hector_amd.Core(os.path.join(ROOT, "hector_amd", "data", "ssp245.hxs"), n, lib_path=lib, **kw)
        if B > 1:
            f.split_biome(["b%d" % b for b in range(B)])
        f.set_outputs(outs)
        f.set_pair_kernel_limit(sel["pair"]).set_two_wave_from(sel["w2"])
        for (name, b), v in vals.items():
            f.setvar("b%d.%s" % (b, name) if b is not None and B > 1 else name, v, PARAMS[name][2])
        f.run(run_to)
        fresh = (f.last_run_kernel(), f.last_run_variant())
        if used == {fresh}:
            stats["bitwise"] += 1
            for v in outs:
                assert np.array_equal(c.fetchvars(v, (1745, run_to)), f.fetchvars(v, (1745, run_to))), (rd, B, v, log)
            assert np.array_equal(c.status(), f.status()), (rd, log)
            for i in range(n):
                assert c.spinup_steps(i) == f.spinup_steps(i), (rd, i, log)
        else:
            stats["oracle"] += 1
            ill = []
            for i in sorted({0, n // 2, n - 1}):
                p = o.default_params()
                if B > 1:
                    p = o.split_equal(p, B)
                p.nbiome = B
                for (name, b), v in vals.items():
                    if name in ORACLE_SCALARS: setattr(p, name, v[i])
                    else: getattr(p, name)[b if b is not None else 0] = v[i]
                r, err, steps = o.run(p, run_to)
                assert err == 0 and c.status()[i] == 0, (rd, i, log)
                k = run_to - 1745 + 1
                co2 = c.fetchvars("CO2_concentration", (1745, run_to))[:, i]
                tg = c.fetchvars("global_tas", (1745, run_to))[:, i]
                dev = {"CO2_concentration": np.abs(co2 - r["CO2_concentration"][:k]).max() / r["CO2_concentration"][:k].max(),
                       "global_tas": np.abs(tg - r["global_tas"][:k]).max()}
                check_member(o, p, dev, {"CO2_concentration": 2e-8, "global_tas": 2e-8}, (rd, i, log), ill)
                assert np.array_equal(c.fetchvars("timesteps", (1746, run_to))[:, i], r["timesteps"][1:k]), (rd, i, log)
                assert c.spinup_steps(i) == steps, (rd, i, log)
        c.shutdown(); f.shutdown()
    return stats


def test_param_workflow_fuzz(emul_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_CALIBRATE_ALWAYS", "1")
    print(param_workflow_fuzz(emul_lib, seed=11, rounds=10, biomes=(1, 2), n=8, allow_emulation=True))


def test_param_workflow_fuzz_with_lane_calibration(emul_lib, monkeypatch):
    """72 members: sorted lanes, re-ordered by measured cost after a complete run."""
    monkeypatch.setenv("HECTOR_AMD_CALIBRATE_ALWAYS", "1")
    stats = param_workflow_fuzz(emul_lib, seed=12, rounds=6, biomes=(1, 2), n=72, allow_emulation=True)
    print(stats)
    assert stats["measured order"] > 0


@pytest.mark.gpu
def test_param_workflow_fuzz_on_gpu(hip_lib, monkeypatch):
    monkeypatch.setenv("HECTOR_AMD_CALIBRATE_ALWAYS", "1")
    stats = param_workflow_fuzz(hip_lib, seed=13, rounds=10, biomes=(1, 4), n=128, device=0)
    print(stats)
    assert stats["measured order"] > 0
