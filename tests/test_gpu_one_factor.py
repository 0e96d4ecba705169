"""One parameter varied alone, on every kernel flavour, on the device: 128 members (two
wavefronts) against the oracle, plus bitwise independence of a member's neighbours and the
spinup classification of kParams.  (tests/test_one_factor.py: the host-build tier, bit for bit
against the uniform ensemble.)"""
import numpy as np
import pytest

from test_one_factor import (DEFAULTS, EDGES, FLAVOURS, OUTS, PARAMS, TRACK_DATE, assert_flavour,
                             biome_values, capability, cases, check_vs_oracle, make_core, oracle_params)
from test_tracking import FRAC_TOL

pytestmark = pytest.mark.gpu

N = 128
RUN_TO = 2300
GPU_FLAVOURS = ["run", "run2", "pair", "b2", "b4", "b4pair", "b6", "b9", "ext", "trk"]
# probe members: the INI default, a low and a high value (in both wavefronts, never member 0 --
# the one whose values the uniform tables hold while the rows are unsorted), then the edges
PROBES = {"default": (5, 70), "low": (40, 101), "high": (20, 90)}
EDGE_AT = (60, 120)
SHUFFLE = np.random.default_rng(2024).permutation(N)


def gpu_values(name):
    lo, hi = PARAMS[name][:2]
    rng = np.random.default_rng(sum(map(ord, name)))
    v = rng.uniform(lo, hi, N)
    v[1], v[2] = lo, hi   # (the range's ends: neither probe sorts to lane 0)
    plo, phi = lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo)
    for what, x in (("default", DEFAULTS[name]), ("low", plo), ("high", phi)):
        for i in PROBES[what]:
            v[i] = x
    for i, e in zip(EDGE_AT, EDGES.get(name, []) * 2):
        v[i] = e
    v[0] = v.min()   # (a stable sort keeps member 0 in lane 0: the default of lo_warming_ratio, 0,
    return v         # lies below its range)


def probe_members(name):
    ps = [i for t in PROBES.values() for i in t]
    return ps + list(EDGE_AT[:len(EDGES[name]) * 2 if name in EDGES else 0])


def outputs(c, outs):
    return {v: c.fetchvars(v, (1745, RUN_TO)) for v in outs}


_ORACLE_MAPS = {}


def check_maps_vs_oracle(o, c, i, name, value, B, where):
    """Member i's origin maps against the oracle's, at the tolerances of tests/test_tracking.py
    (the companion wavefronts of two biomes: the host build cannot hold them to anything).
    -> the member's (values, fractions) of the tracked span."""
    key = (name, float(value), B)
    if key not in _ORACLE_MAPS:   # (the probes come in pairs of one value)
        ov, of, _, err = o.run_tracking(oracle_params(o, name, value, B), TRACK_DATE, RUN_TO)
        assert err == 0, where
        k0, k1 = TRACK_DATE - o.start, RUN_TO - o.start + 1
        _ORACLE_MAPS[key] = (ov[k0:k1].copy(), of[k0:k1].copy())
    ov, of = _ORACLE_MAPS[key]
    gv, gf = c.tracking_data(i, (TRACK_DATE, RUN_TO))
    assert np.abs(gv - ov).max() < 1e-10 * np.abs(ov).max(), where
    assert np.abs(gf - of).max() < FRAC_TOL, (where, np.abs(gf - of).max())
    assert np.abs(gf.sum(axis=2) - 1.0).max() < 1e-12, where
    return gv, gf


def assert_maps_are(c, i, maps, where):
    gv, gf = c.tracking_data(i, (TRACK_DATE, RUN_TO))
    assert np.array_equal(gv, maps[0]) and np.array_equal(gf, maps[1]), (where, "tracking")


@pytest.mark.parametrize("flavour,name", cases(GPU_FLAVOURS), ids=["-".join(c) for c in cases(GPU_FLAVOURS)])
def test_one_parameter_varied_alone_on_gpu(hip_lib, oracle, monkeypatch, flavour, name):
    fl = FLAVOURS[flavour]
    for k, v in fl.get("env", {}).items():
        monkeypatch.setenv(k, v)
    spinup = PARAMS[name][4]
    vals = gpu_values(name)
    outs = OUTS + fl.get("outs", [])
    c = make_core(hip_lib, fl, name, vals, RUN_TO, device=0)
    assert_flavour(c, fl, name, vals)
    assert (c.status() == 0).all()
    lanes = c.lane_of_member()
    for what in ("default", "low", "high"):
        assert all(lanes[i] != 0 for i in PROBES[what]), (what, lanes[list(PROBES[what])])
    assert {lanes[i] // 64 for i in probe_members(name)} == {0, 1}
    first = outputs(c, outs)
    steps = [c.spinup_steps(i) for i in range(N)]
    ill = []
    for i in (range(N) if fl["B"] == 1 else probe_members(name)):
        check_vs_oracle(oracle, c, i, name, vals[i], fl["B"], RUN_TO, (flavour, name, i), ill)
    maps = {}
    if fl.get("track"):
        maps = {i: check_maps_vs_oracle(oracle, c, i, name, vals[i], fl["B"], (flavour, name, i))
                for i in probe_members(name)}
    # the same members next to other neighbours: a fixed shuffle (a second edit of the same row) ...
    cap = capability(name, fl["B"])
    c.setvar(cap, biome_values(name, vals[SHUFFLE], fl["B"]), PARAMS[name][2])
    c.run(RUN_TO)
    assert_flavour(c, fl, name, vals)
    # ... with a spinup that sees the parameter per member, else the earlier shared one reused
    if spinup:
        assert c.last_spinup_ms() > 0
    else:
        assert c.last_spinup_ms() == 0, (name, c.last_spinup_ms())
    again = outputs(c, outs)
    for v in outs:
        assert np.array_equal(again[v], first[v][:, SHUFFLE]), (flavour, name, "shuffled", v)
    assert [c.spinup_steps(i) for i in range(N)] == [steps[j] for j in SHUFFLE]
    for i in range(N):   # (member i holds what member SHUFFLE[i] held)
        if SHUFFLE[i] in maps:
            assert_maps_are(c, i, maps[SHUFFLE[i]], (flavour, name, "shuffled", i))
    # ... and in member order (no sorting by the parameter)
    c.set_member_sorting(False)
    c.setvar(cap, biome_values(name, vals, fl["B"]), PARAMS[name][2])
    c.run(RUN_TO)
    assert_flavour(c, fl, name, vals)
    assert (c.lane_of_member() == np.arange(N)).all()
    again = outputs(c, outs)
    for v in outs:
        assert np.array_equal(again[v], first[v]), (flavour, name, "unsorted", v)
    for i in maps:
        assert_maps_are(c, i, maps[i], (flavour, name, "unsorted", i))
    c.shutdown()
    if ill:
        print("ill-conditioned members:", ill)
