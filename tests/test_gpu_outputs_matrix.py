"""Every output and diagnostic against the oracle on every kernel flavour, on the device: the
matrix of tests/outputs_matrix.py with 128 members (two wavefronts; one ragged case of 65), probe
members in both wavefronts and never in lane 0.  With one biome every member meets the oracle
(13 ms of oracle time a member, cached per condition: the flavours share their members), with
several the six probes do.  (tests/test_outputs_matrix.py: the host-build tier.)"""
import numpy as np
import pytest

import outputs_matrix as om

pytestmark = pytest.mark.gpu

N = 128


def _env(monkeypatch, cs):
    monkeypatch.delenv("HECTOR_AMD_EXTENDED_CONS", raising=False)
    for k, v in cs["env"].items():
        monkeypatch.setenv(k, v)


GPU_CASES = om.CASES + om.RAGGED


@pytest.mark.parametrize("cs", GPU_CASES, ids=[c["id"] for c in GPU_CASES])
def test_every_output_vs_oracle_on_gpu(hip_lib, monkeypatch, cs):
    _env(monkeypatch, cs)
    n = cs["n"] or N
    c, v, compared, requested, got = om.run_case(hip_lib, cs, n, True, device=0)
    om.assert_lanes(c, n)
    if n % 64:   # the ragged ensemble's last member, a probe, alone in the second wavefront's first lanes
        assert c.lane_of_member()[n - 1] >= 64
    if cs["flavour"] == "trk":   # (the tracking core records every row of ALL: nothing to refuse by name)
        assert set(om.ALL) <= set(compared)
    # the probes come in pairs of one value: bit for bit the same in whatever lane
    # (under a land-ocean warming ratio by member parity the two of a pair differ in it)
    twins = {}
    for i, kind in om.probes(n).items():
        twins.setdefault((kind,) + tuple(v[k][i] for k in sorted(v)), []).append(i)
    assert cs["cond"] == "lo" or any(len(t) > 1 for t in twins.values())
    for kind, (i, *rest) in twins.items():
        for j in rest:
            for row in compared:
                assert np.array_equal(got[row][:, i], got[row][:, j]), (cs["id"], kind, row)
    c.shutdown()


@pytest.mark.parametrize("cs", om.GPU_REPLAY, ids=[c["id"] for c in om.GPU_REPLAY])
def test_replay_is_bitwise_on_gpu(hip_lib, monkeypatch, cs):
    _env(monkeypatch, cs)
    for c in om.replay_case(hip_lib, cs, N, device=0):
        c.shutdown()


def test_zz_report():
    """The worst deviation per row over the module's cases (profiles/parity_history.md holds a copy)."""
    print("\n".join(om.report_lines()))
    assert om.WORST
    for (cid, row), d in om.WORST.items():
        assert d < om.tol(cid, row, True), (cid, row, d)
