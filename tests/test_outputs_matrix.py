"""Every output and diagnostic against the oracle on every kernel flavour of the host build
(tests/emul): the matrix of tests/outputs_matrix.py with five members per case, every one compared.
The host build has no FMA contraction and no pair kernel; tests/test_gpu_outputs_matrix.py runs
the matrix on the device, where every instantiation is compiled and contracted separately."""
import numpy as np
import pytest

import outputs_matrix as om

N = 5


def _env(monkeypatch, cs):
    monkeypatch.delenv("HECTOR_AMD_EXTENDED_CONS", raising=False)
    for k, v in cs["env"].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("cs", om.HOST_CASES, ids=[c["id"] for c in om.HOST_CASES])
def test_every_output_vs_oracle_and_replayed(emul_lib, monkeypatch, cs):
    _env(monkeypatch, cs)
    c, v, compared, requested, got = om.run_case(emul_lib, cs, N, False, allow_emulation=True)
    if cs["flavour"] == "trk":   # (the tracking core records every row of ALL: nothing to refuse by name)
        assert set(om.ALL) <= set(compared)
    om.replay_case(emul_lib, cs, N, one=c, allow_emulation=True)


def test_oracle_rows_satisfy_the_identities():
    """The tolerances of outputs_matrix.assert_identities are twice what the oracle's own rows
    satisfy them to."""
    worst_up, worst_c = 0.0, 0.0
    for cond in (None, "co2", "ch4"):
        v = om.members(N, cond)
        for B in (1, 4):
            for i in range(N):
                _, r, err = om.reference(cond, v, i, B)
                assert err == 0
                up = np.abs(r["HL_ocean_uptake"] + r["LL_ocean_uptake"] - r["ocean_uptake"]).max() / np.abs(r["ocean_uptake"]).max()
                oc = np.abs(r["HL_ocean_c"] + r["LL_ocean_c"] + r["IO_ocean_c"] + r["DO_ocean_c"] - r["ocean_c"]).max() / r["ocean_c"].max()
                worst_up, worst_c = max(worst_up, up), max(worst_c, oc)
    print("oracle: uptake parts %.3g, ocean_c boxes %.3g" % (worst_up, worst_c))
    assert 2 * worst_up <= om.UPTAKE_SUM_TOL and 2 * worst_c <= om.OCEAN_C_SUM_TOL


def test_zz_report():
    print("\n".join(om.report_lines()))
    assert om.WORST and max(om.WORST.values()) < om.TOL
