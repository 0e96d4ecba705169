"""Carbon-tracking origin maps of EVERY member on the device, on every lane and at the zero-pool
edges, against the oracle.

One- and two-biome ensembles keep their maps on companion wavefronts (track_companion with
track_post_stash, hx_run_kernel<B, ., ., 3>): arithmetic of their own (tvr_add_to_empty,
tvr_add_names, a column slice per wavefront, one reciprocal) and a protocol of their own (two sets
of LDS slots, one barrier per stash of the wavefront, TRKR_ACTIVE naming the lanes at a segment
end).  The host build never runs them, so nothing but the device can hold them to the oracle.
HECTOR_AMD_TRACK_INLINE (read at every launch) sends the same ensembles through the inline maps
(track_stash), which three and more biomes always take.

The ensemble (test_tracking.edge_ensemble): 70 members -- a full wavefront and six lanes -- in
sorted lane order, S, Q10 and beta spread so that the lanes of a wavefront take different numbers
of stashes in a third and more of the tracked years, members with permafrost_c = 0 (equal shares
of a zero total, chosen wave-wide and selected per lane), fpf_static = 1 and 0, beta = 0 and
f_litterd = 1 between them; ssp245 from 1950 and ssp534-over from 2000 (direct air capture: the
earth_c map is not 100 % earth).  The default lane order sorts by the standardised parameters, and
a zero among 865s lies 4.7 standard deviations low: the three permafrost_c = 0 members sit in the
low lanes of the full wavefront next to ordinary members; the six-lane wavefront holds the
fpf_static = 1 and f_litterd = 1 members.

Every case also runs a second core in pieces and, with the history on, from a reset into the
tracked span: each member's values, fractions and names bit for bit the straight run's (the
companions resume from the record: slot0, columns read past the last source).

Worst deviations from the oracle over the 70 members, measured on an MI355X (pool values relative
to the largest pool; fractions absolute; the tolerances are test_tracking's 1e-10 and 1e-8 -- the
host build's inline maps give <= 7e-15 and <= 1.8e-12 on these inputs):

    case                 scenario      pools      fractions
    companions-1         ssp245        7.4e-15    2.0e-12
    companions-1         ssp534-over   1.1e-14    1.8e-13
    companions-1-diff    ssp245        8.5e-15    3.6e-12
    companions-2         ssp245        6.9e-15    3.0e-12
    companions-2         ssp534-over   7.8e-15    2.2e-13
    companions-2-diff    ssp245        7.4e-15    3.3e-12
    inline-1             ssp534-over   1.1e-14    1.8e-13
    inline-2             ssp534-over   7.8e-15    2.2e-13
    inline-4             ssp245        7.8e-15    2.9e-12
    looped-6             ssp245        6.8e-15    4.1e-13
"""
import numpy as np
import pytest

from test_tracking import (EDGE_N, EDGE_PF0, EDGE_SPANS, check_maps_every_member, edge_core,
                           edge_ensemble, edge_min_counts, edge_params, scenario_oracle)

pytestmark = pytest.mark.gpu

# case: biomes, maps, per-member diffusivity, scenarios
CASES = {
    "companions-1": (1, "companions", False, ("ssp245", "ssp534-over")),
    "companions-1-diff": (1, "companions", True, ("ssp245",)),
    # three companion wavefronts of 6 columns for 16 pools: the last one's columns pass the last pool
    "companions-2": (2, "companions", False, ("ssp245", "ssp534-over")),
    "companions-2-diff": (2, "companions", True, ("ssp245",)),
    "inline-1": (1, "inline", False, ("ssp534-over",)),
    "inline-2": (2, "inline", False, ("ssp534-over",)),
    "inline-4": (4, "inline", False, ("ssp245",)),            # unrolled, 4-column chunks
    "looped-6": (6, "inline", False, ("ssp245",)),            # looped: 8-column chunks, two mask words
}
PARAMS = [(case, sc) for case, v in CASES.items() for sc in v[3]]
# The spread of Q10 and beta reaches the last biome only: with 4 and 6 biomes the oracle's lanes
# part in 47 and 44 of the 151 years, not in a third of them (1 and 2 biomes: 51 to 88).
MIN_DIVERGENT = {4: 0.25, 6: 0.25}


def every_members_maps(c, T0, END):
    return [c.tracking_data(i, (T0, END), masks=True) for i in range(c.n_members)]


@pytest.mark.parametrize("case,scenario", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_every_members_maps_vs_oracle_on_gpu(hip_lib, monkeypatch, case, scenario):
    nb, maps, diff, _ = CASES[case]
    if maps == "inline":
        monkeypatch.setenv("HECTOR_AMD_TRACK_INLINE", "1")
    else:
        monkeypatch.delenv("HECTOR_AMD_TRACK_INLINE", raising=False)
    path, o = scenario_oracle(scenario)
    T0, END = EDGE_SPANS[scenario]
    ens = edge_ensemble(diff)
    c = edge_core(hip_lib, path, ens, nb, T0, device=0)
    c.run(END)
    assert c.backend == "hip"
    assert c.last_run_kernel() == "run" and c.last_run_variant() == 2
    lanes = c.lane_of_member()
    assert not (lanes == np.arange(EDGE_N)).all()
    # equal-shares lanes among ordinary ones in the full wavefront; the partial one is peopled
    assert all(lanes[i] < 64 for i in EDGE_PF0) and (lanes >= 64).sum() == EDGE_N - 64
    worst = check_maps_every_member(c, o, lambda i: edge_params(o, ens, i, nb), T0, END,
                                    daccs=scenario == "ssp534-over",
                                    min_divergent=MIN_DIVERGENT.get(nb, 1.0 / 3.0),
                                    min_counts=edge_min_counts(scenario, T0))
    print("%s %s: worst pool deviation %.2e, worst fraction deviation %.2e" % ((case, scenario) + worst))
    straight = every_members_maps(c, T0, END)
    c.shutdown()
    # in pieces (a launch that ends before, at and just after the tracking date; resumed launches
    # start from the record), then from a reset into the tracked span
    d = edge_core(hip_lib, path, ens, nb, T0, device=0)
    d.enable_history(True)
    for to in (T0 - 7, T0, T0 + 1, T0 + 33, END):
        d.run(to)
    assert d.last_run_kernel() == "run" and d.last_run_variant() == 2
    assert (d.lane_of_member() == lanes).all()
    for what in ("pieces", "reset"):
        if what == "reset":
            d.reset(T0 + 20)
            d.run(END)
        for i, (a, b) in enumerate(zip(every_members_maps(d, T0, END), straight)):
            for x, y, name in zip(a, b, ("values", "fractions", "names")):
                assert np.array_equal(x, y), (what, i, name)
    d.shutdown()
