"""The three families of mixes in ONE core, leaving one family at a time.

A mix of a carbon / CH4 series is expanded into the variable's table (hx_mseries_mix_kernel), a mix
of N2O_emissions, RF_albedo or a halocarbon's emissions is evaluated by the gas pre-pass
(hx_gas_mix_kernel), a mix of an aerosol or ozone / OH precursor emission by hx_slcf_mix_kernel.  Each
family is held to the oracle on its own in test_member_mix / test_member_gas_mix /
test_member_slcf_mix; here all three live in one core and are removed family by family, in three
orders in which every family leaves first, second and last at least once.  After every removal the
core has to give, bit for bit and with the same kernel, what a fresh core gives that was only ever
handed the mixes still present -- in the end one that never had a mix.

S is unsorted (test_member_series.member_S): the lane order is a real permutation of the member
order.  This file: the helpers and the host-build tier (tests/emul, 70 members).
tests/test_gpu_member_mix_families.py: the same on the device, 130 members."""
import numpy as np
import pytest

import hector_amd
import test_member_gas_mix as gm
import test_member_mix as tm
import test_member_series as ts
import test_member_slcf_mix as sm
from test_member_mix import assert_equal_results
from test_member_series import FLAVOURS

N_HOST = 70
HOST = dict(allow_emulation=True)
Error = hector_amd.HectorAmdError
TO = 2100
FAMILY = {
    "table": ["ffi_emissions", "CH4_emissions"],                          # lag 1, lag 0
    "gas": ["N2O_emissions", "RF_albedo", gm.WITH_EMISSIONS + "_emissions"],
    "slcf": ["SO2_emissions", "NOX_emissions"],                           # aerosol group, precursor group
}
ALL_NAMES = [name for names in FAMILY.values() for name in names]
UNIT = dict(ts.UNIT, **gm.UNIT, **sm.UNIT)
ORDERS = [("table", "gas", "slcf"), ("slcf", "gas", "table"), ("gas", "slcf", "table")]


def family_mixes(n):
    """family -> [(name, years, basis[3, year], coeff[3, member])], 2030-2100: the modules' own
    standard mixes of the names above."""
    pool = tm.standard_mixes(n) + gm.standard_mixes(n) + sm.standard_mixes(n)
    by_name = {m[0]: m for m in pool}
    return {f: [by_name[name] for name in names] for f, names in FAMILY.items()}


def set_mixes(c, mixes):
    for name, years, basis, coeff in mixes:
        assert basis.shape[0] == 3 and years[0] == 2030 and years[-1] == TO
        assert c.setvar_dated_mix(name, years, basis, coeff, UNIT[name]) is c


def finished(c):
    """-> (everything the core answers, the kernel it ran)"""
    c.run(TO)
    return sm.result(c, run_to=TO, inputs=ALL_NAMES), (c.last_run_kernel(), c.last_run_variant())


_FRESH = {}


def fresh(lib, n, kw, families):
    """A core that was only ever given the mixes of `families`; once per (lib, n, families)."""
    key = (lib, n, frozenset(families))
    if key not in _FRESH:
        mixes = family_mixes(n)
        c = sm.slcf_core(lib, FLAVOURS["run"], n, kw)
        for f in FAMILY:
            if f in families:
                set_mixes(c, mixes[f])
        _FRESH[key] = finished(c)
        assert (_FRESH[key][0]["status"] == 0).all()
        c.shutdown()
    return _FRESH[key]


def check_families_leave(lib, n, kw, order):
    mixes = family_mixes(n)
    c = sm.slcf_core(lib, FLAVOURS["run"], n, kw)
    for f in FAMILY:
        set_mixes(c, mixes[f])
    present = list(FAMILY)
    for leaving in order + (None,):
        got, kernel = finished(c)
        want, want_kernel = fresh(lib, n, kw, present)
        where = "%s: %s left" % ("-".join(order), "+".join(present) or "nothing")
        assert kernel == want_kernel, (where, kernel, want_kernel)
        assert (got["status"] == 0).all(), where
        assert_equal_results(got, want, where)
        if leaving is not None:
            for name in FAMILY[leaving]:
                assert c.clear_mix(name) is c
            present.remove(leaving)
    assert present == []
    c.shutdown()


def check_shared_edit_refused(lib, n, kw):
    """setvar_dated in a covered year, for a name of every family: refused by name, nothing changed."""
    mixes = family_mixes(n)
    c = sm.slcf_core(lib, FLAVOURS["run"], n, kw)
    for f in FAMILY:
        set_mixes(c, mixes[f])
    before, _ = finished(c)
    for name in ALL_NAMES:
        with pytest.raises(Error) as e:
            c.setvar_dated(name, [2050], [1.0], UNIT[name])
        assert "hx_setvar_dated: %s has a mix that covers 2050: remove the mix first" % name in str(e.value)
    after, _ = finished(c)
    assert_equal_results(after, before, "after the seven refusals")
    assert_equal_results(before, fresh(lib, n, kw, list(FAMILY))[0], "all seven mixes")
    c.shutdown()


# ---------------------------------------------------------------------------------------------
# the host-build tier

@pytest.mark.parametrize("order", ORDERS, ids="-".join)
def test_families_leave_one_at_a_time(emul_lib, order):
    check_families_leave(emul_lib, N_HOST, HOST, order)


def test_shared_edit_in_a_covered_year_is_refused_for_every_family(emul_lib):
    check_shared_edit_refused(emul_lib, N_HOST, HOST)
