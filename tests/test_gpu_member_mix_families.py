"""The three families of mixes in one core, leaving one family at a time, on the device: 130 members
(npad 192: three wavefronts, two real lanes in the last), unsorted S.  (tests/
test_member_mix_families.py: the helpers, the inputs and the host-build tier.)"""
import pytest

import test_member_mix_families as mf

pytestmark = pytest.mark.gpu

N = 130
GPU = dict(device=0)   # (no allow_emulation: make_core() asserts core.backend == "hip")


@pytest.mark.parametrize("order", mf.ORDERS, ids="-".join)
def test_families_leave_one_at_a_time_on_gpu(hip_lib, order):
    mf.check_families_leave(hip_lib, N, GPU, order)


def test_shared_edit_in_a_covered_year_is_refused_for_every_family_on_gpu(hip_lib):
    mf.check_shared_edit_refused(hip_lib, N, GPU)
