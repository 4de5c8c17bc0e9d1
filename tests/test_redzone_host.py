"""tests/redzone.py without a device: the module imports, the zone pattern is a quiet NaN with the documented bits in both
number types, it survives a copy through numpy bit for bit, and a zone is longer than the longest per-batch dof list."""
import numpy as np

import pymfgpu as mf
import redzone


def test_zone_pattern_is_a_quiet_nan_with_its_payload():
    for nt, want, quiet in ((mf.F64, 0x7ff8dead0000beef, 1 << 51), (mf.F32, 0x7fc0beef, 1 << 22)):
        z = redzone.pattern(5, nt)
        assert z.dtype == mf.np_dtype(nt) and np.isnan(z).all()
        assert (redzone.bits(z) == want).all() and want & quiet
        assert (redzone.bits(np.ascontiguousarray(z.copy(), dtype=z.dtype)) == want).all()
        assert np.isnan(z + 1.0).all()  # a zone value that enters arithmetic poisons the result


def test_zone_exceeds_the_longest_batch_dof_list():
    # p_kgu(7) * 64 slots at p = 6 (csrc/mfgpu_internal.h: p_ji(7) + p_hs(7) = 41 rows of 64)
    assert redzone.ZONE == 4096 > 41 * 64 == 2624
