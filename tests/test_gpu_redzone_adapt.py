"""mfgpu_transfer_interpolate on vectors inside red zones (tests/redzone.py): both vectors are zoned -- they have different
lengths -- and the call runs 16-byte aligned and one element off, in double and in float.  The destination's payload starts
as the NaN pattern, so the dofs the call must zero (coarse Dirichlet dofs, dofs no coarse cell owns) show that it stored
them.  Reference and tolerance are test_gpu_adapt.py's: the sparse J of adapt_reference.py with TRANSFER_TOL."""
import numpy as np
import pytest

import pymfgpu as mf
from redzone import Zoned
from test_gpu_adapt import reference
from test_gpu_gc import pair
from test_gpu_pmg import TRANSFER_TOL, rel, typed

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
ALIGN = pytest.mark.parametrize("offset_one", [False, True], ids=["aligned", "offset"])
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["f64", "f32"])


@ALIGN
@TYPES
@pytest.mark.parametrize("name,p", [("3d_two", 4), ("3d_edge", 1), ("2d_L", 3), ("2d_center", 6)])
def test_interpolate(name, p, nt, offset_one):
    J, stored = reference(name, p, True)
    dim, c, f = pair(name, p, nt)
    t = mf.Transfer.h_hn_interp_from_meshes(c, f)
    x = typed(np.random.default_rng(f.n_dofs + p).standard_normal(f.n_dofs), nt)
    src, dst = Zoned(x, nt, offset_one), Zoned(c.n_dofs, nt, offset_one)
    t.interpolate(dst.vec, src.vec)
    got = dst.result()
    src.unchanged()
    err = rel(got, J @ x)
    print(f"{name} p = {p}: interpolate between zones {err:.2e}")
    assert err <= TRANSFER_TOL[nt]
    assert (~stored).any() and not got[~stored].any()
