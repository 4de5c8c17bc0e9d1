"""Host side of mfgpu_vmult_multi (no GPU): the exported symbols, the unchanged description struct, the ctypes
signatures against the header, and the rule that cuts n_vectors into fused groups."""
import ctypes as C
import os
import re

import pytest

import pymfgpu as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mfgpu.h")

# sizeof(mfgpu_desc) as it was before the multi-vector entry points were added
DESC_SIZE = 136

CTYPE = {"mfgpu_handle *": C.c_void_p, "const mfgpu_handle *": C.c_void_p, "void *": C.c_void_p,
         "const void *": C.c_void_p, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
         "const uint32_t *": C.POINTER(C.c_uint32), "uint32_t *": C.POINTER(C.c_uint32)}


def prototype(name):
    """[ctypes of the parameters] of `int name(...)` as the header declares it"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    out = []
    for param in m.group(1).split(","):
        param = " ".join(param.split())
        t = re.match(r"(.*?)(\w+)$", param).group(1).strip()  # drop the parameter's name
        out.append(CTYPE[t if t.endswith("*") else t])
    return out


def test_library_exports_the_entry_points():
    L = mf.lib()
    for name in ("mfgpu_vmult_multi", "mfgpu_multi_width", "mfgpu_plan_multi_groups"):
        assert hasattr(L, name), name


def test_desc_size_is_unchanged():
    assert mf.lib().mfgpu_desc_size() == C.sizeof(mf.Desc) == DESC_SIZE


@pytest.mark.parametrize("name", ["mfgpu_vmult_multi", "mfgpu_multi_width", "mfgpu_plan_multi_groups"])
def test_ctypes_signatures_match_the_header(name):
    assert list(getattr(mf.lib(), name).argtypes) == prototype(name)


def test_flag_constants_match_the_header():
    text = open(HEADER).read()
    for name, value in (("ADD", mf.MULTI_ADD), ("LOOP", mf.MULTI_LOOP), ("FUSED", mf.MULTI_FUSED)):
        m = re.search(r"#define\s+MFGPU_MULTI_" + name + r"\s+\(1u << (\d+)\)", text)
        assert m and value == 1 << int(m.group(1)), name
    assert mf.EUNSUPPORTED == int(re.search(r"#define\s+MFGPU_EUNSUPPORTED\s+\((-\d+)\)", text).group(1))


def test_width_grouping():
    """widest first, a remainder of one vector is a single apply"""
    expected = {1: [1], 2: [2], 3: [3], 4: [3, 1], 5: [3, 2], 6: [3, 3], 7: [3, 3, 1], 8: [3, 3, 2], 9: [3, 3, 3],
                10: [3, 3, 3, 1]}
    for n, groups in expected.items():
        assert mf.multi_groups(n, [3, 2]) == groups, n
    assert mf.multi_groups(5, [2]) == [2, 2, 1]      # a handle whose widest instantiation did not fit
    assert mf.multi_groups(4, []) == [1, 1, 1, 1]    # no fused instantiation: single applies
    assert mf.multi_groups(0, [3, 2]) == []
