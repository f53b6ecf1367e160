"""CPU-side checks of the weight-gradient accumulation bit of the C ABI (TFNAS_CELL_ACCUM_WGRAD) and of its path-level setter
(tfnas_path_set_wgrad_accum): the plan accepts the bit, still refuses the undefined / retired flag bits, and the setter is
declared, exported and bound.  (The setter's range check on a planned context needs a device: tests/test_gpu_accum.py.)"""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _desc():
    from tfnas_amd import _lib
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride, d.act, d.has_res, d.G = 2, 9, 11, 24, 24, 1, 1, 1, 2
    d.eps = 1e-5
    for g, (m, k, s) in enumerate(((32, 3, 0), (53, 5, 24))):
        d.g[g].mc, d.g[g].k, d.g[g].se = m, k, s
    return d


def test_header_constant_matches_binding():
    from tfnas_amd import _lib
    src = open(HEADER).read()
    m = re.search(r'#define TFNAS_CELL_ACCUM_WGRAD (0x[0-9a-fA-F]+)', src)
    assert m and int(m.group(1), 16) == _lib.CELL_ACCUM_WGRAD == 0x20
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src)


def test_plan_accepts_the_accumulate_bit(lib):
    from tfnas_amd import _lib
    for flags in (_lib.CELL_ACCUM_WGRAD, _lib.CELL_ACCUM_WGRAD | _lib.CELL_LAZY_JOIN):
        d = _desc()
        d.need_wgrad = 1
        d.flags = flags
        assert lib.tfnas_cell_plan(C.byref(d)) == 0
        assert d.flags == flags                       # (the plan keeps the caller's bits)


def test_plan_still_refuses_undefined_and_retired_bits(lib):
    from tfnas_amd import _lib
    for bad in (0x2, 0x4, 0x8, 0x10, 0x40, 0x10 | _lib.CELL_ACCUM_WGRAD):
        d = _desc()
        d.flags = bad
        assert lib.tfnas_cell_plan(C.byref(d)) == -1, hex(bad)      # TFNAS_EINVAL


def test_setter_is_declared_exported_and_bound(lib):
    from tfnas_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert re.search(r'^\s*int\s+tfnas_path_set_wgrad_accum\s*\(\s*void \*ctx,\s*uint32_t cell_mask\s*\);', src, flags=re.M)
    assert hasattr(lib, 'tfnas_path_set_wgrad_accum')
    assert 'tfnas_path_set_wgrad_accum' in _lib.exported_names()
    assert lib.tfnas_path_set_wgrad_accum(None, 0) == -2                 # TFNAS_ENULL
    assert lib.tfnas_path_set_wgrad_accum(None, 1 << 31) == -2
