"""CPU-side checks of the retrain tail's C ABI (include/tfnas_hip.h: tfnas_cls_ce_ex, tfnas_cls_reduce): both are declared, exported
and bound with matching arities, the ABI version stays 4, and the documented argument checks answer before any launch (no GPU)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'tfnas_hip.h')
EINVAL, ENULL, ERANGE = -1, -2, -3
NAMES = ('tfnas_cls_ce_ex', 'tfnas_cls_reduce')


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def _declarations():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r'^\s*int\s+(tfnas_\w+)\s*\(([^;]*)\)\s*;', src, flags=re.M | re.S)}


def test_symbols_are_declared_exported_and_bound_with_matching_arity(lib):
    from tfnas_amd import _lib
    decl = _declarations()
    for name in NAMES:
        assert name in decl, '%s is not declared in include/tfnas_hip.h' % name
        assert hasattr(lib, name), '%s is not exported' % name
        assert name in _lib.exported_names()
        nargs = len([a for a in decl[name].split(',') if a.strip()])
        res, args = _lib._PROTOS[name]
        assert res is C.c_int and len(args) == nargs, (name, len(args), nargs)
    assert len(_lib._PROTOS['tfnas_cls_ce_ex'][1]) == 15 and len(_lib._PROTOS['tfnas_cls_reduce'][1]) == 14
    # the float / int arguments sit where the header has them
    assert [i for i, a in enumerate(_lib._PROTOS['tfnas_cls_ce_ex'][1]) if a is C.c_float] == [7, 8]
    assert [i for i, a in enumerate(_lib._PROTOS['tfnas_cls_reduce'][1]) if a is C.c_int] == [0, 1, 2, 8]


def test_abi_version_stays_4_and_the_header_documents_the_rules(lib):
    assert lib.tfnas_abi_version() == 4
    src = open(HEADER).read()
    assert re.search(r'#define TFNAS_ABI_VERSION 4\b', src)
    assert 'tfnas_cls_ce_fwd_bwd' not in src and 'HipModes.from_env' not in src        # (names that never existed)
    doc = src[src.index('tfnas_cls_ce_ex ='):src.index('int tfnas_cls_ce_ex(')]
    for word in ('TIE RULE', 'NaN', 'rank[n] = -1', 'forward-only', 'bit-identical', 'meter[5]', 'gscale'):
        assert word in doc, word


def test_per_image_launch_argument_checks(lib):
    # never dereferenced: every call below is refused before a launch (a call that passed the checks WOULD launch where a GPU is
    # present, so none is made with these pointers)
    p = C.c_void_p(64)

    def call(N=4, Cf=8, K=3, pooled=p, W=p, target=p, eps=0.1, logits=p, loss_n=p, rank=p, dlogits=p, dpooled=p):
        return lib.tfnas_cls_ce_ex(N, Cf, K, pooled, W, None, target, 1.0, eps, logits, loss_n, rank, dlogits, dpooled, None)
    for missing in ('pooled', 'W', 'target', 'logits', 'loss_n', 'rank'):
        assert call(**{missing: None}) == ENULL, missing
    assert call(Cf=6) == EINVAL and call(Cf=1282) == EINVAL                # C % 4
    assert call(K=4097) == ERANGE and call(K=0) == ERANGE
    assert call(Cf=4100) == ERANGE and call(Cf=0) == ERANGE and call(N=0) == ERANGE
    assert call(dpooled=None) == EINVAL                                    # d logits without d pooled
    assert call(dlogits=None) == EINVAL
    for eps in (-0.1, 1.0, float('nan')):
        assert call(eps=eps) == EINVAL, eps


def test_reduction_launch_argument_checks(lib):
    p = C.c_void_p(64)

    def call(N=4, Cf=8, K=3, pooled=p, dlogits=p, loss_n=p, rank=p, gscale=None, acc=0, dW=p, db=p, out=p, meter=None):
        return lib.tfnas_cls_reduce(N, Cf, K, pooled, dlogits, loss_n, rank, gscale, acc, dW, db, out, meter, None)
    for missing in ('loss_n', 'rank', 'pooled', 'dlogits', 'dW', 'db'):
        assert call(**{missing: None}) == ENULL, missing
    assert call(dW=None, db=None, out=None, meter=None) == ENULL           # nothing to write
    assert call(K=4097) == ERANGE and call(Cf=4097) == ERANGE and call(N=0) == ERANGE
    assert call(pooled=None, dlogits=None, dW=None, db=None, K=5000) == ERANGE
    assert call(acc=2) == EINVAL and call(acc=-1) == EINVAL


def test_python_side_shape_limits_mirror_the_library():
    from tfnas_amd import tail
    assert tail.cls_shapes_ok(1280, 1000) and tail.cls_shapes_ok(64, 7) and tail.cls_shapes_ok(4096, 4096)
    assert not tail.cls_shapes_ok(1282, 10) and not tail.cls_shapes_ok(4100, 10) and not tail.cls_shapes_ok(1280, 4097)
