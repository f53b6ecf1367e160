#!/usr/bin/env python3
"""Golden vectors of MBConv blocks WITHOUT an expand convolution (mid_channels <= in_channels), recorded by running the REFERENCE
itself (imported from $TFNAS_REFERENCE, tests/_refload.py) on the CPU -- the companion of make_golden_k7.py for
tests/test_noexp_oracle_pin.py.

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_noexp.py
Output (committed):     tests/golden/oracle_noexp_pin.npz
The fixture is data only (the reference's outputs).  While recording, the oracle's blocks are compared with the reference's on the
spot (the same comparison tests/test_noexp_oracle_pin.py replays from the recorded side)."""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _noexp  # noqa: E402
import _refload  # noqa: E402

ref = _refload.import_reference()


def reference_block(form, case, oracle_blk):
    """The reference's MBInvertedResBlock of one pin case (built with the case's OWN mid_channels: 16 or 8) with the oracle
    block's weights."""
    mid, s, act, se = case
    q = _noexp.PIN_GEOM
    blk = ref.layers.MBInvertedResBlock(q['ic'], mid, se, q['oc'], _noexp.pin_k(case), s, affine=(form == 'derived'),
                                        act_func=act)
    assert blk.inverted_bottleneck is None and blk.mid_channels == q['ic']
    blk.load_state_dict(oracle_blk.state_dict())
    blk.drop_connect_rate = getattr(oracle_blk, 'drop_connect_rate', 0.0)
    return blk.double().train()


def pin_fixture():
    out = OrderedDict()
    for form in _noexp.PIN_FORMS:
        for case in _noexp.PIN_CASES:
            o, x, r, seed = _noexp.pin_oracle_block(form, case)
            want = _noexp.pin_run(reference_block(form, case, o), x, r, seed)
            got = _noexp.pin_run(o, x, r, seed)
            assert list(got) == list(want), (list(got), list(want))
            for k in want:
                assert np.allclose(got[k], want[k], atol=2e-6, rtol=1e-4), (form, case, k)
            for k, v in _noexp.pin_record(want).items():
                out[_noexp.pin_tag(form, case) + '/' + k] = v
            print('pin', _noexp.pin_tag(form, case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'oracle_noexp_pin.npz'), **out)


if __name__ == '__main__':
    pin_fixture()
