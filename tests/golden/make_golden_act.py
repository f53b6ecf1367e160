#!/usr/bin/env python3
"""Golden vectors of the ReLU6 / hard-swish blocks, recorded by running the REFERENCE itself (imported from $TFNAS_REFERENCE,
tests/_refload.py) on the CPU -- the companion of make_golden_k7.py for tests/test_act_oracle_pin.py.

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_act.py
Output (committed):     tests/golden/oracle_act_pin.npz
The fixture is data only (_golden.probe of the reference's outputs and gradients, the depthwise weight gradient whole).  While
recording, the wrapped oracle's blocks (tests/_acts.py) are compared with the reference's on the spot -- the same comparison
tests/test_act_oracle_pin.py replays from the recorded side."""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _acts  # noqa: E402
import _k7  # noqa: E402
import _refload  # noqa: E402

ref = _refload.import_reference()


def reference_block(form, case, oracle_blk):
    """The reference's MBInvertedResBlock(act_func='relu6' | 'h-swish') of one pin case with the oracle block's weights."""
    act, s, se, k = case
    q = _acts.PIN_GEOM
    blk = ref.layers.MBInvertedResBlock(q['ic'], q['mc'], se, q['oc'], k, s, affine=(form == 'derived'), act_func=act)
    blk.load_state_dict(oracle_blk.state_dict())
    blk.drop_connect_rate = getattr(oracle_blk, 'drop_connect_rate', 0.0)
    return blk.double().train()


def pin_fixture():
    out = OrderedDict()
    for form in _acts.PIN_FORMS:
        for case in _acts.PIN_CASES:
            o, x, r, seed = _acts.pin_oracle_block(form, case)
            want = _k7.pin_run(reference_block(form, case, o), x, r, seed)
            with _acts.wrapped_oracle():
                got = _k7.pin_run(o, x, r, seed)
            assert list(got) == list(want), (list(got), list(want))
            for k in want:
                assert np.allclose(got[k], want[k], atol=2e-6, rtol=1e-4), (form, case, k)
            for k, v in _k7.pin_record(want).items():
                out[_acts.pin_tag(form, case) + '/' + k] = v
            print('pin', _acts.pin_tag(form, case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'oracle_act_pin.npz'), **out)


if __name__ == '__main__':
    pin_fixture()
