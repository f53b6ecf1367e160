#!/usr/bin/env python3
"""Golden vectors of MBConv blocks whose squeeze-excite hidden activation differs from the block's own, recorded by running the
REFERENCE itself (imported from $TFNAS_REFERENCE, tests/_refload.py) on the CPU -- the companion of make_golden_act.py for
tests/test_sestyle_oracle_pin.py.

Where the reference exists:   TFNAS_REFERENCE=<reference dir> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sestyle.py
Output (committed):     tests/golden/oracle_sestyle_pin.npz
The reference builds its SE branch as Sequential(conv_reduce, act, conv_expand) with ``act`` chosen by the block's act_func
(models/layers.py:510-523); here the reference's own MBInvertedResBlock.forward runs over a block whose ``squeeze_excite.act``
module was replaced by the reference's module of another activation.  (Its gate is a literal torch.sigmoid in that forward and
cannot be swapped inside it: the gate is pinned in the test to torch.nn.functional.hardsigmoid instead.)  The fixture is data only
(_golden.probe of the reference's outputs and gradients, the depthwise weight gradient whole).  While recording, the styled
restatement (tests/_sestyle.py) is compared with the reference's block on the spot -- the same comparison the test replays from the
recorded side."""
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _k7  # noqa: E402
import _refload  # noqa: E402
import _sestyle  # noqa: E402

ref = _refload.import_reference()


def reference_block(form, case, oracle_blk):
    """The reference's MBInvertedResBlock of one pin case with the oracle block's weights and the SE branch's act module replaced."""
    import torch.nn as nn
    cell, se_act, s = case
    q = _sestyle.PIN_GEOM
    blk = ref.layers.MBInvertedResBlock(q['ic'], q['mc'], q['se'], q['oc'], 3, s, affine=(form == 'derived'), act_func=cell)
    blk.load_state_dict(oracle_blk.state_dict())
    blk.squeeze_excite.act = {'relu': nn.ReLU(), 'swish': ref.layers.Swish()}[se_act]
    blk.drop_connect_rate = getattr(oracle_blk, 'drop_connect_rate', 0.0)
    return blk.double().train()


def pin_fixture():
    out = OrderedDict()
    for form in _sestyle.PIN_FORMS:
        for case in _sestyle.PIN_HIDDEN:
            o, x, r, seed = _sestyle.pin_block(form, case)
            want = _k7.pin_run(reference_block(form, case, o), x, r, seed)
            got = _k7.pin_run(_sestyle.restyle(o, case[1], 'sigmoid'), x, r, seed)
            assert list(got) == list(want), (list(got), list(want))
            for k in want:
                assert np.allclose(got[k], want[k], atol=2e-6, rtol=1e-4), (form, case, k)
            for k, v in _k7.pin_record(want).items():
                out[_sestyle.pin_tag(form, case) + '/' + k] = v
            print('pin', _sestyle.pin_tag(form, case), 'ok')
    np.savez_compressed(os.path.join(HERE, 'oracle_sestyle_pin.npz'), **out)


if __name__ == '__main__':
    pin_fixture()
