#!/usr/bin/env python3
"""Records tests/golden/block_kind_pin.json: what the plans of the three block kinds (plain MBConv, expand-free, Fused-MBConv), a
two-candidate plan and the stem and head plans hand to the library, the blocks' state_dict keys and seeded initialisation, and
the hand-written MAC / parameter counts of the k7 / expand-free / fused network configurations (tests/_kindpin.py).

Run it on the commit BEFORE a change of how kinds are decided (CPU only, the library built):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kind.py
The fixture is data only; tests/test_block_kind.py replays the same calls on the code under test."""
import json
import os
import sys
from collections import OrderedDict

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tf-nas_amd')):
    sys.path.insert(0, p)
import _fused  # noqa: E402
import _k7  # noqa: E402
import _kindpin  # noqa: E402
import _noexp  # noqa: E402


def hand_counts():
    cfgs = _kindpin.network_configs()
    out = OrderedDict()
    for size in _kindpin.HAND_SIZES:
        fm, fp = _fused.hand_counts(cfgs['fused'], size)
        out[str(size)] = OrderedDict(k7_macs=_k7.hand_macs_in_M(cfgs['k7'], size), noexp_macs=_noexp.hand_macs_in_M(cfgs['noexp'], size),
                                     fused_macs=fm, fused_params=fp)
    out['k7_params'] = _k7.hand_params_in_MB(cfgs['k7'])
    return out


def main():
    out = OrderedDict(cases=OrderedDict((_kindpin.case_tag(c), _kindpin.record_block_case(c)) for c in _kindpin.BLOCK_CASES))
    out['cases'].update(_kindpin.record_other_plans())
    out['state_keys'], out['seeded'] = _kindpin.record_forms()
    out['hand'] = hand_counts()
    with open(os.path.join(HERE, 'block_kind_pin.json'), 'w') as f:
        json.dump(out, f, indent=0, separators=(',', ':'))
        f.write('\n')
    print('wrote %d cases' % len(out['cases']))


if __name__ == '__main__':
    main()
