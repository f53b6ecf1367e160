"""Fused-MBConv blocks in the derived-network ("retrain") path: ``layers.FusedMBConvBlock(affine=True)`` -- two BatchNorm sites,
tfnas_mbconv_fwd/bwd with TFNAS_CELL_FUSED -- against the float32 CPU restatement of tests/_fused.py in train mode, train mode
with injected drop-connect draws (images 0 and 2 dropped) and eval mode, with a negative gamma at both sites: out, dx, every
weight and BatchNorm gradient, the running statistics.  Gate: _hipcheck.worst (atol 2e-5 + rtol 1e-4 * max|ref|).  Then a
NetworkCfg whose stage 1 holds fused blocks through one train_step and one validate at 2 x 3 x 32 x 32, and the latency measurer."""
import math

import pytest
import torch

import _fused
import _hipcheck as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('mode', ['train', 'train_drop', 'eval'])
@pytest.mark.parametrize('geom', _fused.DERIVED_GEOMS, ids=_fused.geom_id)
def test_affine_block_matches_the_restatement(geom, mode):
    o, x, r, seed = _fused.derived_case(geom, mode)
    m = _fused.hip_block_like(o)
    if mode == 'eval':
        m.eval()
    if mode == 'train_drop':
        m.drop_u = o.drop_u
    assert len(m.bn_modules()) == 2 and m.training == o.training
    res = _fused.compare(o, m, x, r)
    print(_fused.geom_id(geom), mode, ' '.join('%s=%.2e/%.2e' % (k, v[0], v[1]) for k, v in res.items()))
    assert {'b.fused_conv.bn.running_mean', 'b.point_linear.bn.running_var', 'g.fused_conv.bn.weight'} <= set(res)
    bad = hc.worst(res)
    assert not bad, bad
    if mode == 'train_drop' and o.has_residual:
        assert float(torch.floor(0.6 + o.drop_u).min()) == 0.0         # (an image was really dropped)


def test_network_cfg_with_fused_blocks_trains_and_validates():
    from tfnas_amd import model_eval as me
    cfg = _fused.fused_network_config(20)
    torch.manual_seed(5)
    m = me.NetworkCfg(20, cfg, None, 0.0, 0.2).cuda()
    before = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    opt = torch.optim.SGD(m.parameters(), 0.05, momentum=0.9, weight_decay=4e-5)
    crit = me.CrossEntropyLabelSmooth(20, 0.1)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 32, 32, generator=gen).cuda()
    y = torch.randint(0, 20, (2,), generator=gen).cuda()
    for b in [m.second_stem] + [b for st in m._stages() for b in st]:
        b.drop_u = torch.tensor([0.9, 0.1])
    loss, logits = me.train_step(m, x, y, crit, opt, 5.0)
    torch.cuda.synchronize()
    assert getattr(m, '_retrain_state', None) is not None               # (RetrainState: in-place gradients, lazy join)
    assert math.isfinite(float(loss)) and torch.isfinite(logits).all()
    for k, p in m.named_parameters():
        assert torch.isfinite(p).all(), k
        assert not torch.equal(p.detach().cpu(), before[k]), k          # every parameter moved, the dense weights included
    assert float(m.stage1[0].fused_conv.bn.num_batches_tracked) == 1
    top1, top5, obj = me.validate(m, [(x, y)])
    assert all(math.isfinite(float(v)) for v in (top1, top5, obj))
    assert m.config == cfg


@pytest.mark.parametrize('mode', ['inference', 'search'])
def test_measurer_times_a_fused_block(mode):
    from tfnas_amd.lut_builder import Measurer
    t = Measurer(torch.device('cuda')).measure(16, 48, 16, 24, 3, 2, 'relu', 28, batch=4, iters=2, reps=1, mode=mode,
                                               block='FusedMBConvBlock')
    assert math.isfinite(t) and t > 0
    with pytest.raises(NotImplementedError):
        Measurer(torch.device('cuda')).measure(16, 48, 0, 24, 5, 2, 'relu', 28, batch=4, iters=2, reps=1, mode=mode,
                                               block='FusedMBConvBlock')


def test_latency_table_of_fused_blocks_has_fused_keys_and_every_width():
    from tfnas_amd import lut_builder as lb
    key, gm = [(k, g) for k, g in lb.lut_keys() if g['k'] == 3][-1]              # (the smallest images: 7 x 7)
    mb5 = [(k, g) for k, g in lb.lut_keys() if g['k'] == 5][-1]
    lut = lb.build_latency_lookup('cuda', step=10 ** 6, batch=2, iters=1, keys=[(key, gm), mb5], mode='inference',
                                  block='FusedMBConvBlock')
    want = 'FusedMBConvBlock' + key[key.index('_'):]
    assert list(lut) == ['base', want]                                          # (k = 5 geometries have no fused block)
    assert list(lut[want]) == list(range(1, gm['max_mc'] + 1))                  # every width from 1: no expand-free form
    assert all(math.isfinite(v) and v > 0 for v in lut[want].values()) and lut['base'] > 0
    with pytest.raises(ValueError):
        lb.build_latency_lookup('cuda', keys=[(key, gm)], block='ConvLayer')
