"""GPU: the epoch driver's training statistics and log lines (tfnas_amd/epoch.py: search_epoch / run_search with tail.SearchMeter).

Reference: train_search.py:212-225 (``train_acc = train_wo_arch / train_w_arch(...)``, ``logging.info('Train_acc %f', train_acc)``) and the
per-step lines at :351-352 and :428-430.  The expected numbers are a host replay of the reference's AverageMeters over what the steps
returned, top-k by the rank rule of include/tfnas_hip.h."""
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NUM_CLASSES = 8
FLOAT = r'(-?\d+\.\d{6})'


def _hits(logits, target, k):
    lg, hits = logits.cpu().numpy(), 0
    for row, t in zip(lg, target.cpu().tolist()):
        hits += int((row > row[t]).sum() + (row[:t] == row[t]).sum()) < k
    return hits


def test_two_epochs_report_the_reference_training_log(tmp_path, monkeypatch):
    from tfnas_amd import epoch as ep, search
    from tfnas_amd.latency import load_lat_lookup
    lut = load_lat_lookup('gpu')
    gen = torch.Generator().manual_seed(0)

    def queue(n):
        return lambda e: [(torch.randn(4, 3, 224, 224, generator=gen), torch.randint(0, NUM_CLASSES, (4,), generator=gen))
                          for _ in range(n)]
    rec = dict(w=[], a=[])
    w_step, a_step = search.w_step, search.a_step

    def rec_w(state, x, target, *a, **kw):
        assert kw.get('meter') is not None
        out = w_step(state, x, target, *a, **kw)
        rec['w'].append((out[0], out[1], target))
        return out

    def rec_a(state, x, target, *a, **kw):
        assert kw.get('meter') is not None
        out = a_step(state, x, target, *a, **kw)
        rec['a'].append((out[0], out[1], target.size(0)))
        return out
    monkeypatch.setattr(search, 'w_step', rec_w)
    monkeypatch.setattr(search, 'a_step', rec_a)
    logs = []
    hist = ep.run_search(str(tmp_path), lut, queue(3), queue(2), num_classes=NUM_CLASSES, epochs=2, warmup_epochs=1,
                         log=logs.append)
    assert [h['steps'] for h in hist] == [3, 3] and len(rec['w']) == 6 and len(rec['a']) == 2
    for h in hist:
        for k in ('train_top1', 'train_top5', 'train_objs_w'):
            assert math.isfinite(h[k]), (k, h[k])
        assert 0 <= h['train_top1'] <= h['train_top5'] <= 100
    assert 'train_objs_a' not in hist[0] and 'train_objs_l' not in hist[0]
    assert math.isfinite(hist[1]['train_objs_a']) and math.isfinite(hist[1]['train_objs_l'])

    # host replay of the reference's AverageMeters: epoch 0 = w-steps 0..2 (one path), epoch 1 = w-steps 3..5 + both alpha-steps
    for e, h in enumerate(hist):
        objs_w, top1, top5 = (search.AverageMeter() for _ in range(3))
        for loss, logits, y in rec['w'][3 * e:3 * e + 3]:
            n = y.size(0)
            objs_w.update(float(loss), n)
            top1.update(100.0 * _hits(logits, y, 1) / n, n)
            top5.update(100.0 * _hits(logits, y, 5) / n, n)
        print('epoch %d: host top1 %f top5 %f objs_w %.9g; stats %r' % (e, top1.avg, top5.avg, objs_w.avg,
                                                                        {k: v for k, v in h.items() if k.startswith('train_')}))
        assert abs(h['train_top1'] - top1.avg) <= 1e-9 and abs(h['train_top5'] - top5.avg) <= 1e-9
        assert abs(h['train_objs_w'] - objs_w.avg) <= 1e-6 * abs(objs_w.avg)
    objs_a, objs_l = search.AverageMeter(), search.AverageMeter()
    for la, ll, n in rec['a']:
        objs_a.update(float(la), n)
        objs_l.update(float(ll), n)
    assert abs(hist[1]['train_objs_a'] - objs_a.avg) <= 1e-6 * abs(objs_a.avg)
    assert abs(hist[1]['train_objs_l'] - objs_l.avg) <= 1e-6 * abs(objs_l.avg)

    # the reference's lines: step 0 of each epoch (print_freq = 100), Train_acc per epoch
    lines = [str(l) for l in logs]
    wo = [l for l in lines if l.startswith('TRAIN wo_Arch')]
    wa = [l for l in lines if l.startswith('TRAIN w_Arch')]
    acc = [l for l in lines if l.startswith('Train_acc')]
    assert len(wo) == 1 and re.fullmatch(r'TRAIN wo_Arch Step: 0000 Objs: %s R1: %s R5: %s' % (FLOAT, FLOAT, FLOAT), wo[0]), wo
    assert len(wa) == 1 and re.fullmatch(r'TRAIN w_Arch Step: 0000 Objs_W: %s R1: %s R5: %s Objs_A: %s Objs_L: %s' % ((FLOAT,) * 5),
                                         wa[0]), wa
    assert acc == ['Train_acc %f' % h['train_top1'] for h in hist]
    # the step-0 lines hold the first step's numbers
    loss0, logits0, y0 = rec['w'][0]
    got = [float(v) for v in re.findall(FLOAT, wo[0])]
    assert abs(got[0] - float(loss0)) <= 1e-6 + 1e-6 * abs(float(loss0)) and got[1] == 25.0 * _hits(logits0, y0, 1)
    loss3, logits3, y3 = rec['w'][3]
    got = [float(v) for v in re.findall(FLOAT, wa[0])]
    assert abs(got[0] - float(loss3)) <= 1e-6 + 1e-6 * abs(float(loss3)) and got[2] == 25.0 * _hits(logits3, y3, 5)
    assert abs(got[3] - float(rec['a'][0][0])) <= 1e-5 and abs(got[4] - float(rec['a'][0][1])) <= 1e-5
    assert np.isfinite(got).all()
