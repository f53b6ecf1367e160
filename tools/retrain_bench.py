#!/usr/bin/env python3
"""Throughput of the derived-network retrain step (BASELINE configs[4]: 224x224, batch 256 per GPU) on the HIP path
(tfnas_amd/model_eval.py): forward + label-smoothed loss + backward + clip + SGD, synthetic data.
  python tools/retrain_bench.py [--batch 256] [--steps 20]           (one rank per GPU under torch.distributed.run for N > 1)
  --ema off | fused | foreach: no weight EMA (default); model_eval.WeightEma kept inside the fused SGD pass; or the user-side
  stand-in, ``torch._foreach_lerp_`` over ``state_dict()`` after every step (what timm's ModelEmaV2 does).  With --ema fused /
  foreach, or --sync-steps, the line also carries the median of device-synchronised steps and the library's launch count of one step (tfnas_prof_collect; torch's
  own multi-tensor launches of the foreach stand-in are not the library's and are not in it).
  --opt sgd | sgd-groups | nesterov-groups | rmsprop-groups | rmsprop-tf-groups: the optimizer; ``-groups``: two parameter
  groups, no weight decay on BatchNorm and biases.  Built here from the public torch API (only rmsprop-tf needs tfnas_amd.optim),
  so the tool also runs against a tree whose RetrainState has no 'groups' plan -- there those optimizers take the torch route.
  --route fused | torch: ``train_step(fused=...)``; torch = clip_grad_norm_ + optimizer.step() without RetrainState.
The architecture is the all-candidate-1 (k3 e6) full-depth network scaled to the 18 ms target of SURVEY 8(c).6 -- the TF-NAS-A
config itself is not in the reference repository."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tf-nas_amd'))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--ema', choices=('off', 'fused', 'foreach'), default='off')
    ap.add_argument('--ema-decay', type=float, default=0.9999)
    ap.add_argument('--sync-steps', action='store_true', help='the median / launch-count figures of --ema, also with --ema off')
    ap.add_argument('--opt', choices=('sgd', 'sgd-groups', 'nesterov-groups', 'rmsprop-groups', 'rmsprop-tf-groups'), default='sgd')
    ap.add_argument('--route', choices=('fused', 'torch'), default='fused')
    args = ap.parse_args()
    from tfnas_amd import geometry as g, model_eval as me
    from tfnas_amd.elasticity import fit_mc_num_by_latency
    from tfnas_amd.latency import load_lat_lookup
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (('RANK', '0'), ('WORLD_SIZE', '1'), ('LOCAL_RANK', '0')))
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if 'RANK' in os.environ:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29571')
        dist.init_process_group('nccl', rank=rank, world_size=world)     # (NOT device_id=...: see DESIGN.md 4a, eager RCCL init)
    lut = load_lat_lookup('gpu')
    mc = g.initial_mc_num_dddict()
    arch = OrderedDict((st, OrderedDict((b, 1) for b in mc[st])) for st in mc)
    mc, lat = fit_mc_num_by_latency(arch, mc, g.get_mc_num_dddict(g.make_mc_mask_dddict(), is_max=True),
                                    g.make_lat_lookup_key_dddict(), lut, 18.0, list(mc.keys()), 1)
    torch.manual_seed(0)
    model = me.Network(1000, arch, mc, lut, 0.2, 0.2).to(dev)
    params = model.parameters()
    if args.opt.endswith('-groups'):
        # the recipes' two groups from the public torch API (optim.param_groups does the same): no decay on BatchNorm and biases
        rest = {id(p) for mod in model.modules() if isinstance(mod, torch.nn.modules.batchnorm._NormBase)
                for p in mod.parameters(recurse=False)} | {id(p) for k, p in model.named_parameters() if k.endswith('bias')}
        params = [{'params': [p for p in model.parameters() if id(p) not in rest], 'weight_decay': 4e-5},
                  {'params': [p for p in model.parameters() if id(p) in rest], 'weight_decay': 0.0}]
    kind = args.opt[:-len('-groups')] if args.opt.endswith('-groups') else args.opt
    if kind in ('sgd', 'nesterov'):
        opt = torch.optim.SGD(params, 0.2, momentum=0.9, weight_decay=4e-5, nesterov=kind == 'nesterov')
    elif kind == 'rmsprop':
        opt = torch.optim.RMSprop(params, 0.016, alpha=0.9, eps=1e-3, momentum=0.9, weight_decay=4e-5)
    else:
        from tfnas_amd.optim import RMSpropTF
        opt = RMSpropTF(params, 0.016, alpha=0.9, eps=1e-3, momentum=0.9, weight_decay=4e-5)
    fused = args.route == 'fused'
    crit = me.CrossEntropyLabelSmooth(1000, 0.1)
    x = torch.randn(args.batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (args.batch,), device=dev)
    ema = me.WeightEma(model, args.ema_decay) if args.ema == 'fused' else None
    shadow = live = None
    if args.ema == 'foreach':
        live = [v for v in model.state_dict().values() if v.is_floating_point()]
        shadow = [v.detach().clone() for v in live]

    def step():
        me.train_step(model, x, y, crit, opt, 5.0, fused=fused, ema=ema)
        if shadow is not None:
            if live[0].data_ptr() != next(iter(model.state_dict().values())).data_ptr():      # (the first step built the arena)
                live[:] = [v for v in model.state_dict().values() if v.is_floating_point()]
            torch._foreach_lerp_(shadow, live, 1.0 - args.ema_decay)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier(device_ids=[local])
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier(device_ids=[local])
    dt = time.perf_counter() - t0
    extra = {}
    if args.ema != 'off' or args.sync_steps:
        import ctypes as C
        from tfnas_amd import _lib
        each = []
        for _ in range(args.steps):                                  # device-synchronised steps: their median
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            each.append(time.perf_counter() - t1)
        lib = _lib.lib()
        nfam = lib.tfnas_prof_count()
        lib.tfnas_prof_enable((1 << nfam) - 1)
        step()
        torch.cuda.synchronize()
        total = 0
        for i in range(nfam):
            cnt, ms = C.c_uint64(0), C.c_double(0.0)
            _lib.check(lib.tfnas_prof_collect(i, C.byref(cnt), C.byref(ms)), 'tfnas_prof_collect')
            total += cnt.value
        lib.tfnas_prof_enable(0)
        extra = dict(ema=args.ema, median_sync_step_ms=round(sorted(each)[len(each) // 2] * 1e3, 3), library_launches_per_step=total,
                     ema_tensors=len(shadow) if shadow is not None else None)
    if rank == 0:
        print(json.dumps(dict(metric='derived-network retrain images/sec', value=round(args.batch * world * args.steps / dt, 1),
                              ms_per_step=round(dt / args.steps * 1e3, 2), opt=args.opt, route=args.route,
                              retrain_state=getattr(model, '_retrain_state', None) is not None, n_gpus=world, batch_per_gpu=args.batch, dtype='fp32',
                              arch='all-op-1 full depth, widths scaled to 18 ms (%.3f ms in the LUT)' % lat,
                              params_MB=round(sum(p.numel() for p in model.parameters()) / 1e6, 3), **extra)))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
