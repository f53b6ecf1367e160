"""Derived ("searched") network for the retrain path -- drop-in for the reference's ``models/model_eval.py``
(BASELINE configs[4]).

``Network(num_classes, parsed_arch, mc_num_dddict, lat_lookup, dropout_rate, drop_connect_rate)`` (model_eval.py:31-244) and
``NetworkCfg(num_classes, model_config, ...)`` (:247-430) with the reference's module / parameter / buffer names (``state_dict``
keys identical, incl. BatchNorm running statistics), ``forward(x) -> logits``, ``get_lookup_latency(x)`` and ``config``.  Every
block -- stems, MBConv blocks with AFFINE BatchNorm, running statistics in train / eval mode and drop-connect, the feature-mix
head -- runs on the HIP kernels of the search path (``tfnas_mbconv_fwd/bwd``, ``tfnas_head_affine_fwd/bwd``: the affine part is
folded into the per-channel statistics tables, csrc/bn_affine.hip); dropout is a torch op, and so are the classifier GEMM and
the loss inside ``forward``.  ``CrossEntropyLabelSmooth`` and ``train_step`` / ``validate`` restate train_eval.py:72-85, 228-293;
there the classifier, the (label-smoothed) loss, their gradients and top-1 / top-5 are the retrain tail's HIP launches
(tail.RetrainTailFn, ``FUSED_TAIL``) whenever ``fused_tail_eligible`` says the model and the criterion are what those compute.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, geometry
from .functions import CellPlan, HeadAffineFn, MBConvAffineFn
from .layers import ConvLayer, FusedMBConvBlock, IdentityLayer, LinearLayer, MBInvertedResBlock
from .parsing import derived_config


class _StemBlock:
    """first_stem.conv + second_stem presented as one candidate block of a TFNAS_MODE_STEM cell."""

    def __init__(self, first, second):
        self.first, self.second = first, second
        self.mid_channels, self.kernel_size, self.se_channels = second.mid_channels, second.kernel_size, second.se_channels

    def hip_params(self):
        se = self.second.squeeze_excite
        return [self.first.conv.weight, self.second.depth_conv.conv.weight, self.second.point_linear.conv.weight,
                se.conv_reduce.weight, se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias]


class _HeadBlock:
    def __init__(self, layer):
        self.layer = layer
        self.mid_channels, self.kernel_size, self.se_channels = layer.out_channels, 3, 0

    def hip_params(self):
        return [self.layer.conv.weight]


class _DerivedBase(nn.Module):
    def _finish(self, num_classes, head_act='swish'):
        _lib.act_id(head_act)
        self.feature_mix_layer = ConvLayer(320, 1280, kernel_size=1, stride=1, affine=True, act_func=head_act)
        self.global_avg_pooling = nn.AdaptiveAvgPool2d(1)
        self.classifier = LinearLayer(1280, num_classes)
        self._initialization()
        self._stem_plan = self._head_plan = None
        from .functions import adopt_modes
        adopt_modes(self)                      # self.hip_modes (functions.HipModes), shared by every sub-module's plans

    def set_hip_modes(self, **kw):
        """e.g. set_hip_modes(gemm='bf16'): this model's launches only (TfnasCellDesc.gemm_mode; functions.HipModes)."""
        for k, v in kw.items():
            if not hasattr(self.hip_modes, k):
                raise AttributeError(k)
            setattr(self.hip_modes, k, v)

    def _stages(self):
        return [getattr(self, 'stage%d' % i) for i in range(1, 7)]

    def _stem(self, x):
        fs, ss = self.first_stem, self.second_stem
        if self._stem_plan is None:
            self._stem_plan = CellPlan(27, ss.out_channels, 1, 'relu', [_StemBlock(fs, ss)], mode=_lib.MODE_STEM, modes=self.hip_modes)
        plan = self._stem_plan
        bns = [fs.bn, ss.depth_conv.bn, ss.point_linear.bn]
        conv = plan.params()
        bnp = [t for m in bns for t in (m.weight, m.bias)]
        return MBConvAffineFn.apply(plan, x, None, bns, self.training, len(conv), *conv, *bnp)

    def _head(self, x):
        fm = self.feature_mix_layer
        if self._head_plan is None:
            self._head_plan = CellPlan(fm.in_channels, 4, 1, fm.act_func, [_HeadBlock(fm)], mode=_lib.MODE_HEAD, modes=self.hip_modes)
        return HeadAffineFn.apply(self._head_plan, x, fm.bn, self.training, fm.conv.weight, fm.bn.weight, fm.bn.bias)

    def features(self, x):
        """Everything in front of the classifier: stem -> stages -> head -> dropout, [N, 1280]."""
        x = self._stem(x)
        for stage in self._stages():
            for block in stage:
                x = block(x)
        x = self._head(x)                                   # feature_mix_layer + global_avg_pooling, [N, 1280]
        if self.dropout_rate > 0.0:
            x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return x

    def forward(self, x):
        return self.classifier(self.features(x))

    def get_lookup_latency(self, x):
        """Sum of the looked-up block latencies (model_eval.py:133-212); ``x`` only provides the input resolution."""
        if not self.lat_lookup:
            return 0.0
        lat = self.lat_lookup['base']
        size = (x.size(-1) - 1) // 2 + 1                    # after first_stem (stride 2); second_stem keeps it
        for stage in self._stages():
            for b in stage:
                if isinstance(b, IdentityLayer):           # a skipped block costs nothing and keeps the resolution
                    continue
                key = '{}_{}_{}_{}_{}_{}_s{}_{}'.format(b.name, size, b.in_channels, b.se_channels, b.out_channels,
                                                        geometry.kernel_tag(b.kernel_size, getattr(b, 'dilation', 1),
                                                                            getattr(b, 'mix_kernels', None)), b.stride,
                                                        b.act_func)
                lat += self.lat_lookup[key][b.mid_channels]
                size = (size - 1) // b.stride + 1
        return lat

    @staticmethod
    def _block_config(b):
        if isinstance(b, IdentityLayer):
            return b.config
        return {'name': b.name, 'in_channels': b.in_channels, 'mid_channels': b.mid_channels,
                'se_channels': b.se_channels, 'out_channels': b.out_channels, 'kernel_size': b.kernel_size, 'stride': b.stride,
                'groups': 1, 'has_shuffle': False, 'bias': False, 'use_bn': True, 'affine': True, 'act_func': b.act_func,
                **geometry.se_style_keys(b.se_act, b.se_gate),      # ('se_act' / 'se_gate': only where not the default)
                **geometry.dilation_keys(getattr(b, 'dilation', 1)),  # ('dilation': only where not 1)
                **geometry.mix_keys(getattr(b, 'mix_kernels', None))}  # ('mix_kernels': only a MixConv block)

    @property
    def config(self):
        from .parsing import _conv_layer_config
        cfg = {'first_stem': _conv_layer_config(3, 32, 3, 2, 'relu'), 'second_stem': self._block_config(self.second_stem)}
        for i, stage in enumerate(self._stages(), start=1):
            cfg['stage%d' % i] = [self._block_config(b) for b in stage]
        cfg['feature_mix_layer'] = _conv_layer_config(320, 1280, 1, 1, self.feature_mix_layer.act_func)
        cl = self.classifier
        cfg['classifier'] = {'name': 'LinearLayer', 'in_features': cl.in_features, 'out_features': cl.out_features,
                             'bias': True, 'use_bn': False, 'affine': False, 'act_func': None, 'ops_order': 'weight_bn_act'}
        return cfg

    def _initialization(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)) and m.bias is not None:
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)


class Network(_DerivedBase):
    def __init__(self, num_classes, parsed_arch, mc_num_dddict, lat_lookup=None, dropout_rate=0.0, drop_connect_rate=0.0,
                 primitives=None, se_style=None):
        super().__init__()
        self.lat_lookup, self.mc_num_dddict, self.parsed_arch = lat_lookup, mc_num_dddict, parsed_arch
        self.dropout_rate, self.drop_connect_rate = dropout_rate, drop_connect_rate
        self.block_count = 1 + sum(len(parsed_arch[st]) for st in parsed_arch)
        self.block_idx = 0
        self.first_stem = ConvLayer(3, 32, kernel_size=3, stride=2, affine=True, act_func='relu')
        self.second_stem = MBInvertedResBlock(32, 32, 8, 16, kernel_size=3, stride=1, affine=True, act_func='relu')
        self.block_idx += 1
        self.second_stem.drop_connect_rate = self.drop_connect_rate * self.block_idx / self.block_count
        for name, cfg in geometry.STAGES.items():
            stage = nn.ModuleList()
            for i, block_name in enumerate(parsed_arch[name]):
                self.block_idx += 1
                op = parsed_arch[name][block_name]
                ic, oc, s = cfg['ics'][i], cfg['ocs'][i], cfg['ss'][i]
                # (``primitives``: what the searched network was built with, model_search.Network(primitives=...))
                prim = geometry.cell_primitives(primitives, name, block_name)[op]
                if prim == geometry.SKIP:              # a chosen skip: counted like any block, nothing to drop-connect
                    stage.append(IdentityLayer(ic, oc))
                    continue
                layer, mc, se, k = geometry.primitive_block(prim, ic, mc_num_dddict[name][block_name][op])
                cls = FusedMBConvBlock if layer == 'FusedMBConvBlock' else MBInvertedResBlock
                # (``se_style``: likewise -- None, one (se_act, se_gate) pair or a {stage: pair} mapping; the stems keep theirs)
                se_act, se_gate = _lib.se_style_pair(geometry.cell_se_style(se_style, name, block_name))
                dil = geometry.dilation_keys(geometry.primitive_dilation(prim))      # (FusedMBConvBlock has no such argument)
                mk = geometry.primitive_mix_kernels(prim)
                if mk is not None:
                    dil['mix_kernels'] = mk
                blk = cls(ic, mc, se, oc, k, s, affine=True, act_func=cfg['act'], se_act=se_act, se_gate=se_gate, **dil)
                blk.drop_connect_rate = self.drop_connect_rate * self.block_idx / self.block_count
                stage.append(blk)
            setattr(self, name, stage)
        self._finish(num_classes)


class NetworkCfg(_DerivedBase):
    """Built from the exported ``model.config`` JSON (model_eval.py:247-300; parsing.derived_config writes it)."""

    def __init__(self, num_classes, model_config, lat_lookup=None, dropout_rate=0.0, drop_connect_rate=0.0):
        super().__init__()
        self.lat_lookup, self.model_config = lat_lookup, model_config
        self.dropout_rate, self.drop_connect_rate = dropout_rate, drop_connect_rate
        self.block_count = 1 + sum(len(v) for k, v in model_config.items() if k.startswith('stage'))
        self.block_idx = 0

        def mb(c, fused_ok=True):
            kinds = {'MBInvertedResBlock': MBInvertedResBlock}
            if fused_ok:                                   # (stage entries only: second_stem stays an MBConv, fused with first_stem)
                kinds['FusedMBConvBlock'] = FusedMBConvBlock
            if c['name'] not in kinds or c.get('groups', 1) != 1 or c.get('has_shuffle') or c.get('bias'):
                raise NotImplementedError('only plain MBInvertedResBlock / FusedMBConvBlock configs are supported: %r' % (c,))
            se_act, se_gate = c.get('se_act'), c.get('se_gate', 'sigmoid')
            if not fused_ok and _lib.se_style_id(se_act, se_gate) != 0:
                raise NotImplementedError('second_stem runs fused with first_stem and keeps the default squeeze-excite: %r' % (c,))
            dil = geometry.dilation_keys(c.get('dilation', 1))
            if dil and (not fused_ok or c['name'] != 'MBInvertedResBlock'):
                raise NotImplementedError('only an MBInvertedResBlock of a stage may be dilated (second_stem runs fused with '
                                          'first_stem, FusedMBConvBlock has no depthwise convolution): %r' % (c,))
            if c.get('mix_kernels') is not None:
                if not fused_ok or c['name'] != 'MBInvertedResBlock':
                    raise NotImplementedError('only an MBInvertedResBlock of a stage may be a MixConv block (second_stem runs '
                                              'fused with first_stem, FusedMBConvBlock has no depthwise convolution): %r' % (c,))
                dil['mix_kernels'] = tuple(c['mix_kernels'])
            return kinds[c['name']](c['in_channels'], c['mid_channels'], c['se_channels'], c['out_channels'],
                                      c['kernel_size'], c['stride'], affine=c.get('affine', True), act_func=c['act_func'],
                                      se_act=se_act, se_gate=se_gate, **dil)
        fs = model_config['first_stem']
        self.first_stem = ConvLayer(fs['in_channels'], fs['out_channels'], fs['kernel_size'], fs['stride'], affine=True,
                                    act_func=fs['act_func'])
        self.second_stem = mb(model_config['second_stem'], fused_ok=False)
        self.block_idx += 1
        self.second_stem.drop_connect_rate = self.drop_connect_rate * self.block_idx / self.block_count
        for i in range(1, 7):
            stage = nn.ModuleList()
            for c in model_config['stage%d' % i]:
                self.block_idx += 1
                if c['name'] == 'IdentityLayer':       # (counted, as the reference's loop over the entries does; no drop-connect)
                    stage.append(IdentityLayer(**{k: v for k, v in c.items() if k != 'name'}))
                    continue
                blk = mb(c)
                blk.drop_connect_rate = self.drop_connect_rate * self.block_idx / self.block_count
                stage.append(blk)
            setattr(self, 'stage%d' % i, stage)
        # (the head's activation as the config names it: MobileNetV3-style configs end in 'h-swish')
        self._finish(num_classes, model_config.get('feature_mix_layer', {}).get('act_func') or 'swish')


class CrossEntropyLabelSmooth(nn.Module):
    """train_eval.py:72-85: mean over the batch of -sum_k ((1-eps) onehot + eps/K) log_softmax."""

    def __init__(self, num_classes, epsilon):
        super().__init__()
        self.num_classes, self.epsilon = num_classes, epsilon

    def forward(self, xs, targets):
        return F.cross_entropy(xs, targets, label_smoothing=self.epsilon)


# TFNAS_RETRAIN_DIRECT=0: the blocks return gradient temporaries and autograd adds them into the arena (one launch per parameter);
# TFNAS_RETRAIN_LAZY=0: every block joins its weight-gradient kernels before it returns.
DIRECT_GRADS = True          # (tests flip these two module flags to compare with the plain route)
LAZY_JOIN = True


# the classifier + loss + top-k tail of train_step / validate on the HIP launches of tail.RetrainTailFn (tests flip it to compare with
# the torch route)
FUSED_TAIL = True


def _has_hooks(m):
    return bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, '_backward_pre_hooks', None))


def _fused_tail_plan(model, criterion, validating=False):
    """(derived network, eps) when the fused retrain tail computes exactly what ``criterion(model(x), target)`` would, else None."""
    core = model
    if not isinstance(core, _DerivedBase):
        # a wrapper's own forward is skipped by the fused route (features + tail are called on the network itself): only look
        # through one whose forward is nothing but ``self.module(x)`` -- nn.DataParallel on at most one device
        core = getattr(model, 'module', None)
        if not (isinstance(core, _DerivedBase) and isinstance(model, nn.DataParallel) and len(model.device_ids) <= 1):
            return None
    lin = core.classifier.linear
    W, b = lin.weight, lin.bias
    if b is None or any(_has_hooks(m) for m in (model, core, core.classifier, lin)):
        return None
    for p in (W, b):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != W.device:
            return None
    trainable = W.requires_grad and b.requires_grad
    frozen = not W.requires_grad and not b.requires_grad
    if not (trainable or (validating and frozen)):
        return None
    from .tail import cls_shapes_ok
    K = lin.out_features
    if not cls_shapes_ok(lin.in_features, K):
        return None
    if isinstance(criterion, CrossEntropyLabelSmooth):
        if type(criterion) is not CrossEntropyLabelSmooth or criterion.num_classes != K or _has_hooks(criterion):
            return None
        eps = criterion.epsilon
    elif type(criterion) is nn.CrossEntropyLoss:
        if criterion.weight is not None or criterion.ignore_index != -100 or criterion.reduction != 'mean' or _has_hooks(criterion):
            return None
        eps = criterion.label_smoothing
    elif validating and (criterion is None or criterion is F.cross_entropy):
        eps = 0.0
    else:
        return None
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        return None
    return core, eps


def fused_tail_eligible(model, criterion, validating=False):
    """True when train_step (``validating``: validate) may run classifier + loss + top-k on the retrain tail's HIP launches:
    the model is a derived network (or nn.DataParallel on one device around one) without forward / backward hooks on the way;
    classifier weight and bias are contiguous CUDA fp32 and both trainable (validate: or both frozen); in_features % 4 == 0,
    in_features and num_classes <= 4096, LDS <= 64 KiB; and the criterion is ``CrossEntropyLabelSmooth`` with num_classes == K,
    or ``nn.CrossEntropyLoss`` with no class weights, the default ignore_index and mean reduction (eps = its label_smoothing),
    or -- validate only -- None / ``F.cross_entropy``.  Anything else takes the torch route untouched."""
    return _fused_tail_plan(model, criterion, validating) is not None


class RetrainState:
    """Flat weight / gradient / momentum arenas of the derived network (path.WeightArena) + the fused step tail of the search
    path: ``.grad`` of every parameter is a view into ONE gradient buffer (autograd accumulates in place), so a data-parallel
    step is ONE all-reduce of that buffer (no ``torch.cat``, no copy back -- what apex DDP's ``delay_allreduce`` flattening does,
    train_eval_amp.py:188) and clip_grad_norm_ + SGD(momentum, weight decay) are the two launches of ``tfnas_sgd_clip_step``
    (1 / world folded in), sharing the momentum buffers with the caller's ``torch.optim.SGD`` (checkpoints keep working)."""

    def __init__(self, model):
        from .path import WeightArena
        self.model = model
        self.arena = WeightArena(model)
        self._bound = None
        self._scratch = self._gnorm = None
        # the 'groups' plan: squared-gradient arena, device group map (+ the membership it was built for), descriptor, step counters
        self._v = self._gmap = self._gmap_key = self._gdesc = None
        self._gbound = None
        self._gsteps = ()

    def intact(self):
        return self.arena.intact()

    @staticmethod
    def fusable(opt, model=None):
        """The fused tail updates EVERY parameter of the arena with one set of hyper-parameters, so it stands in for
        ``optimizer.step()`` only when that is what the optimizer would do: a plain SGD with ONE param group that holds exactly
        the model's parameters, all of them trainable, and no step hooks registered (they would never run).  Anything else --
        frozen parameters, a subset, per-group rates, hooks -- takes torch's clip_grad_norm_ + optimizer.step()."""
        g = opt.param_groups
        if not (isinstance(opt, torch.optim.SGD) and len(g) == 1 and not g[0].get('nesterov') and not g[0].get('dampening')
                and not g[0].get('maximize')):
            return False
        if getattr(opt, '_optimizer_step_pre_hooks', None) or getattr(opt, '_optimizer_step_post_hooks', None):
            return False
        if model is not None:
            mine = list(model.parameters())
            if not all(p.requires_grad for p in mine) or {id(p) for p in g[0]['params']} != {id(p) for p in mine}:
                return False
        return True

    @staticmethod
    def plan(opt, model):
        """Which fused tail stands in for ``optimizer.step()`` -- pure inspection, nothing is touched.  'sgd': ``fusable`` holds
        (``tfnas_sgd_clip_step``, as ever).  'groups' (``tfnas_opt_groups_step``): ``torch.optim.SGD`` (dampening 0, not maximize;
        Nesterov allowed), ``torch.optim.RMSprop`` (not centered / maximize / capturable) or ``optim.RMSpropTF`` with 1..8 param
        groups that are disjoint and together hold exactly the model's parameters, all trainable; momentum, nesterov, alpha and eps
        equal across the groups (lr and weight_decay may differ); no step hooks.  None: torch's clip_grad_norm_ +
        optimizer.step()."""
        from .optim import RMSpropTF
        if RetrainState.fusable(opt, model):
            return 'sgd'
        g = opt.param_groups
        if not 1 <= len(g) <= _lib.OPT_MAX_GROUPS:
            return None
        if getattr(opt, '_optimizer_step_pre_hooks', None) or getattr(opt, '_optimizer_step_post_hooks', None):
            return None
        if any(q.get('maximize') or q.get('differentiable') for q in g):
            return None
        if isinstance(opt, torch.optim.SGD):
            shared = ('momentum', 'nesterov')
            if any(q.get('dampening') for q in g):
                return None
        elif isinstance(opt, (torch.optim.RMSprop, RMSpropTF)):
            shared = ('momentum', 'alpha', 'eps')
            if any(q.get('centered') or q.get('capturable') for q in g) or not g[0]['eps'] > 0 or not 0 <= g[0]['alpha'] <= 1:
                return None
        else:
            return None
        if any(q[k] != g[0][k] for q in g[1:] for k in shared) or not g[0]['momentum'] >= 0:
            return None
        ids = [id(p) for q in g for p in q['params']]
        mine = list(model.parameters())
        if len(set(ids)) != len(ids) or set(ids) != {id(p) for p in mine} or not all(p.requires_grad for p in mine):
            return None
        return 'groups'

    def _bind_groups(self, opt):
        """The 'groups' plan's share of the state: the optimizer's ``momentum_buffer`` / ``square_avg`` become views into the m / v
        arenas (existing values are copied in; missing state starts as the optimizer itself would start it), and the device group
        map is (re)built when the groups' membership is not the one it was built for.  Returns (kind, flags)."""
        from .optim import RMSpropTF
        a = self.arena
        hp = opt.param_groups[0]
        if isinstance(opt, RMSpropTF):
            kind, flags, want = _lib.OPT_RMSPROP_TF, 0, ('momentum_buffer', 'square_avg')
        elif isinstance(opt, torch.optim.RMSprop):
            kind, flags, want = _lib.OPT_RMSPROP, 0, (('momentum_buffer', 'square_avg') if hp['momentum'] > 0 else ('square_avg',))
        else:
            kind, flags = _lib.OPT_SGD, (_lib.OPT_NESTEROV if hp.get('nesterov') else 0)
            want = ('momentum_buffer',) if hp['momentum'] != 0 else ()
        if kind != _lib.OPT_SGD and self._v is None:
            self._v = torch.zeros(a.total, device=a.device, dtype=torch.float32)
        arenas = {'momentum_buffer': a.m, 'square_avg': self._v}

        def bound(p):
            st, o = opt.state.get(p, {}), a.slot[id(p)][0]
            return all(st.get(k) is not None and st[k].data_ptr() == arenas[k].data_ptr() + 4 * o for k in want)

        if not (self._gbound == (id(opt), want) and bound(a.params[0]) and bound(a.params[-1])):
            with torch.no_grad():
                if 'momentum_buffer' not in want:
                    a.m.zero_()                          # (nobody's state: what a later momentum > 0 starts from)
                steps = []
                for p in a.params:
                    o, n = a.slot[id(p)]
                    st = opt.state[p]
                    if kind != _lib.OPT_SGD and 'step' not in st:
                        st['step'] = 0 if kind == _lib.OPT_RMSPROP_TF else torch.zeros(())     # (torch's: a CPU scalar tensor)
                    for k in want:
                        view = arenas[k][o:o + n].view(p.shape)
                        old = st.get(k)
                        if old is None:
                            view.fill_(1.0 if (k == 'square_avg' and kind == _lib.OPT_RMSPROP_TF) else 0.0)
                        elif old.data_ptr() != view.data_ptr():
                            view.copy_(old)
                        st[k] = view
                    if 'step' in st:
                        steps.append(st)
                self._gsteps = steps
            self._gbound = (id(opt), want)
            self._bound = None                           # (the 'sgd' plan re-binds if it ever gets this arena back)
        key = tuple(tuple(id(p) for p in q['params']) for q in opt.param_groups)
        if self._gmap is None or self._gmap_key != key:
            ids = torch.full((a.total // 64,), 255, dtype=torch.uint8)
            for k, q in enumerate(opt.param_groups):
                for p in q['params']:
                    o, n = a.slot[id(p)]
                    ids[o // 64:(o + n + 63) // 64] = k
            self._gmap, self._gmap_key = ids.to(a.device), key
        return kind, flags

    def _step_groups(self, opt, grad_clip, scale, ema, stream):
        """clip + the optimizer's update over the whole arena with per-group lr / weight decay: the two launches of
        ``tfnas_opt_groups_step`` (the EMA of the parameters inside the second one)."""
        import ctypes as C
        a = self.arena
        kind, flags = self._bind_groups(opt)
        d = self._gdesc
        if d is None:
            d = self._gdesc = _lib.TfnasOptGroups()
        g = opt.param_groups
        d.kind, d.flags, d.ngroups = kind, flags, len(g)
        for k, q in enumerate(g):                        # read at every step: schedulers write lr here
            d.lr[k], d.wd[k] = float(q['lr']), float(q['weight_decay'])
        d.momentum = float(g[0]['momentum'])
        d.alpha, d.eps = float(g[0].get('alpha', 0.0)), float(g[0].get('eps', 0.0))
        d.max_norm, d.grad_scale = float(grad_clip), float(scale)
        eflat = None
        if ema is not None:
            _, bufs = ema._sync(self.model)
            if ema._arena is not a:
                raise RuntimeError('RetrainState.step: the EMA could not lay its parameter shadow out on this arena')
            alpha = ema.alpha()
            d.ema_alpha, eflat = alpha, ema._pflat
        _lib.check(_lib.lib().tfnas_opt_groups_step(C.byref(d), _lib.ptr(a.w), _lib.ptr(a.g), _lib.ptr(a.m), _lib.ptr(self._v),
                                                    _lib.ptr(eflat), _lib.ptr(self._gmap), a.total, _lib.ptr(self._scratch),
                                                    self._scratch.numel(), _lib.ptr(self._gnorm), stream), 'tfnas_opt_groups_step')
        if ema is not None:
            ema._update_buffers(bufs, alpha)
            ema.updates += 1
        for st in self._gsteps:                          # what optimizer.step() counts per parameter
            st['step'] += 1

    def _bind_momentum(self, opt):
        a = self.arena
        probe = a.params[0]
        buf = opt.state.get(probe, {}).get('momentum_buffer')
        if self._bound is opt and buf is not None and buf.data_ptr() == a.m.data_ptr() + 4 * a.slot[id(probe)][0]:
            return
        with torch.no_grad():
            for p in a.params:
                o, n = a.slot[id(p)]
                view = a.m[o:o + n].view(p.shape)
                old = opt.state.get(p, {}).get('momentum_buffer')
                if old is not None and old.data_ptr() != view.data_ptr():
                    view.copy_(old)
                elif old is None:
                    view.zero_()
                opt.state[p]['momentum_buffer'] = view
        self._bound = opt

    def begin(self):
        """Zero the gradient arena (one memset), make every .grad a view of it, and switch the blocks' backward to writing the
        gradients in place with a lazily joined weight-gradient stream (functions.retrain_context)."""
        from . import functions
        a = self.arena
        a.g.zero_()
        for p in a.params:
            if p.grad is None or p.grad.data_ptr() != a.grad_ptr(p):
                p.grad = a.grad_view(p)
        functions.retrain_context(DIRECT_GRADS, LAZY_JOIN, self._modes_owner())

    def _modes_owner(self):
        """The module whose ``hip_modes`` the blocks of this model consult: the model itself, or -- when ``self.model`` is a
        wrapper without one (nn.DataParallel / DDP / nn.Sequential / a user wrapper) -- the first sub-module that has it."""
        m = self.model
        if getattr(m, 'hip_modes', None) is not None:
            return m
        for sub in m.modules():
            if getattr(sub, 'hip_modes', None) is not None:
                return sub
        return None                                      # (no HIP module inside: functions.retrain_context falls back to DEFAULT_MODES)

    def end(self):
        """Join the weight-gradient stream and leave the training-step context (also on an error path)."""
        from . import functions
        owner = self._modes_owner()
        modes = owner.hip_modes if owner is not None else functions.DEFAULT_MODES
        if modes.lazy_join:
            functions.retrain_join(self.arena.device)
        functions.retrain_context(False, False, owner)

    def step(self, opt, grad_clip, group=None, ema=None, plan=None):
        """Join, all-reduce (with a group), then clip + SGD over the whole arena in two launches.  ``plan`` (what ``plan(opt,
        model)`` returned, where the caller already asked): 'groups' takes the same two launches through ``tfnas_opt_groups_step``
        -- parameter groups, Nesterov, RMSprop; 'sgd' makes the calls below.  ``ema`` (a WeightEma): the SGD
        pass keeps the parameters' average as it stores them (``tfnas_sgd_clip_ema_step``, same two launches), ONE further launch
        averages the floating-point buffers, and the EMA's count goes up by one.  The average is taken after the all-reduce, so the
        parameter shadows are identical on all ranks; the buffer shadows are per rank, as the running statistics themselves are
        without sync-stats."""
        import ctypes as C
        import torch.distributed as dist
        a = self.arena
        self.end()                                       # the gradients are complete on the current stream from here on
        if plan is None:
            plan = self.plan(opt, self.model)
        groups = plan == 'groups'
        if not groups:
            self._bind_momentum(opt)
        hp = opt.param_groups[0]
        scale = 1.0
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(a.g, group=group)            # ONE message: the whole gradient arena
            scale = 1.0 / dist.get_world_size(group)
        dev = a.device
        nblk = (a.total + 8191) // 8192
        if self._scratch is None or self._scratch.numel() < nblk + 8:
            self._scratch = torch.empty(max(4096, 2 * nblk), device=dev, dtype=torch.float64)
            self._gnorm = torch.zeros(2, device=dev, dtype=torch.float32)
        off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(a.total)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if groups:
            self._step_groups(opt, grad_clip, scale, ema, stream)
        elif ema is None:
            _lib.check(_lib.lib().tfnas_sgd_clip_step(_lib.ptr(a.w), _lib.ptr(a.g), _lib.ptr(a.m), 1, off, None, ln, float(grad_clip),
                                                      float(hp['lr']), float(hp['momentum']), float(hp['weight_decay']), float(scale),
                                                      _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(self._gnorm), stream),
                       'tfnas_sgd_clip_step')
        else:
            _, bufs = ema._sync(self.model)
            if ema._arena is not a:
                raise RuntimeError('RetrainState.step: the EMA could not lay its parameter shadow out on this arena')
            alpha = ema.alpha()
            _lib.check(_lib.lib().tfnas_sgd_clip_ema_step(_lib.ptr(a.w), _lib.ptr(a.g), _lib.ptr(a.m), 1, off, None, ln,
                                                          float(grad_clip), float(hp['lr']), float(hp['momentum']),
                                                          float(hp['weight_decay']), float(scale), _lib.ptr(ema._pflat), alpha,
                                                          _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(self._gnorm),
                                                          stream), 'tfnas_sgd_clip_ema_step')
            ema._update_buffers(bufs, alpha)
            ema.updates += 1
        # what optimizer.step() would have recorded: learning-rate schedulers check these before their own step()
        if hasattr(opt, '_step_count'):
            opt._step_count += 1
        opt._opt_called = True


class WeightEma:
    """Exponential moving average of a derived network's weights -- what the MobileNetV3 / MixNet / EfficientNet / FBNet recipes
    evaluate and publish.  Shadows every parameter and every floating-point buffer of ``model`` (the shadow starts as a copy);
    integer buffers (``num_batches_tracked``) are copied at each update, not averaged.  One update is
    ``shadow <- fma(alpha_t, live - shadow, shadow)`` with ``alpha_t = 1 - min(decay, (1 + t) / (10 + t))`` (``warmup``; else
    ``1 - decay``), t = the updates done so far, formed in Python floats and handed to the kernels as the step weight itself.

    Parameters: where the model has an intact ``RetrainState`` the shadow is ONE flat tensor with the arena's layout (gaps zero, and
    they stay zero), and ``RetrainState.step(..., ema=self)`` keeps it inside the update pass on both plans (``tfnas_sgd_clip_ema_step``
    on 'sgd', the ``ema`` argument of ``tfnas_opt_groups_step`` on 'groups': no launch).
    When the arena is rebuilt (``model.to()``, ``p.data = ...``) the shadow re-lays itself by parameter name and keeps its values.
    Float buffers: on a CUDA model they are moved into one flat tensor (path.BufferArena) when the EMA is attached, so that their
    average is ONE ``tfnas_ema_lerp`` launch per step.  Without an arena (CPU; an optimizer that ``RetrainState.plan`` sends to
    the torch route, before any fused step) the shadows are per tensor and the update is ``torch._foreach_lerp_``.

    Known property of any fp32 EMA (timm's ModelEmaV2 alike): at alpha = 1e-4 an element stops moving once
    |w - ema| < 2^-24 |ema| / alpha, about 6e-4 |ema|."""

    COUNT_KEY = '.ema_updates'     # in state_dict()._metadata: no module path has an empty first component

    def __init__(self, model, decay=0.9999, warmup=True):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError('WeightEma: decay must lie in [0, 1], got %r' % (decay,))
        self.decay, self.warmup, self.updates = decay, bool(warmup), 0
        self._arena = self._barena = None          # the WeightArena / BufferArena the flat shadows are laid out for
        self._pflat = self._bflat = None
        self._shadow = {}                          # name -> shadow tensor (a view of a flat one where there is an arena)
        self._sync(model)

    def alpha(self, t=None):
        """Step weight of update number ``t`` (default: the next one), a Python float."""
        t = self.updates if t is None else t
        return 1.0 - (min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay)

    # ---------------------------------------------------------------------------------------------------------- layout
    def _sync(self, model):
        """Bring the shadows' layout in line with the model's: new names start as copies, known names keep their values."""
        from .path import BufferArena
        with torch.no_grad():
            st = getattr(model, '_retrain_state', None)
            arena = st.arena if st is not None and st.intact() else None
            params = dict(model.named_parameters())
            if arena is not None and set(arena.names) != set(params):
                arena = None
            relaid = False
            if arena is not self._arena or any(k not in self._shadow for k in params):
                relaid = True
                flat = None if arena is None else torch.zeros(arena.total, device=arena.device, dtype=torch.float32)
                for k, p in params.items():
                    if flat is not None:
                        o, n = arena.slot[id(p)]
                        new = flat[o:o + n].view(p.shape)
                    else:
                        new = torch.empty_like(p.data, memory_format=torch.contiguous_format)
                    new.copy_(self._shadow[k] if k in self._shadow else p.data)
                    self._shadow[k] = new
                self._arena, self._pflat = arena, flat
            bufs = dict(model.named_buffers())
            fb = {k: b for k, b in bufs.items() if b.is_floating_point()}
            ba = None
            if fb and all(b.is_cuda and b.dtype == torch.float32 for b in fb.values()) and len({b.device for b in fb.values()}) == 1:
                ba = getattr(model, '_buffer_arena', None)
                if ba is None or not ba.intact(model):
                    ba = BufferArena(model)
                    object.__setattr__(model, '_buffer_arena', ba)      # (like _retrain_state: stays out of state_dict)
            if ba is not self._barena or any(k not in self._shadow for k in bufs):
                relaid = True
                flat = None if ba is None else torch.zeros(ba.total, device=ba.device, dtype=torch.float32)
                for k, b in bufs.items():
                    if flat is not None and k in fb:
                        o, n = ba.slot[k]
                        new = flat[o:o + n].view(b.shape)
                    else:
                        new = torch.empty_like(b.data, memory_format=torch.contiguous_format)
                    new.copy_(self._shadow[k] if k in self._shadow else b.data)
                    self._shadow[k] = new
                self._barena, self._bflat = ba, flat
            if relaid:
                for k in [k for k in self._shadow if k not in params and k not in bufs]:
                    del self._shadow[k]
                sd = model.state_dict()
                self._keys = list(sd.keys())
                self._metadata = dict(getattr(sd, '_metadata', None) or {})
        return params, bufs

    def _pairs(self, model):
        """([live], [shadow]) over everything shadowed -- the flat tensors where both sides have one."""
        params, bufs = self._sync(model)
        live, shadow = [], []
        if self._pflat is not None:
            live.append(self._arena.w)
            shadow.append(self._pflat)
        else:
            live += [p.data for p in params.values()]
            shadow += [self._shadow[k] for k in params]
        for k, b in bufs.items():
            if self._bflat is None or not b.is_floating_point():
                live.append(b.data)
                shadow.append(self._shadow[k])
        if self._bflat is not None:
            live.append(self._barena.b)
            shadow.append(self._bflat)
        return live, shadow

    # --------------------------------------------------------------------------------------------------------- updates
    @staticmethod
    def _lerp_launch(shadow, live, alpha):
        """shadow <- fma(alpha, live - shadow, shadow) over two whole flat CUDA tensors: one launch."""
        import ctypes as C
        dev = shadow.device
        off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(shadow.numel())
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(_lib.lib().tfnas_ema_lerp(_lib.ptr(shadow), _lib.ptr(live), 1, off, ln, float(alpha), stream), 'tfnas_ema_lerp')

    def _update_buffers(self, bufs, alpha):
        """The buffers' share of one update: ONE launch for the floating-point ones where they are flat, a copy of the integers."""
        with torch.no_grad():
            fl = [k for k, b in bufs.items() if b.is_floating_point()]
            if self._bflat is not None:
                if self._bflat.numel():
                    self._lerp_launch(self._bflat, self._barena.b, alpha)
            elif fl:
                torch._foreach_lerp_([self._shadow[k] for k in fl], [bufs[k].data for k in fl], alpha)
            ints = [k for k, b in bufs.items() if not b.is_floating_point()]
            if ints:
                torch._foreach_copy_([self._shadow[k] for k in ints], [bufs[k].data for k in ints])

    def update(self, model):
        """The stand-alone update, after any optimizer's step: ``tfnas_ema_lerp`` over the weight arena and over the buffer tensor
        on a CUDA model that has them, ``torch._foreach_lerp_`` otherwise."""
        params, bufs = self._sync(model)
        alpha = self.alpha()
        with torch.no_grad():
            if self._pflat is not None:
                self._lerp_launch(self._pflat, self._arena.w, alpha)
            else:
                torch._foreach_lerp_([self._shadow[k] for k in params], [p.data for p in params.values()], alpha)
        self._update_buffers(bufs, alpha)
        self.updates += 1

    # ----------------------------------------------------------------------------------------------------------- state
    def state_dict(self):
        """The averaged network, keyed exactly like ``model.state_dict()`` (clones: it loads straight into a fresh ``NetworkCfg``
        and is what one deploys).  The update count travels in the dict's ``_metadata`` under ``COUNT_KEY``, where torch keeps the
        modules' versions: no tensor key is added, so ``load_state_dict(strict=True)`` of a model accepts it."""
        from collections import OrderedDict
        out = OrderedDict((k, self._shadow[k].detach().clone()) for k in self._keys)
        out._metadata = OrderedDict(self._metadata)
        out._metadata[self.COUNT_KEY] = {'updates': int(self.updates)}
        return out

    def load_state_dict(self, state, updates=None):
        """Values from a dict keyed like ``state_dict()`` (every key must be there); the update count from its ``_metadata``, or from
        ``updates`` (a checkpoint that stores it beside the dict)."""
        missing = [k for k in self._keys if k not in state]
        if missing:
            raise KeyError('WeightEma.load_state_dict: missing %s' % missing[:5])
        with torch.no_grad():
            for k in self._keys:
                self._shadow[k].copy_(state[k])
        meta = (getattr(state, '_metadata', None) or {}).get(self.COUNT_KEY)
        if updates is not None:
            self.updates = int(updates)
        elif meta is not None:
            self.updates = int(meta['updates'])

    def copy_to(self, model):
        """Overwrite the model's parameters and buffers with the averaged ones."""
        live, shadow = self._pairs(model)
        with torch.no_grad():
            for l, s in zip(live, shadow):
                l.copy_(s)

    def swapped(self, model):
        """Context manager: inside, the model holds the averaged values and the shadow holds the live ones (exchanged in place,
        plain torch copies -- the arenas' pointers stay what they are); they are exchanged back on exit, on an exception too."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            live, shadow = self._pairs(model)

            def exchange():
                with torch.no_grad():
                    for l, s in zip(live, shadow):
                        t = l.clone()
                        l.copy_(s)
                        s.copy_(t)
            exchange()
            try:
                yield model
            finally:
                exchange()
        return ctx()


def train_step(model, x, target, criterion, optimizer, grad_clip=5.0, group=None, fused=True, meter=None, ema=None):
    """One iteration of train_eval.py:228-252 (forward, label-smoothed loss, backward, clip, SGD); with a process group the
    gradients are averaged with ONE all-reduce of the flat gradient arena before clipping (one process per GPU instead of apex
    DDP).  ``fused`` (GPU models with a plain torch.optim.SGD): RetrainState -- gradient arena + tfnas_sgd_clip_step; otherwise
    torch's clip_grad_norm_ + optimizer.step().  Classifier + loss run on the fused retrain tail when ``FUSED_TAIL`` and
    ``fused_tail_eligible``; ``meter`` (a tail.DeviceMeter) collects loss / top-1 / top-5 of the step on the device.  ``ema`` (a
    WeightEma of this model): updated once per step -- inside the fused SGD pass, or with ``ema.update(model)`` after
    ``optimizer.step()`` on the torch route."""
    import torch.distributed as dist
    model.train()
    tail_plan = _fused_tail_plan(model, criterion) if FUSED_TAIL and x.is_cuda else None
    st = None
    plan = RetrainState.plan(optimizer, model) if fused and x.is_cuda else None
    if plan is not None:
        st = getattr(model, '_retrain_state', None)
        if st is None or not st.intact():
            st = RetrainState(model)
            object.__setattr__(model, '_retrain_state', st)         # (not a submodule / buffer: stays out of state_dict)
        st.begin()
    try:
        if tail_plan is not None:
            from .tail import RetrainTailFn
            core, eps = tail_plan
            lin = core.classifier.linear
            loss, logits, _ = RetrainTailFn.apply(core.features(x), lin.weight, lin.bias, target, eps, core.hip_modes, meter)
        else:
            logits = model(x)
            loss = criterion(logits, target)
            if meter is not None:
                meter.add(loss, logits, target)
        if st is None:
            optimizer.zero_grad()
        loss.backward()
    except BaseException:
        if st is not None:
            st.end()
        raise
    if st is not None:
        st.step(optimizer, grad_clip, group, ema, plan)
        return loss.detach(), logits.detach()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        dist.all_reduce(flat, group=group)
        flat.mul_(1.0 / dist.get_world_size(group))
        torch._foreach_copy_(grads, [v.view_as(g) for v, g in zip(flat.split([g.numel() for g in grads]), grads)])
    if grad_clip > 0:
        nn.utils.clip_grad_norm_(model.parameters(), grad_clip)
    optimizer.step()
    if ema is not None:
        ema.update(model)
    return loss.detach(), logits.detach()


def validate(model, val_queue, criterion=None, ema=None):
    """train_eval.py:271-293: eval mode (running statistics), top-1 / top-5 / loss.  ``ema`` (a WeightEma of this model): the
    averaged weights and statistics are evaluated -- exchanged into the model for the loop (``ema.swapped``) and out again."""
    if ema is not None:
        with ema.swapped(model):
            return _validate(model, val_queue, criterion)
    return _validate(model, val_queue, criterion)


def _validate(model, val_queue, criterion):
    from .tail import DeviceMeter, retrain_tail_forward
    model.eval()
    dev = next(model.parameters()).device
    tail_plan = _fused_tail_plan(model, criterion, validating=True) if FUSED_TAIL and dev.type == 'cuda' else None
    criterion = criterion or F.cross_entropy
    meter = DeviceMeter(dev)                                # ONE device -> host copy after the loop instead of one per batch
    for x, target in val_queue:
        x, target = x.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        with torch.no_grad():
            if tail_plan is not None:
                core, eps = tail_plan
                lin = core.classifier.linear
                retrain_tail_forward(core.features(x), lin.weight, lin.bias, target, eps, meter)
            else:
                logits = model(x)
                meter.add(criterion(logits, target), logits, target)
    obj, top1, top5, _, bad = meter.read()
    if bad:
        raise ValueError('validate: %d target(s) outside [0, num_classes)' % bad)
    return top1, top5, obj


def build_derived_network(num_classes, model_path=None, config_path=None, dropout_rate=0.2, drop_connect_rate=0.2):
    """train_eval.py:102-115: the derived network from a search checkpoint (``--model_path``: parse the architecture, widths
    from its masks) or from an exported ``model.config`` (``--config_path``)."""
    import json
    import os
    if model_path and os.path.isfile(model_path):
        from .epoch import get_op_and_depth_weights, parse_architecture
        ck = torch.load(model_path, map_location='cpu', weights_only=False)
        parsed = parse_architecture(*get_op_and_depth_weights(ck['state_dict']))
        return Network(num_classes, parsed, geometry.get_mc_num_dddict(ck['mc_mask_dddict']), None, dropout_rate,
                       drop_connect_rate)
    if config_path and os.path.isfile(config_path):
        return NetworkCfg(num_classes, json.load(open(config_path)), None, dropout_rate, drop_connect_rate)
    raise ValueError('invalid model_path and config_path')


def run_retrain(save_dir, model, make_train_queue, make_val_queue, *, epochs=250, lr=0.2, momentum=0.9, weight_decay=4e-5,
                label_smooth=0.1, grad_clip=5.0, batch_size=256, snapshot=None, device='cuda', group=None, log=print,
                ema_decay=None, ema_warmup=True, optimizer='sgd', no_decay=(), rmsprop_alpha=0.9, rmsprop_eps=1e-3, lr_at=None):
    """The retrain schedule of train_eval.py:118-226: SGD + cosine learning rate (5 warm-up epochs of linearly increasing rate
    when batch_size > 256), label-smoothed training loss, plain cross-entropy validation every epoch, ``checkpoint.pth.tar`` /
    ``model_best.pth.tar`` with the reference's keys ('epoch', 'state_dict' with DataParallel's ``module.`` prefix,
    'best_acc_top1', 'best_acc_top5', 'optimizer'), resume from ``snapshot``, ``model.config`` written next to them.

    ``ema_decay`` (None: nothing below happens, the checkpoints keep exactly those five keys): a ``WeightEma(model, ema_decay,
    ema_warmup)`` is updated at every step; each epoch validates the raw weights and the average (history rows gain
    ``val_top1_ema`` / ``val_top5_ema`` / ``val_obj_ema``, the log line shows both); ``best_acc_top1`` / ``top5`` and
    ``model_best.pth.tar`` follow the AVERAGE's top-1; checkpoints gain 'state_dict_ema' (``module.`` prefix, like 'state_dict')
    and 'ema_updates', which ``snapshot`` restores -- a snapshot without them starts the average from the loaded weights.

    ``optimizer`` ('sgd' | 'sgd-nesterov' | 'rmsprop' | 'rmsprop-tf'; the RMSprop ones with ``rmsprop_alpha`` / ``rmsprop_eps``,
    'rmsprop-tf' is ``optim.RMSpropTF``) and ``no_decay`` (() | any of 'bn', 'bias': those parameters form a second group without
    weight decay, ``optim.param_groups``) choose what the published recipes train with; every combination runs on the fused tail
    (``RetrainState.plan``).  ``lr_at`` (a callable epoch -> learning rate) replaces the cosine rule and its warm-up.  With none
    of the four passed, optimizer, schedule and checkpoint keys are what they always were."""
    import json
    import math
    import os
    import shutil
    from .tail import DeviceMeter
    os.makedirs(save_dir, exist_ok=True)
    dev = torch.device(device)
    model = model.to(dev)
    num_classes = model.classifier.out_features
    with open(os.path.join(save_dir, 'model.config'), 'w') as f:
        json.dump(model.config, f, indent=4)
    crit_smooth = CrossEntropyLabelSmooth(num_classes, label_smooth)
    if no_decay:
        from .optim import param_groups
        params = param_groups(model, weight_decay, no_decay)
    else:
        params = model.parameters()
    if optimizer in ('sgd', 'sgd-nesterov'):
        opt = torch.optim.SGD(params, lr, momentum=momentum, weight_decay=weight_decay, nesterov=optimizer == 'sgd-nesterov')
    elif optimizer == 'rmsprop':
        opt = torch.optim.RMSprop(params, lr, alpha=rmsprop_alpha, eps=rmsprop_eps, weight_decay=weight_decay, momentum=momentum)
    elif optimizer == 'rmsprop-tf':
        from .optim import RMSpropTF
        opt = RMSpropTF(params, lr, alpha=rmsprop_alpha, eps=rmsprop_eps, weight_decay=weight_decay, momentum=momentum)
    else:
        raise ValueError("run_retrain: optimizer is 'sgd', 'sgd-nesterov', 'rmsprop' or 'rmsprop-tf', got %r" % (optimizer,))
    best1 = best5 = 0.0
    start = 0
    if snapshot:
        ck = torch.load(snapshot, map_location=dev, weights_only=False)
        start, best1, best5 = ck['epoch'], ck['best_acc_top1'], ck['best_acc_top5']
        model.load_state_dict({k[len('module.'):] if k.startswith('module.') else k: v for k, v in ck['state_dict'].items()})
        opt.load_state_dict(ck['optimizer'])
    ema = None
    if ema_decay is not None:
        ema = WeightEma(model, ema_decay, ema_warmup)                   # (after the snapshot's weights are in: starts as their copy)
        if snapshot and 'state_dict_ema' in ck:
            ema.load_state_dict({k[len('module.'):] if k.startswith('module.') else k: v for k, v in ck['state_dict_ema'].items()},
                                updates=ck.get('ema_updates', 0))
    history = []
    meter = DeviceMeter(dev)
    for epoch in range(start, epochs):
        cur = 0.5 * lr * (1.0 + math.cos(math.pi * epoch / float(epochs)))          # CosineAnnealingLR(T_max=epochs).get_lr()
        warm = epoch < 5 and batch_size > 256
        if lr_at is not None:
            cur, warm = float(lr_at(epoch)), False
        for g in opt.param_groups:
            g['lr'] = cur * (epoch + 1) / 5.0 if warm else cur
        meter.reset()
        for x, y in make_train_queue(epoch):
            x, y = x.to(dev, non_blocking=True), y.to(dev, non_blocking=True)
            train_step(model, x, y, crit_smooth, opt, grad_clip, group, meter=meter, ema=ema)
        train_obj, train_acc, _, _, bad = meter.read()      # the epoch's only device -> host copy of the training loop
        if bad:
            raise ValueError('run_retrain: epoch %d saw %d training target(s) outside [0, %d)' % (epoch, bad, num_classes))
        v1, v5, vobj = validate(model, make_val_queue(epoch))
        if ema is not None:
            e1, e5, eobj = validate(model, make_val_queue(epoch), ema=ema)
        sel1, sel5 = (v1, v5) if ema is None else (e1, e5)
        is_best = sel1 > best1
        if is_best:
            best1, best5 = sel1, sel5
        state = {'epoch': epoch + 1, 'state_dict': {'module.' + k: v for k, v in model.state_dict().items()},
                 'best_acc_top1': best1, 'best_acc_top5': best5, 'optimizer': opt.state_dict()}
        if ema is not None:
            state['state_dict_ema'] = {'module.' + k: v for k, v in ema.state_dict().items()}
            state['ema_updates'] = ema.updates
        path = os.path.join(save_dir, 'checkpoint.pth.tar')
        torch.save(state, path)
        if is_best:
            shutil.copyfile(path, os.path.join(save_dir, 'model_best.pth.tar'))
        history.append(dict(epoch=epoch, lr=opt.param_groups[0]['lr'], train_acc=train_acc, train_obj=train_obj, val_top1=v1,
                            val_top5=v5, val_obj=vobj))
        if ema is None:
            log('Epoch %d lr %e train_acc %f val_top1 %f val_top5 %f' % (epoch, opt.param_groups[0]['lr'], train_acc, v1, v5))
        else:
            history[-1].update(val_top1_ema=e1, val_top5_ema=e5, val_obj_ema=eobj)
            log('Epoch %d lr %e train_acc %f val_top1 %f val_top5 %f ema_top1 %f ema_top5 %f' % (
                epoch, opt.param_groups[0]['lr'], train_acc, v1, v5, e1, e5))
    return history
