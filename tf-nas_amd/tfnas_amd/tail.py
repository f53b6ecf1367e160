"""Tail of a weight step: feature_mix_layer + global pooling + classifier + cross-entropy of BOTH bi-sampling paths, forward and
backward, on the two paths' own streams.

Reference: models/model_search.py:299-303 (``feature_mix_layer`` -> ``global_avg_pooling`` -> ``classifier``) evaluated for the
gumbel path and the random path (train_search.py:375-378), ``criterion`` = nn.CrossEntropyLoss (train_search.py:107) on each,
``loss = loss_g + loss_r; loss.backward()`` (:379-380).

Why it exists (round 6, `tools/trace_wstep.sh`): between the end of the cells' forward and the start of their backward NOTHING else is
on the chip, and rounds 1-5 ran both heads one after the other on one stream with the classifier / loss as ten stock torch launches
per path and the head's weight gradient in front of the cells' backward: ~1.4 ms of a 16.4 ms weight step for ~0.35 ms of work per
path.  Here path A's tail runs on the caller's stream and path B's on the side stream (concurrently), classifier + loss + their
gradients are ONE launch per path (tfnas_cls_ce) plus ONE for everything that sums over images and paths (tfnas_cls_wgrad), and the
weight gradients of the shared head / classifier parameters are leaves on the weight-gradient streams, written straight into the
WeightArena (no AccumulateGrad, no zero-fill + two adds).

Private to ``search._w_step_paths``: the backward of ``BiTailFn`` hands out gradients computed in its forward under the assumption
that the loss it returned is differentiated with gradient 1 -- ``loss.backward()``, which is what the weight step does.

Every route makes the same two launches (include/tfnas_hip.h): the per-image one (``_cls_ce``) and one that sums over images
(``_cls_wgrad`` for both paths of a weight step, tfnas_cls_reduce for one path).  The derived network's retrain path
(model_eval.train_step / validate; train_eval.py:228-293) reaches them through ``RetrainTailFn`` (label-smoothed loss, logits and
the target's rank, correct under any upstream gradient) and ``retrain_tail_forward`` (forward only).  An epoch's loss / top-1 /
top-5 sums stay on the device in ``MeterBlock``s, fed by the summation launches (by torch ops on the routes without one) and read
once: ``DeviceMeter`` (retrain) is one block, ``SearchMeter`` (train_search.py:318-432) two and the latency loss.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import TfnasCellDesc, check, ptr
from . import functions
from .functions import _nhwc, _on


class _PathTail:
    """Persistent buffers + descriptors of ONE path's tail at one geometry."""

    def __init__(self, plan, N, H, W, K, dev, own_grad):
        lib = _lib.lib()
        d0, ws = plan.desc(N, H, W)
        self.ws = ws
        # two private copies of the planned descriptor: without / with the weight-gradient binding
        self.d = TfnasCellDesc.from_buffer_copy(d0)
        self.dw = TfnasCellDesc.from_buffer_copy(d0)
        f32, f64 = torch.float32, torch.float64
        M, mc = d0.M, d0.g[0].mc
        piece, slots = int(lib.tfnas_sizeof(7)), int(lib.tfnas_sizeof(8))
        npart = -(-int(ws.part) // piece) * piece

        def part():
            b = torch.empty(npart, device=dev, dtype=f32)
            b.view(-1, piece)[:, piece - slots:].zero_()
            return b
        self.E = torch.empty(int(ws.E), device=dev, dtype=f32)
        self.dEh = torch.empty(int(ws.dEh), device=dev, dtype=f32)
        self.stats = torch.empty(2 * M, device=dev, dtype=f64)
        self.red = torch.empty(2 * M, device=dev, dtype=f64)
        self.cb1 = torch.empty(4 * M, device=dev, dtype=f32)
        self.part, self.part_w = part(), part()
        self.pooled = torch.empty((N, mc), device=dev, dtype=f32)
        self.dpooled = torch.empty((N, mc), device=dev, dtype=f32)
        self.dx = torch.empty((N, H, W, plan.ic), device=dev, dtype=f32)
        self.dxp = torch.empty(int(ws.dxp), device=dev, dtype=f32)
        self.dlogits = torch.empty((N, K), device=dev, dtype=f32)
        self.logits = torch.empty((N, K), device=dev, dtype=f32)          # (path B's logits: nobody reads them)
        self.loss_n = torch.empty(N, device=dev, dtype=f32)
        self.rank = torch.empty(N, device=dev, dtype=torch.int32)        # (path A with a meter: the target's rank)
        self.gw = torch.empty(mc * plan.ic, device=dev, dtype=f32) if own_grad else None     # path B's share of d W_feature_mix


class BiTail:
    """Owned by a SearchState; rebuilt when the geometry or the parameter storages change."""

    def __init__(self, state):
        self.state = state
        self._key = None
        self.a = self.b = None

    def _prepare(self, model, N, H, W, dev):
        fm, lin = model.feature_mix_layer, model.classifier.linear
        plan = model.head_plan()
        arena = self.state.arena
        key = (N, H, W, fm.conv.weight.data_ptr(), lin.weight.data_ptr(), arena.g.data_ptr(), lin.out_features)
        if key == self._key:
            return
        for p in (fm.conv.weight, lin.weight, lin.bias):
            if p is None or not arena.owns(p):
                raise RuntimeError('tfnas_amd: the fused step tail needs the head / classifier parameters in the WeightArena')
        K = lin.out_features
        self.a = _PathTail(plan, N, H, W, K, dev, False)
        self.b = _PathTail(plan, N, H, W, K, dev, True)
        self.loss = torch.zeros((), device=dev, dtype=torch.float32)
        self._key = key

    def run(self, model, oa, ob, target, side, wgrad_streams, meter=None):
        """Enqueue both tails; returns (loss 0-dim tensor, logits of path A, d oa, d ob) -- NHWC gradient buffers.
        ``meter`` (a SearchMeter): path A's per-image launch becomes tfnas_cls_ce_ex(eps = 0) -- bit-identical outputs plus the
        target's rank -- and the summation launch tfnas_cls_wgrad_ex, which adds the step to the meter's w block; no launch more."""
        lib = _lib.lib()
        xa, xb = _nhwc(oa), _nhwc(ob)
        dev = xa.device
        N, H, W, _ = xa.shape
        self._prepare(model, N, H, W, dev)
        fm, lin = model.feature_mix_layer, model.classifier.linear
        arena = self.state.arena
        K, Cf = lin.out_features, lin.in_features
        cur = torch.cuda.current_stream(dev)
        t64 = _int64(target)
        if t64 is not target:
            side.wait_stream(cur)                        # (made on the current stream just now; path B reads it on `side`)
            t64.record_stream(side)
        wsa, wsb = (wgrad_streams + [None, None])[:2] if wgrad_streams else (None, None)
        logits = [torch.empty((N, K), device=dev, dtype=torch.float32), self.b.logits]
        w_fm, w_cls, b_cls = fm.conv.weight, lin.weight, lin.bias
        with _on(dev):
            for t, x, st, wst, lg, gdst in ((self.a, xa, cur, wsa, logits[0], arena.grad_ptr(w_fm)),
                                            (self.b, xb, side, wsb, logits[1], self.b.gw.data_ptr())):
                s = C.c_void_p(st.cuda_stream)
                for d in (t.d, t.dw):
                    model.hip_modes.apply(d)
                    d.g[0].w_expand = w_fm.data_ptr()
                t.d.need_wgrad, t.d.g[0].g_expand = 0, None
                t.dw.need_wgrad, t.dw.g[0].g_expand = 1, gdst
                check(lib.tfnas_head_fwd(C.byref(t.d), ptr(x), ptr(t.E), ptr(t.stats), ptr(t.part), ptr(t.pooled), s), 'tfnas_head_fwd')
                _cls_ce(t.pooled, w_cls, b_cls, t64, s, rank=meter is not None and t is self.a,
                        out=dict(logits=lg, loss_n=t.loss_n, rank=t.rank, dlogits=t.dlogits, dpooled=t.dpooled))
                check(lib.tfnas_head_bwd(C.byref(t.d), ptr(x), ptr(t.E), ptr(t.stats), ptr(t.dpooled), ptr(t.dEh), ptr(t.cb1),
                                         ptr(t.red), ptr(t.part), ptr(t.dx), ptr(t.dxp), s), 'tfnas_head_bwd')
                # the head's weight gradient: a leaf, on the path's weight-gradient stream (joined by tfnas_paths_bwd / w_step)
                w = wst if wst is not None else st
                if w is not st:
                    w.wait_stream(st)
                check(lib.tfnas_head_wgrad(C.byref(t.dw), ptr(x), ptr(t.E), ptr(t.dEh), ptr(t.cb1), ptr(t.part_w),
                                           C.c_void_p(w.cuda_stream)), 'tfnas_head_wgrad')
            # what sums over both paths: classifier gradients + the loss scalar, and path B's share of d W_feature_mix
            w = wsa if wsa is not None else cur
            for other in (cur, side, wsb):
                if other is not None and other is not w:
                    w.wait_stream(other)
            _cls_wgrad((self.a, self.b), N, Cf, K, C.c_void_p(arena.grad_ptr(w_cls)), C.c_void_p(arena.grad_ptr(b_cls)), self.loss,
                       C.c_void_p(w.cuda_stream), None if meter is None else meter.w.ptr(dev))
            check(lib.tfnas_add_into(C.c_void_p(arena.grad_ptr(w_fm)), ptr(self.b.gw), w_fm.numel(), C.c_void_p(w.cuda_stream)),
                  'tfnas_add_into')
        self.join_stream = w if w is not cur else None
        return self.loss, logits[0], self.a.dx, self.b.dx


class BiTailFn(torch.autograd.Function):
    """(loss, logits_g) = CE(classifier(head(oa))) + CE(classifier(head(ob))); see the module docstring for the contract."""

    @staticmethod
    def forward(ctx, tail, model, oa, ob, target, side, wgrad_streams, meter=None):
        loss, logits, dxa, dxb = tail.run(model, oa, ob, target, side, wgrad_streams, meter)
        ctx.dxa, ctx.dxb = dxa, dxb
        ctx.mark_non_differentiable(logits)
        # (a fresh 0-dim tensor per step: the persistent one is overwritten by the next step)
        out = loss.clone() if tail.join_stream is None else _clone_on(loss, tail.join_stream)
        return out, logits

    @staticmethod
    def backward(ctx, gloss, glogits):
        return None, None, ctx.dxa.permute(0, 3, 1, 2), ctx.dxb.permute(0, 3, 1, 2), None, None, None, None


class ClsCeFn(torch.autograd.Function):
    """(loss, logits) = cross_entropy(linear(pooled, W, b), target), mean reduction, for FROZEN classifier weights (the architecture
    step, ``validate``): ONE launch forward (tfnas_cls_ce: logits, per-image loss, d logits, d pooled) + a 128-element sum, one
    scaling launch backward -- instead of eight stock torch launches (GEMM, log-softmax, nll and their backward kernels).
    Reference: models/model_search.py:301-303 + train_search.py:107,410.
    ``meter`` (a SearchMeter): the launch is tfnas_cls_ce_ex(eps = 0) -- bit-identical outputs plus the target's rank -- followed by
    one metrics-only tfnas_cls_reduce into the meter's a block: loss sum, top-1 / top-5, images, invalid targets."""

    @staticmethod
    def forward(ctx, pooled, W, b, target, meter=None):
        dev, N = pooled.device, pooled.size(0)
        s = functions._stream(dev)
        _, logits, loss_n, rank, _, dpooled = _cls_ce(pooled, W, b, target, s, rank=meter is not None)
        if meter is not None:
            _cls_metrics(loss_n, rank, W.shape[0], meter.a.ptr(dev), s, want_out=False)
        ctx.save_for_backward(dpooled)
        ctx.mark_non_differentiable(logits)
        return loss_n.sum() * (1.0 / N), logits

    @staticmethod
    def backward(ctx, gloss, glogits):
        dpooled, = ctx.saved_tensors
        return dpooled * gloss, None, None, None, None


def frozen_classifier_loss(model, pooled, target, meter=None):
    """loss, logits through ClsCeFn when the classifier's parameters are frozen CUDA fp32 tensors; None otherwise (then nothing
    was added to ``meter`` either)."""
    lin = getattr(getattr(model, 'classifier', None), 'linear', None)
    if lin is None or lin.bias is None or lin.weight.requires_grad or lin.bias.requires_grad or not pooled.is_cuda:
        return None
    # (the limits of the launch, stated once: for C, K <= 4096 the LDS term of cls_shapes_ok never binds -- C + K + KG * C is at most
    # 3 * 4096 floats, 48 KiB -- so this is the C % 4, C <= 4096, K <= 4096 this function has always asked for)
    if lin.weight.dtype != torch.float32 or not cls_shapes_ok(lin.in_features, lin.out_features):
        return None
    return ClsCeFn.apply(pooled, lin.weight.detach(), lin.bias.detach(), target, meter)


def cls_shapes_ok(Cf, K):
    """The limits of tfnas_cls_ce / tfnas_cls_ce_ex (include/tfnas_hip.h): C % 4 == 0, 4 <= C <= 4096, K <= 4096, LDS <= 64 KiB."""
    if Cf < 4 or (Cf & 3) or Cf > 4096 or K < 1 or K > 4096:
        return False
    kg = max(1, min(8, K, 1024 // (Cf >> 2)))
    return 4 * (Cf + ((K + 3) & ~3) + kg * Cf) <= 64 * 1024


def _int64(target):
    """The targets as the kernels read them: contiguous int64 (the same tensor when they already are)."""
    return target if target.dtype == torch.int64 and target.is_contiguous() else target.long().contiguous()


def _cls_ce(pooled, W, b, target, stream, eps=0.0, rank=False, grads=True, out=None):
    """THE per-image launch, on ``stream`` (a launch pointer) -> (pooled, logits, loss_n, rank, dlogits, dpooled), into the buffers of
    ``out`` (by those names) where it has them and fresh ones otherwise.  tfnas_cls_ce unless something only tfnas_cls_ce_ex has is
    asked for -- the target's ``rank``, ``eps`` != 0, or the forward-only form (``grads`` False: no dlogits / dpooled) -- so a step
    without a meter launches what it always did, and an invalid target there gives loss 0, not NaN.  Without ``rank`` the
    returned rank is None.  dlogits carries the 1 / N of the mean reduction."""
    pooled, target = pooled.contiguous(), _int64(target)
    (N, Cf), K, dev = pooled.shape, W.shape[0], pooled.device
    ex = bool(rank) or eps != 0 or not grads
    out = out or {}

    def buf(name, shape, dtype=torch.float32):
        t = out.get(name)
        return torch.empty(shape, device=dev, dtype=dtype) if t is None else t
    logits, loss_n = buf('logits', (N, K)), buf('loss_n', N)
    rk = buf('rank', N, torch.int32) if ex else None
    dlogits, dpooled = (buf('dlogits', (N, K)), buf('dpooled', (N, Cf))) if grads else (None, None)
    lib = _lib.lib()
    with _on(dev):
        if ex:
            check(lib.tfnas_cls_ce_ex(N, Cf, K, ptr(pooled), ptr(W), ptr(b), ptr(target), 1.0 / N, float(eps), ptr(logits),
                                      ptr(loss_n), ptr(rk), ptr(dlogits), ptr(dpooled), stream), 'tfnas_cls_ce_ex')
        else:
            check(lib.tfnas_cls_ce(N, Cf, K, ptr(pooled), ptr(W), ptr(b), ptr(target), 1.0 / N, ptr(logits), ptr(loss_n),
                                   ptr(dlogits), ptr(dpooled), stream), 'tfnas_cls_ce')
    return pooled, logits, loss_n, rk, dlogits, dpooled


def _cls_wgrad(paths, N, Cf, K, dW, db, loss, stream, meter=None):
    """THE summation launch of a weight step over ``paths`` (_PathTail): tfnas_cls_wgrad, or with ``meter`` (a launch pointer to
    a meter block) tfnas_cls_wgrad_ex with the rank of paths[0].  dW / db / stream are launch pointers."""
    lib = _lib.lib()
    P = lambda name: _lib.raw_array([getattr(t, name).data_ptr() for t in paths])
    head = (len(paths), N, Cf, K, P('pooled'), P('dlogits'), P('loss_n'))
    if meter is None:
        check(lib.tfnas_cls_wgrad(*head, 1.0 / N, dW, db, ptr(loss), stream), 'tfnas_cls_wgrad')
    else:
        check(lib.tfnas_cls_wgrad_ex(*head, ptr(paths[0].rank), 1.0 / N, dW, db, ptr(loss), meter, stream), 'tfnas_cls_wgrad_ex')


def _cls_metrics(loss_n, rank, K, meter, stream, want_out=True):
    """The metrics-only tfnas_cls_reduce: out[4] = {mean loss, top-1 count, top-5 count, invalid count} (returned; None without
    ``want_out``), and the sums of ``meter`` (a launch pointer to a meter block, or None)."""
    dev = loss_n.device
    out = torch.empty(4, device=dev, dtype=torch.float32) if want_out else None
    with _on(dev):
        check(_lib.lib().tfnas_cls_reduce(loss_n.numel(), 4, K, None, None, ptr(loss_n), ptr(rank), None, 0, None, None, ptr(out),
                                          meter, stream), 'tfnas_cls_reduce')
    return out


def target_rank(logits, target):
    """(rank, valid) of every row's target by the rule of tfnas_cls_ce_ex (include/tfnas_hip.h), as torch ops on any device:
    rank = #{k: l_k > l_t} + #{k < t: l_k == l_t} -- ties go to the lower class index, where torch.topk promises no order -- and
    -1 where the target is outside [0, K).  Nothing is indexed by an invalid target."""
    K = logits.size(1)
    t = target.view(-1, 1).long()
    valid = (t >= 0) & (t < K)
    lt = logits.gather(1, t.clamp(0, K - 1))
    ks = torch.arange(K, device=logits.device).view(1, -1)
    rank = ((logits > lt) | ((logits == lt) & (ks < t))).sum(1, keepdim=True)
    return torch.where(valid, rank, torch.full_like(rank, -1)).view(-1), valid.view(-1)


class MeterBlock:
    """THE meter layout of include/tfnas_hip.h -- five doubles {sum of per-image losses, top-1 hits, top-5 hits, images, invalid
    targets} -- on ``buf[first:first + 5]`` of its owner's buffer: what a launch adds to (``ptr``), the same sums as torch ops
    (``add``) and the averages of five host numbers (``averages``).  Nothing here synchronises with the host."""

    def __init__(self, buf, first=0):
        self.buf = buf[first:first + 5]                  # (a view: the owner zeroes, reduces and reads the whole buffer)

    def ptr(self, dev):
        """The block as a launch argument of a step on ``dev``."""
        if self.buf.device != dev:
            raise RuntimeError('tfnas_amd: the meter lives on %s, the step runs on %s' % (self.buf.device, dev))
        return C.c_void_p(self.buf.data_ptr())

    def add(self, loss, n, logits=None, target=None):
        """What the fused tails add, from a mean loss over ``n`` images and -- for the hits and the invalid count, by
        ``target_rank`` -- logits and targets."""
        f64 = torch.float64
        s = loss.detach().to(f64) * n
        cnt = torch.full((), float(n), dtype=f64, device=s.device)
        if logits is None:
            vals = [s, torch.zeros_like(s), torch.zeros_like(s), cnt]
        else:
            rank, valid = target_rank(logits.detach(), target)
            vals = [s, (valid & (rank < 1)).sum().to(f64), (valid & (rank < 5)).sum().to(f64), cnt, (~valid).sum().to(f64)]
        self.buf[:len(vals)].add_(torch.stack(vals))

    @staticmethod
    def averages(v):
        """(loss average, top-1 %, top-5 %, images, invalid targets) of a block's five numbers on the host; zeros when empty."""
        s, c1, c5, cnt, bad = v
        n = cnt or 1.0
        return s / n, 100.0 * c1 / n, 100.0 * c5 / n, int(cnt), int(bad)


class DeviceMeter:
    """An epoch's running sums of the retrain path as ONE MeterBlock on the device: the retrain tail's reduction launch adds to it
    (tfnas_cls_reduce), the torch route adds with torch ops (``add``), and ``read`` is the only device -> host copy -- once per
    epoch instead of a ``.tolist()`` per step (train_eval.py:246-250,287-291 keep AverageMeters on the host).  Every update is
    enqueued on the caller's current stream."""

    def __init__(self, device):
        self.buf = torch.zeros(5, device=device, dtype=torch.float64)
        self.block = MeterBlock(self.buf)

    def reset(self):
        self.buf.zero_()

    def add(self, loss, logits, target):
        """What the fused tail adds, from a mean loss and logits computed by torch ops (no host sync either).  Hits are counted by
        ``target_rank`` -- the kernels' tie rule: a target logit exactly tied with another class's is a hit only against higher
        class indices, where torch.topk promised no order -- and the fifth slot counts the targets outside [0, K)."""
        self.block.add(loss, target.size(0), logits, target)

    def read(self):
        """(loss average, top-1 %, top-5 %, images, invalid targets)"""
        return MeterBlock.averages(self.buf.tolist())


class SearchMeter:
    """A search epoch's running sums (train_search.py:318-432: the AverageMeters objs_w, top1, top5, objs_a, objs_l) as eleven
    doubles ON THE DEVICE: two MeterBlocks -- ``w`` for the weight steps (loss = loss_g + loss_r, hits of the gumbel path), ``a``
    for the architecture steps -- and sum n * loss_l.  The fused tails add to the blocks from their own launches
    (tfnas_cls_wgrad_ex, tfnas_cls_reduce); ``add_w`` / ``add_a`` are the same sums as torch ops for the routes without a fused
    tail and for host tensors.  Nothing here synchronises with the host except ``read``.  Updates are ordered by the steps'
    streams: every step joins its side streams into the caller's stream before it returns."""
    W, A, L, SIZE = 0, 5, 10, 11

    def __init__(self, device):
        self.buf = torch.zeros(self.SIZE, device=device, dtype=torch.float64)
        self.w, self.a = MeterBlock(self.buf, self.W), MeterBlock(self.buf, self.A)

    def reset(self):
        self.buf.zero_()

    def add_w(self, loss, logits, target):
        """One weight step from its returned mean loss (both paths' sum under bi-sampling) and the gumbel path's logits."""
        self.w.add(loss, target.size(0), logits, target)

    def add_a(self, loss_a, loss_l, n, logits=None, target=None):
        """One architecture step: n * loss_l always; n * loss_a, the images and -- with logits / target -- the hits unless
        ``loss_a`` is None (the fused classifier tail has added its block from its own launch)."""
        if loss_a is not None:
            self.a.add(loss_a, n, logits, target)
        self.buf[self.L:self.L + 1].add_(loss_l.detach().to(torch.float64).view(1) * n)

    def reduce_(self, group=None):
        """Sum the buffer over the ranks of ``group`` with one all-reduce (nothing when not distributed)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.buf, op=dist.ReduceOp.SUM, group=group)

    def read(self):
        """The only device -> host copy: the reference's averages (losses per image, top-k in percent) and the counts."""
        v = self.buf.tolist()
        w, a = MeterBlock.averages(v[self.W:self.W + 5]), MeterBlock.averages(v[self.A:self.A + 5])
        return dict(objs_w=w[0], top1=w[1], top5=w[2], images_w=w[3], objs_a=a[0], objs_l=v[self.L] / (a[3] or 1.0), top1_a=a[1],
                    top5_a=a[2], images_a=a[3], invalid=w[4] + a[4])


def retrain_tail_forward(pooled, W, b, target, eps=0.0, meter=None):
    """(loss, logits, rank) without gradients: the forward-only kernel (no d logits / d pooled phase) + the metrics launch."""
    s = functions._stream(pooled.device)
    _, logits, loss_n, rank, _, _ = _cls_ce(pooled, W, b, target, s, eps, rank=True, grads=False)
    out = _cls_metrics(loss_n, rank, W.shape[0], meter and meter.block.ptr(pooled.device), s)
    return out[0], logits, rank


class RetrainTailFn(torch.autograd.Function):
    """(loss, logits, rank) = f(pooled, W, b, target, eps[, modes, meter]): classifier + label-smoothed cross-entropy (mean
    reduction; train_eval.py:72-85 with num_classes == K) + the target's rank (top-k is ``rank < k``; ties go to the lower class
    index, -1 marks a target outside [0, K), whose loss is NaN and whose gradient rows are zero) -- include/tfnas_hip.h:
    tfnas_cls_ce_ex / tfnas_cls_reduce.  Forward: the per-image launch + the metrics launch (which feeds ``meter``, a DeviceMeter).
    Backward, correct for ANY upstream d loss with no host read: the weight-gradient launch takes it as a device scalar, d pooled
    is scaled by it.  ``modes`` (a functions.HipModes, default functions.DEFAULT_MODES) is honoured like MBConvAffineFn does: with
    ``direct_grads`` and usable ``.grad`` views dW / db are written in place and None is returned for them; with ``lazy_join`` as
    well that launch rides the weight-gradient side stream (joined once per step by RetrainState).  logits and rank carry no
    gradient."""

    @staticmethod
    def forward(ctx, pooled, W, b, target, eps, modes=None, meter=None):
        modes = functions.DEFAULT_MODES if modes is None else modes
        s = functions._stream(pooled.device)
        pooled, logits, loss_n, rank, dlogits, dpooled = _cls_ce(pooled, W, b, target, s, eps, rank=True)
        out = _cls_metrics(loss_n, rank, W.shape[0], meter and meter.block.ptr(pooled.device), s)
        ctx.modes = modes
        ctx.direct = functions._direct_targets([W, b], modes) if W.requires_grad and b.requires_grad else None
        ctx.save_for_backward(pooled, dlogits, dpooled, loss_n, rank, W, b)
        ctx.mark_non_differentiable(logits, rank)
        return out[0], logits, rank

    @staticmethod
    def backward(ctx, gloss, glogits, grank):
        pooled, dlogits, dpooled, loss_n, rank, W, b = ctx.saved_tensors
        dev = pooled.device
        N, Cf = pooled.shape
        K = W.shape[0]
        gs = gloss.to(torch.float32).contiguous()
        gW = gb = None
        direct = ctx.direct
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            if direct is not None:
                gW, gb = direct
            else:
                gW, gb = torch.empty_like(W), torch.empty_like(b)
            side = functions._side_stream(dev) if ctx.modes.lazy_join and direct is not None else None
            if side is not None:
                side.wait_stream(torch.cuda.current_stream(dev))
            stream = functions._stream(dev) if side is None else C.c_void_p(side.cuda_stream)
            with _on(dev):
                check(_lib.lib().tfnas_cls_reduce(N, Cf, K, ptr(pooled), ptr(dlogits), ptr(loss_n), ptr(rank), ptr(gs), 0, ptr(gW),
                                                  ptr(gb), None, None, stream), 'tfnas_cls_reduce')
            if side is not None:                 # the launch still reads these when this function returns
                for t in (pooled, dlogits, loss_n, rank, gs):
                    t.record_stream(side)
            if direct is not None:
                gW = gb = None
        dpo = dpooled * gs if ctx.needs_input_grad[0] else None
        return (dpo, gW if ctx.needs_input_grad[1] else None, gb if ctx.needs_input_grad[2] else None, None, None, None, None)


def _clone_on(t, stream):
    with torch.cuda.stream(stream):
        c = t.clone()
    c.record_stream(torch.cuda.current_stream(t.device))
    return c
