"""Path-level execution of the supernet: all 18 MixedOP cells + 6 sink-connecting stage mixes of a forward (or backward)
in ONE call into the HIP library (include/tfnas_hip.h: tfnas_path_*), instead of one Python / autograd round trip per cell.

What it replaces in the reference: the stage loop of ``Network.forward`` (models/model_search.py:285-297) with the six
``MixedStage.forward`` calls (:157-206) and their autograd backward, as driven by train_search.py:375-379 (the two
bi-sampling paths of the weight step), :409 (the soft architecture step), :333 / :447 (single gumbel path of
``train_wo_arch`` / ``validate``).  The module API of model_search.py stays as it is (``model(x, sampling, mode)`` still
walks the cells one by one); ``tfnas_amd.search`` uses this runner for its steps.

Pieces:
  WeightArena   every weight parameter of the network as a view into ONE flat fp32 buffer, with a gradient buffer and an
                SGD-momentum buffer at identical offsets.  The cells' weight-gradient kernels write straight into the
                gradient buffer (no per-tensor allocations, no AccumulateGrad), one candidate's parameters are one
                contiguous range (one all-reduce bucket entry / one range of the fused clip+SGD kernel).
  PathRunner    descriptor templates per (cell, candidate), arenas, C contexts; autograd Functions SoftPathFn / BiPathFn /
                OnePathFn whose forward / backward are one C call each.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import TfnasCellDesc, TfnasPathDesc, TfnasPathWs, check, ptr, raw_array
from .functions import EFREE, EFREE_STRIDE1, _nhwc, _on, _require_cuda, fill_cell_desc, fill_pass_desc

ALIGN = 64          # floats; every parameter starts on a 256-byte boundary of the arenas


def _is_arch(name):
    return name.endswith('log_alphas') or name.endswith('betas')


class WeightArena:
    """Flat storage of all weight parameters (``w``), their gradients (``g``) and SGD momentum (``m``).

    ``p.data`` of every weight parameter becomes a view into ``w`` (values preserved, ``state_dict`` / ``load_state_dict``
    / optimizers keep working on the same Parameter objects).  Offsets follow ``named_parameters()`` order, so the 3 or 7
    tensors of one MBConv candidate are adjacent: ``block_range`` gives that range.  The gaps that align each tensor to
    256 bytes are zero in all three buffers and stay zero under every update."""

    def __init__(self, model):
        named = [(k, p) for k, p in model.named_parameters() if not _is_arch(k)]
        if not named:
            raise ValueError('model has no weight parameters')
        dev = named[0][1].device
        self.device = dev
        self.names, self.params, self.slot = [], [], {}
        off = 0
        for k, p in named:
            _require_cuda(p, 'weight parameter %s' % k)
            n = p.numel()
            self.slot[id(p)] = (off, n)
            self.names.append(k)
            self.params.append(p)
            off += (n + ALIGN - 1) // ALIGN * ALIGN
        self.total = off
        self.w = torch.zeros(off, device=dev, dtype=torch.float32)
        self.g = torch.zeros(off, device=dev, dtype=torch.float32)
        self.m = torch.zeros(off, device=dev, dtype=torch.float32)
        self._gview = {}
        with torch.no_grad():
            for p in self.params:
                o, n = self.slot[id(p)]
                v = self.w[o:o + n].view(p.shape)
                v.copy_(p.data)
                p.data = v
                self._gview[id(p)] = self.g[o:o + n].view(p.shape)
        self._base = self.w.data_ptr()

    def owns(self, p):
        s = self.slot.get(id(p))
        return s is not None and p.data_ptr() == self._base + 4 * s[0]

    def intact(self):
        """False once somebody replaced a parameter's storage (``p.data = ...`` of another tensor, ``model.to()``):
        the reference does that at every epoch boundary (train_search.py:164-193) -- build a new arena then."""
        return all(self.owns(p) for p in self.params)

    def grad_view(self, p):
        return self._gview[id(p)]

    def grad_ptr(self, p):
        return self.g.data_ptr() + 4 * self.slot[id(p)][0]

    def span(self, params):
        """(offset, length) of the smallest range covering ``params`` (which must be adjacent in the arena); no parameters (a skip
        candidate): the empty range (0, 0)."""
        if not params:
            return 0, 0
        offs = [self.slot[id(p)] for p in params]
        lo = min(o for o, _ in offs)
        hi = max(o + (n + ALIGN - 1) // ALIGN * ALIGN for o, n in offs)
        covered = sum((n + ALIGN - 1) // ALIGN * ALIGN for _, n in offs)
        if covered != hi - lo:
            raise ValueError('parameters are not adjacent in the arena')
        return lo, hi - lo


class BufferArena:
    """Flat storage of a model's floating-point buffers (the BatchNorm running statistics), as WeightArena is of its parameters:
    ``buf.data`` of every fp32 buffer becomes a view into ``b`` (values preserved, ``state_dict`` / ``load_state_dict`` keep
    working, the kernels that update the statistics are handed the views' pointers at every call).  Built only where something
    wants all buffers in ONE launch -- model_eval.WeightEma.  Slots are keyed by NAME: ``model.to()`` replaces the buffer
    objects themselves.  The aligning gaps are zero and stay zero."""

    def __init__(self, model):
        named = [(k, b) for k, b in model.named_buffers() if b.is_floating_point()]
        self.slot = {}
        off = 0
        for k, b in named:
            _require_cuda(b, 'buffer %s' % k)
            self.slot[k] = (off, b.numel())
            off += (b.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.total = off
        self.device = named[0][1].device if named else None
        self.b = torch.zeros(off, device=self.device, dtype=torch.float32)
        with torch.no_grad():
            for k, b in named:
                o, n = self.slot[k]
                v = self.b[o:o + n].view(b.shape)
                v.copy_(b.data)
                b.data = v
        self._base = self.b.data_ptr()

    def intact(self, model):
        seen = 0
        for k, b in model.named_buffers():
            if b.is_floating_point():
                s = self.slot.get(k)
                if s is None or b.numel() != s[1] or b.data_ptr() != self._base + 4 * s[0]:
                    return False
                seen += 1
        return seen == len(self.slot)


class _Slot:
    """One concurrently running path: C context + descriptor + arena."""

    def __init__(self, lib):
        self.ctx = C.c_void_p()
        check(lib.tfnas_path_create(C.byref(self.ctx)), 'tfnas_path_create')
        self.pd = TfnasPathDesc()
        self.ws = TfnasPathWs()
        self.arena = None
        self.gen = 0
        self.dbetas = None


class PathRunner:
    def __init__(self, model, weights=None):
        self.lib = _lib.lib()                       # (no reference to the model itself: cells / stages are enough)
        self.cells = model.cells()
        self.stages = model.stages()
        self.weights = weights                      # WeightArena or None (then need_wgrad paths are refused)
        self._slots = {}
        self._tmpl = {}
        self._tmeta = {}
        self._wide = {}                             # input shape -> per cell the candidate with the largest planned workspace
        self.wgrad_streams = {}                     # slot name -> torch stream for that path's weight-gradient kernels
        self.segment_hook = None                    # callable(cur_stream, side_stream) between the two backward segments
        self.split_stage = 3                        # stages [3, 6) = stage4..stage6 hold 89 % of the parameters
        self.device = next(model.parameters()).device
        # TfnasPathDesc.path_flags: a network with candidates beside the plain ones says so (a plain network's paths are what they
        # always were)
        self.path_flags = 0 if getattr(model, 'plain_candidates', lambda: True)() else _lib.PATH_EXTENDED
        nres = [st.num_res for st in self.stages]
        self.nres_total = sum(nres)
        # stage-expanded latency layout: per stage its nres entries, a leading 0 where the stage input is a depth choice
        idx, c = [], 0
        for st in self.stages:
            if st.start_res == 0:
                idx.append(0)
            for _ in range(st.nblocks):
                idx.append(1 + c)
                c += 1
        self._lat_index = torch.tensor(idx, dtype=torch.long, device=self.device)

    def close(self, streams=()):
        """Destroy the C contexts (tfnas_path_destroy waits for the context's side stream) and drop the arenas.  ``streams``: torch
        streams that may still run kernels on the arenas -- the caching allocator then defers their reuse (record_stream) instead
        of the caller synchronising the device."""
        for s in self._slots.values():
            if s.arena is not None and s.arena.is_cuda:
                for st in streams:
                    s.arena.record_stream(st)
            self.lib.tfnas_path_destroy(s.ctx)
            s.ctx = None                            # a backward that still holds this slot must raise (_check_gen), not pass
            s.gen += 1                              # a freed context to tfnas_paths_bwd
            s.arena = None
        self._slots = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- descriptor templates ---------------------------------------------------------------------------------
    def _template(self, ci, idx, N, H, W):
        """Planned TfnasCellDesc of cell ``ci`` with candidate ``idx`` (None: all 8), weight / gradient pointers bound: the cell's
        own CellPlan (the per-cell route's: MixedOP._plan) filled by functions.fill_cell_desc -- every kind, packed and dilated
        groups, skip groups.  A sampled skip is the pass-through descriptor (functions.fill_pass_desc): no plan, no pointers."""
        return self._template_entry(ci, idx, N, H, W)[0]

    def _template_entry(self, ci, idx, N, H, W):
        """(descriptor, gradient pointers are bound); ``_tmpl`` maps the key to the descriptor, ``_tmeta`` to (data pointer of the
        first bound weight, gradient pointers are bound, the plan that filled it)"""
        cell = self.cells[ci]
        key = (ci, idx, N, H, W)
        t = self._tmpl.get(key)
        if idx is not None and cell.m_ops[idx].kind is None:
            if t is None:                                   # (a skip binds nothing: always fresh)
                t = self._tmpl[key] = fill_pass_desc(TfnasCellDesc(), cell.in_channels, N, H, W)
            return t, True
        plan = cell._plan(tuple(range(len(cell.m_ops))) if idx is None else (idx,))
        ps = plan.params()
        first = ps[0].data_ptr()                            # (the first of hip_params(): skips stand last, a plan never starts with one)
        meta = self._tmeta.get(key)
        if t is not None and meta is not None and meta[0] == first and meta[2] is plan:
            plan.refresh(t)                                 # (the model's launch modes may have changed)
            return t, meta[1]
        for p in ps:
            _require_cuda(p, 'MBConv weight')
            if not p.is_contiguous():
                raise RuntimeError('tfnas_amd: MBConv weights must be contiguous')
        d = fill_cell_desc(TfnasCellDesc(), plan, N, H, W)
        owned = self.weights is not None and all(self.weights.owns(p) for p in ps)
        plan.bind(d, ps, [self.weights.grad_view(p) for p in ps] if owned else None)
        d.need_wgrad = 0
        check(self.lib.tfnas_cell_plan(C.byref(d)), 'tfnas_cell_plan')
        self._tmpl[key], self._tmeta[key] = d, (first, owned, plan)
        return d, owned

    def _cell_need(self, ci, idx, N, H, W):
        """Floats of workspace the library plans for candidate ``idx`` of cell ``ci`` (tfnas_cell_ws: saved + scratch tensors); a
        sampled skip owns none."""
        d = self._template(ci, idx, N, H, W)
        if self.cells[ci].m_ops[idx].kind is None:
            return 0
        ws = _lib.TfnasCellWs()
        check(self.lib.tfnas_cell_ws(C.byref(d), C.byref(ws)), 'tfnas_cell_ws')
        return int(ws.E + ws.D + ws.Pr + ws.fsmall + 2 * ws.stats + ws.out + ws.dZ + ws.dEh + ws.bsmall + 2 * ws.red + ws.dx + ws.dxp)

    def _widest(self, N, H, W):
        """Per cell the candidate whose planned workspace is the largest, asked of the library once per input shape (a Fused-MBConv
        candidate is not sized by its mid width, an expand-free one has no E, a skip nothing at all)."""
        key = (N, H, W)
        hit = self._wide.get(key)
        if hit is None:
            hit, h, w = [], H, W
            for ci, cell in enumerate(self.cells):
                hit.append(max(range(len(cell.m_ops)), key=lambda i: self._cell_need(ci, i, N, h, w)))
                h, w = (h - 1) // cell.stride + 1, (w - 1) // cell.stride + 1
            self._wide[key] = hit
        return hit

    def _slot(self, name):
        s = self._slots.get(name)
        if s is None:
            s = self._slots[name] = _Slot(self.lib)
        ws = self.wgrad_streams.get(name)
        if ws is not None and getattr(s, 'side', None) is not ws:
            check(self.lib.tfnas_path_set_side_stream(s.ctx, C.c_void_p(ws.cuda_stream)), 'tfnas_path_set_side_stream')
            s.side = ws
        return s

    def _plan(self, name, idxs, x0h, need_wgrad, need_dx0, need_dbetas):
        """Fill and plan slot ``name`` for candidates ``idxs`` (None: soft mode)."""
        s = self._slot(name)
        N, H, W, _ = x0h.shape
        soft = idxs is None
        pd = s.pd
        pd.ncell, pd.nstage, pd.soft, pd.need_dx0 = len(self.cells), len(self.stages), int(soft), int(need_dx0)
        pd.path_flags = self.path_flags
        mask = 0
        h, w = H, W
        for i, cell in enumerate(self.cells):
            t, owned = self._template_entry(i, None if soft else idxs[i], N, h, w)
            if need_wgrad and not owned:
                raise RuntimeError('tfnas_amd: weight gradients at the path level need a WeightArena that owns the weights')
            pd.cell[i] = t
            pd.cell[i].need_wgrad = int(need_wgrad)
            if soft and not need_wgrad and EFREE and ((cell.stride == 2 and cell.in_channels <= 24) or EFREE_STRIDE1) \
                    and self.lib.tfnas_efree_supported(C.byref(t)):
                mask |= 1 << i
            h, w = (h - 1) // cell.stride + 1, (w - 1) // cell.stride + 1
        pd.efree_mask_lo = mask
        if s.dbetas is None:
            s.dbetas = torch.zeros(self.nres_total, device=self.device, dtype=torch.float32)
        off = 0
        for k, st in enumerate(self.stages):
            sg = pd.stage[k]
            sg.ncell, sg.start_res = st.nblocks, st.start_res
            _require_cuda(st.betas, 'betas')
            sg.betas = st.betas.data_ptr()
            sg.dbetas = (s.dbetas.data_ptr() + 4 * off) if need_dbetas else None
            off += st.num_res
        check(self.lib.tfnas_path_plan(s.ctx, C.byref(pd), C.byref(s.ws)), 'tfnas_path_plan')
        if s.arena is None or s.arena.numel() < s.ws.total:
            need = int(s.ws.total)
            if not soft:
                # size the arena for the widest candidate of every cell once, instead of growing it (device sync + GBs of
                # hipMalloc) whenever a step samples a wider sub-network than any before
                wide = self._widest(N, H, W)
                if list(idxs) != wide:
                    need = max(need, self._sampled_need(name, wide, x0h, need_wgrad, need_dx0))
                    return self._plan_with_arena(name, idxs, x0h, need_wgrad, need_dx0, need_dbetas, need)
            self._grow(s, need)
        s.gen += 1
        return s

    def _grow(self, s, need):
        if s.arena is not None and s.arena.numel() >= need:
            return
        if s.arena is not None:
            torch.cuda.synchronize(self.device)             # (pending kernels may still use the old arena)
        s.arena = None
        s.arena = torch.zeros(int(need * 1.02) + 1024, device=self.device, dtype=torch.float32)

    def _sampled_need(self, name, wide, x0h, need_wgrad, need_dx0):
        tmp = '_size_probe'
        s = self._slot(tmp)
        s.arena = torch.empty(0, device=self.device)        # (never launched on; only the plan's size is wanted)
        N, H, W, _ = x0h.shape
        pd = s.pd
        pd.ncell, pd.nstage, pd.soft, pd.need_dx0, pd.efree_mask_lo = len(self.cells), len(self.stages), 0, int(need_dx0), 0
        pd.path_flags = self.path_flags
        h, w = H, W
        for i, cell in enumerate(self.cells):
            pd.cell[i] = self._template(i, wide[i], N, h, w)
            pd.cell[i].need_wgrad = int(need_wgrad)
            h, w = (h - 1) // cell.stride + 1, (w - 1) // cell.stride + 1
        for k, st in enumerate(self.stages):
            sg = pd.stage[k]
            sg.ncell, sg.start_res, sg.betas, sg.dbetas = st.nblocks, st.start_res, st.betas.data_ptr(), None
        check(self.lib.tfnas_path_plan(s.ctx, C.byref(pd), C.byref(s.ws)), 'tfnas_path_plan')
        return int(s.ws.total)

    def _plan_with_arena(self, name, idxs, x0h, need_wgrad, need_dx0, need_dbetas, need):
        self._grow(self._slot(name), need)
        return self._plan(name, idxs, x0h, need_wgrad, need_dx0, need_dbetas)

    # ---- raw calls ----------------------------------------------------------------------------------------------
    def _fwd(self, slots, x0s, wmix, clx, outs, out_lats, streams):
        n = len(slots)
        with _on(self.device):
            check(self.lib.tfnas_paths_fwd(
                n, raw_array([s.ctx.value for s in slots]), raw_array([t.data_ptr() for t in x0s]),
                raw_array([None if t is None else t.data_ptr() for t in wmix]),
                raw_array([None if t is None else t.data_ptr() for t in clx]),
                raw_array([s.arena.data_ptr() for s in slots]), raw_array([t.data_ptr() for t in outs]),
                raw_array([None if t is None else t.data_ptr() for t in out_lats]),
                raw_array([st.cuda_stream for st in streams])), 'tfnas_paths_fwd')

    def _bwd(self, slots, x0s, wmix, clx, douts, dlats, dx0s, dwmix, dclx, streams, stage_begin=0, stage_end=-1):
        n = len(slots)

        def pa(ts):
            return raw_array([None if t is None else t.data_ptr() for t in ts])
        with _on(self.device):
            check(self.lib.tfnas_paths_bwd(
                n, raw_array([s.ctx.value for s in slots]), pa(x0s), pa(wmix), pa(clx),
                raw_array([s.arena.data_ptr() for s in slots]), pa(douts), pa(dlats), pa(dx0s), pa(dwmix), pa(dclx),
                raw_array([st.cuda_stream for st in streams]), int(stage_begin), int(stage_end)), 'tfnas_paths_bwd')

    def expand_lat(self, CL):
        """[ncell] expected cell latencies -> stage-expanded [sum nres] (differentiable)."""
        return torch.cat([CL.new_zeros(1), CL]).index_select(0, self._lat_index)

    # ---- public: the three kinds of forward ---------------------------------------------------------------------
    def soft(self, x0, W, CL):
        """Architecture step: (out [N,oc,Ho,Wo], stage latencies [nstage]) for gumbel-softmax weights W [ncell, 8] and
        expected cell latencies CL [ncell] (ArchFn)."""
        betas = [st.betas for st in self.stages]
        return SoftPathFn.apply(self, x0, W.contiguous(), self.expand_lat(CL), *betas)

    def _wants_wgrad(self, idxs):
        for c, i in zip(self.cells, idxs):
            ps = c.m_ops[i].hip_params()                    # (a sampled skip has none: the first cell that computes decides)
            if ps:
                return torch.is_grad_enabled() and ps[-1].requires_grad
        return False

    def sampled(self, x0, idxs, name='A', expose=None, main_stream=None):
        """One sampled path (train_wo_arch / validate / a single bi-sampling path).  ``expose``: a SearchState -- the backward
        then points ``.grad`` of the sampled candidates' parameters at the arena ranges it wrote (module-API callers that
        run torch's clip_grad_norm_ / optimizer.step() on ``.grad``).  ``main_stream``: the caller's stream when this path is
        enqueued on ANOTHER (side) stream -- the backward then makes ``main_stream`` wait for the weight gradients it wrote
        (they bypass autograd's AccumulateGrad and its stream bookkeeping) once the whole backward pass has been enqueued."""
        idxs = tuple(int(i) for i in idxs)
        return OnePathFn.apply(self, x0, idxs, name, self._wants_wgrad(idxs), expose, main_stream)

    def bisampled(self, x0, idx_a, idx_b, side_stream):
        """Both bi-sampling paths of a weight step, interleaved on the current stream and ``side_stream``."""
        idx_a, idx_b = tuple(int(i) for i in idx_a), tuple(int(i) for i in idx_b)
        return BiPathFn.apply(self, x0, idx_a, idx_b, side_stream, self._wants_wgrad(idx_a))


def _out_tensor(s, N, dev):
    return torch.empty((N, s.ws.out_h, s.ws.out_w, s.ws.out_c), device=dev, dtype=torch.float32)


def _check_gen(s, gen):
    if s.ctx is None:
        raise RuntimeError('tfnas_amd: the path-level state of this forward was released (Network.close() / SearchState.release() '
                           '/ the model was rebuilt) before its backward ran')
    if s.gen != gen:
        raise RuntimeError('tfnas_amd: the path arena was overwritten by a later forward of the same slot before this '
                           'backward ran; run backward first or use the per-cell route (model(x, sampling, mode))')


class SoftPathFn(torch.autograd.Function):
    """out, stage_lat = all 18 soft MixedOPs + 6 sinks (models/model_search.py:86-91, :157-206) -- one C call each way."""

    @staticmethod
    def forward(ctx, runner, x0, W, CLx, *betas):
        _require_cuda(x0, 'path input')
        x0h = _nhwc(x0)
        dev = x0h.device
        need_w = any(p.requires_grad for p in runner.cells[0].m_ops[0].parameters())
        if need_w:
            raise RuntimeError('tfnas_amd: the soft path level runs with frozen weights (architecture step); use the '
                               'per-cell route for soft-mode weight gradients')
        s = runner._plan('soft', None, x0h, False, ctx.needs_input_grad[1], True)
        out = _out_tensor(s, x0h.shape[0], dev)
        out_lat = torch.empty(len(runner.stages), device=dev, dtype=torch.float32)
        cur = torch.cuda.current_stream(dev)
        runner._fwd([s], [x0h], [W], [CLx], [out], [out_lat], [cur])
        ctx.runner, ctx.slot, ctx.gen = runner, s, s.gen
        ctx.save_for_backward(x0h, W, CLx)
        return out.permute(0, 3, 1, 2), out_lat

    @staticmethod
    def backward(ctx, dout, dlat):
        runner, s = ctx.runner, ctx.slot
        _check_gen(s, ctx.gen)
        x0h, W, CLx = ctx.saved_tensors
        dev = x0h.device
        douth = _nhwc(dout)
        dlat = None if dlat is None else dlat.contiguous()
        want_dx = bool(s.pd.need_dx0)
        dx0 = torch.empty_like(x0h) if want_dx else None
        dW = torch.empty_like(W)
        dCLx = torch.zeros_like(CLx)
        cur = torch.cuda.current_stream(dev)
        runner._bwd([s], [x0h], [W], [CLx], [douth], [dlat], [dx0], [dW], [dCLx], [cur])
        db = s.dbetas.clone()
        dbetas, off = [], 0
        for st in runner.stages:
            dbetas.append(db[off:off + st.num_res])
            off += st.num_res
        return (None, None if dx0 is None else dx0.permute(0, 3, 1, 2), dW, dCLx) + tuple(dbetas)


class OnePathFn(torch.autograd.Function):
    """One sampled path; weight gradients go straight into the WeightArena (not through autograd).  With ``expose`` they are
    summed into existing ``.grad`` the way autograd's AccumulateGrad would (SearchState.prepare_grad_targets)."""

    @staticmethod
    def forward(ctx, runner, x0, idxs, name, need_w, expose=None, main_stream=None):   # (grad mode is off inside forward: need_w comes from outside)
        _require_cuda(x0, 'path input')
        x0h = _nhwc(x0)
        dev = x0h.device
        ctx.expose, ctx.idxs, ctx.need_w, ctx.name, ctx.main_stream = expose, idxs, need_w, name, main_stream
        s = runner._plan(name, idxs, x0h, need_w, ctx.needs_input_grad[1], False)
        out = _out_tensor(s, x0h.shape[0], dev)
        cur = torch.cuda.current_stream(dev)
        runner._fwd([s], [x0h], [None], [None], [out], [None], [cur])
        ctx.runner, ctx.slot, ctx.gen = runner, s, s.gen
        ctx.save_for_backward(x0h)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dout):
        runner, s = ctx.runner, ctx.slot
        _check_gen(s, ctx.gen)
        x0h, = ctx.saved_tensors
        dx0 = torch.empty_like(x0h) if s.pd.need_dx0 else None
        cur = torch.cuda.current_stream(x0h.device)
        if ctx.expose is not None and ctx.need_w:
            # module-API route: sum into .grad like AccumulateGrad would, decided per cell now (a zero_grad() between this
            # path's forward and its backward still makes it write); the plan of the forward stays where it is
            mask = ctx.expose.prepare_grad_targets(ctx.idxs)
            check(runner.lib.tfnas_path_set_wgrad_accum(s.ctx, mask), 'tfnas_path_set_wgrad_accum')
        args = ([s], [x0h], [None], [None], [_nhwc(dout)], [None], [dx0], [None], [None], [cur])
        hook, k = runner.segment_hook, runner.split_stage
        if hook is not None and 0 < k < len(runner.stages):
            runner._bwd(*args, stage_begin=k, stage_end=-1)
            hook(cur, None)
            runner._bwd(*args, stage_begin=0, stage_end=k)
        else:
            runner._bwd(*args)
        if ctx.expose is not None and ctx.need_w:
            ctx.expose.expose_weight_grads([ctx.idxs], track=False)
        main = ctx.main_stream
        if main is not None and main != cur and ctx.need_w:
            # this path ran on a side stream: whatever the caller enqueues on its own stream after backward() -- clip_grad_norm_,
            # optimizer.step() -- reads the arena ranges written here.  Not a wait issued now (the other path's backward is
            # enqueued on `main` after this one and must not queue up behind it) but when the engine has finished the pass.
            ev = torch.cuda.Event()
            ev.record(cur)
            torch.autograd.Variable._execution_engine.queue_callback(lambda: main.wait_event(ev))
        return None, None if dx0 is None else dx0.permute(0, 3, 1, 2), None, None, None, None, None


class BiPathFn(torch.autograd.Function):
    """Both bi-sampling paths of a weight step (train_search.py:375-379) as ONE autograd node: the forward and the backward
    of the two paths are enqueued interleaved, cell by cell, on the current stream (path A) and ``side`` (path B)."""

    @staticmethod
    def forward(ctx, runner, x0, idx_a, idx_b, side, need_w):
        _require_cuda(x0, 'path input')
        x0h = _nhwc(x0)
        dev = x0h.device
        want_dx = ctx.needs_input_grad[1]
        sa = runner._plan('A', idx_a, x0h, need_w, want_dx, False)
        sb = runner._plan('B', idx_b, x0h, need_w, want_dx, False)
        oa, ob = _out_tensor(sa, x0h.shape[0], dev), _out_tensor(sb, x0h.shape[0], dev)
        cur = torch.cuda.current_stream(dev)
        side.wait_stream(cur)                      # x0 and the weights are ready on the current stream
        ob.record_stream(side)
        x0h.record_stream(side)
        runner._fwd([sa, sb], [x0h, x0h], [None, None], [None, None], [oa, ob], [None, None], [cur, side])
        ctx.runner, ctx.slots, ctx.gens, ctx.side = runner, (sa, sb), (sa.gen, sb.gen), side
        ctx.save_for_backward(x0h)
        return oa.permute(0, 3, 1, 2), ob.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, da, db):
        runner, (sa, sb), side = ctx.runner, ctx.slots, ctx.side
        _check_gen(sa, ctx.gens[0])
        _check_gen(sb, ctx.gens[1])
        x0h, = ctx.saved_tensors
        dev = x0h.device
        cur = torch.cuda.current_stream(dev)
        dah, dbh = _nhwc(da), _nhwc(db)
        want_dx = bool(sa.pd.need_dx0)
        dxa = torch.empty_like(x0h) if want_dx else None
        dxb = torch.empty_like(x0h) if want_dx else None
        side.wait_stream(cur)                      # autograd has made the current stream wait for both incoming gradients
        dbh.record_stream(side)
        if dxb is not None:
            dxb.record_stream(side)
        args = ([sa, sb], [x0h, x0h], [None, None], [None, None], [dah, dbh], [None, None], [dxa, dxb], [None, None],
                [None, None], [cur, side])
        hook, k = runner.segment_hook, runner.split_stage
        if hook is not None and 0 < k < len(runner.stages):
            # late stages first; their weight gradients can be reduced across ranks while the early stages still run
            runner._bwd(*args, stage_begin=k, stage_end=-1)
            hook(cur, side)
            runner._bwd(*args, stage_begin=0, stage_end=k)
        else:
            runner._bwd(*args)
        cur.wait_stream(side)
        dx = None
        if want_dx:
            dx = (dxa + dxb).permute(0, 3, 1, 2)
        return None, dx, None, None, None, None
