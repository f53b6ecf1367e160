"""Helpers of the tests of the path level on extended-candidate supernets (model_search.Network(..., extended_paths=True):
tests/test_paths_ext_host.py, tests/test_gpu_paths_ext.py, tests/test_gpu_paths_ext_search.py).

The network: every residual cell holds RES -- a plain, a Fused-MBConv, a dilated expand-free, a MixConv, an SE Fused-MBConv, an SE
expand-free, a 7 x 7 candidate and a skip --, every other cell NONRES (the same list with an SE 5 x 5 candidate in place of the
skip); _kinds.AnyLut-style latencies whose IdentityLayer keys cost nothing (_skip.SkipLut)."""
import ctypes as C

import torch

import _dil
import _fused
import _mix
import _skip
import tfnas_oracle as orc

RES = ['MBI_k3_e3', 'FMB_k3_e6', 'DS_k5d2', 'MBI_k35_e6', 'FMB_k3_e3_se', 'DS_k3_se', 'MBI_k7_e6', 'skip']
NONRES = RES[:7] + ['MBI_k5_e6_se']
SKIP_IDX = 7
# (batch, image size): the existing search tests' shape, and one at which 7 x 7, dilated and MixConv tiles and the stride-2 cells
# of stages 3-5 see more than one pixel
SHAPES = [(4, 32), (2, 64)]


def primitives(stages=None):
    """{stage: {block: names}}: RES in the residual cells, NONRES elsewhere; ``stages``: only these (the others: the defaults)"""
    from tfnas_amd import geometry
    res = set(geometry.residual_cells())
    prims = {}
    for st, b, *_ in geometry.iter_cells():
        if stages is None or st in stages:
            prims.setdefault(st, {})[b] = list(RES if (st, b) in res else NONRES)
    return prims


def lut():
    t = _skip.SkipLut()
    t['base'] = 1.5
    return t


def model(extended_paths=None, seed=2, T=5.0, stages=None, cuda=True):
    """The extended network; ``extended_paths`` None: built without the keyword"""
    from tfnas_amd import Network, geometry
    torch.manual_seed(seed)
    kw = {} if extended_paths is None else {'extended_paths': extended_paths}
    m = Network(100, geometry.initial_mc_num_dddict(), lut(), primitives=primitives(stages), **kw)
    m.set_temperature(T)
    return m.cuda() if cuda else m


def cell_names():
    from tfnas_amd import geometry
    return [(st, b) for st, b, *_ in geometry.iter_cells()]


def cell_index():
    return {c: i for i, c in enumerate(cell_names())}


def residual_index():
    from tfnas_amd import geometry
    idx = cell_index()
    return [idx[c] for c in geometry.residual_cells()]


class Recorder:
    """Records (cell index, sampled candidate index) of every MixedOP.sample_index call of ``m`` while active."""

    def __init__(self, m):
        self.m, self.seen = m, []

    def __enter__(self):
        from tfnas_amd import model_search
        self._cls, self._orig = model_search.MixedOP, model_search.MixedOP.sample_index
        where = {id(c): i for i, c in enumerate(self.m.cells())}
        orig, seen = self._orig, self.seen

        def sample_index(cell, *a, **kw):
            idx = orig(cell, *a, **kw)
            if id(cell) in where:
                seen.append((where[id(cell)], idx))
            return idx
        self._cls.sample_index = sample_index
        return self

    def __exit__(self, *exc):
        self._cls.sample_index = self._orig
        return False


def oracle_pair(seed=2, T=5.0):
    """(oracle Network, product Network(primitives=..., extended_paths=True)) with identical weights: stage 1 on the default
    primitives, the restatement blocks of tests/_fused.py, _dil.py, _mix.py and _skip.py in stages 2-6"""
    from tfnas_amd import Network, geometry
    stages = ('stage2', 'stage3', 'stage4', 'stage5', 'stage6')
    prims = primitives(stages)
    mc = geometry.initial_mc_num_dddict()
    torch.manual_seed(seed)
    o = orc.Network(100, orc.initial_mc_num_dddict(), lut())
    gen = torch.Generator().manual_seed(seed + 1)
    for st, b, ic, oc, s, act, size in geometry.iter_cells():
        names = geometry.cell_primitives(prims, st, b)
        cell = getattr(getattr(o, st), b)
        for i, name in enumerate(names):
            if name == geometry.PRIMITIVES[i]:
                continue
            layer, mid, se, k = geometry.primitive_block(name, ic, mc[st][b][i])
            if layer == 'IdentityLayer':
                cell.m_ops[i] = _skip.IdentityRef(ic, oc)
                continue
            if layer == 'FusedMBConvBlock':
                blk = _fused.FusedRef(ic, mid, se, oc, s, act)
                blk.name = layer
            else:
                blk = orc.MBConv(ic, mid, se, oc, k, s, act)
            with torch.no_grad():
                for p in blk.parameters():
                    if p.dim() == 1:
                        p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            d, ks = geometry.primitive_dilation(name), geometry.primitive_mix_kernels(name)
            if d != 1:
                _dil.dilate(blk, d)
                blk.kernel_size = _dil.KTag(k, d)
            if ks is not None:
                _mix.mixify(blk, ks)
                blk.kernel_size = _mix.KTag(ks)
            cell.m_ops[i] = blk
    m = Network(100, mc, lut(), primitives=prims, extended_paths=True)
    assert list(o.state_dict()) == list(m.state_dict())
    m.load_state_dict(o.state_dict())
    o.set_temperature(T)
    m.set_temperature(T)
    return o, m.cuda()


# ------------------------------------------------------------------------------------------------ descriptors
INT_FIELDS = ('N', 'H', 'W', 'ic', 'oc', 'stride', 'act', 'has_res', 'G', 'need_wgrad', 'Ho', 'Wo', 'M', 'SE', 'mode', 'Hi', 'Wi',
              'stor', 'gemm_mode', 'flags', 'sync_world', 'route', 'fwd_route', 'pad_route')
GROUP_INTS = ('mc', 'k', 'se', 'mcp', 'off', 'se_off', 'kind', 'dil')


def desc_words(d):
    """every field of a TfnasCellDesc as a flat {name: value} (pointers as integers, None as 0)"""
    from tfnas_amd import _lib
    out = {f: getattr(d, f) for f in INT_FIELDS}
    out['eps'] = d.eps
    for f in ('sync_fn', 'sync_user'):
        out[f] = getattr(d, f) or 0
    for k in range(3):
        out['wgrad_stream%d' % k] = d.wgrad_stream[k] or 0
    for g in range(_lib.MAX_GROUPS):
        for f in GROUP_INTS + _lib._W_FIELDS + _lib._G_FIELDS:
            out['g%d.%s' % (g, f)] = getattr(d.g[g], f) or 0
    return out


def expected_desc(cell, idxs, N, H, W, route):
    """The unplanned descriptor the per-cell route builds for candidates ``idxs`` of MixedOP ``cell`` -- restated here from the
    blocks alone (include/tfnas_hip.h), not through functions.CellPlan -- with the blocks' weight pointers bound."""
    from tfnas_amd import _lib
    blocks = [cell.m_ops[i] for i in idxs]
    d = _lib.TfnasCellDesc()
    d.N, d.H, d.W, d.ic, d.oc, d.stride = N, H, W, cell.in_channels, cell.out_channels, cell.stride
    d.mode, d.act, d.G, d.eps = _lib.MODE_CELL, _lib.ACT[cell.act_func], len(blocks), 1e-5
    d.has_res = int(cell.in_channels == cell.out_channels and cell.stride == 1)
    kinds = [b.kind for b in blocks]
    flags = 0
    for g, b in enumerate(blocks):
        gr = d.g[g]
        mk = getattr(b, 'mix_kernels', None)
        gr.mc, gr.se = b.mid_channels, b.se_channels
        gr.k = b.kernel_size if mk is None else sum(k << (4 * s) for s, k in enumerate(mk))
        gr.dil = 2 if getattr(b, 'dilation', 1) == 2 else 0
        if gr.k == 7 or (mk is not None and 7 in mk):
            flags |= _lib.CELL_K7
        if mk is not None:
            flags |= _lib.CELL_MIXK
        if gr.dil == 2:
            flags |= _lib.CELL_DILATION
        if kinds[g] is not None:
            ps = b.hip_params()
            for j, p in zip(kinds[g].bound(b.se_channels > 0), ps):
                setattr(gr, _lib._W_FIELDS[j], p.data_ptr())
    if len(blocks) == 1:
        flags |= kinds[0].flag
    elif any(k is not _lib.MBCONV for k in kinds):
        flags |= _lib.CELL_KINDS
        for g, k in enumerate(kinds):
            if k is None:
                flags |= _lib.CELL_SKIP
                d.g[g].kind = _lib.GROUP_SKIP
            else:
                d.g[g].kind = _lib.KINDS.index(k)
    d.flags = flags
    d.route = route
    return d


# ------------------------------------------------------------------------------------------------ raw path plans
class RawPlan:
    """tfnas_path_plan on a hand-made one-stage TfnasPathDesc (GPU: tfnas_path_create needs a device)"""

    def __init__(self):
        from tfnas_amd import _lib
        self._lib, self.lib = _lib, _lib.lib()
        self.ctx = C.c_void_p()
        _lib.check(self.lib.tfnas_path_create(C.byref(self.ctx)), 'tfnas_path_create')
        self.betas = torch.zeros(8, device='cuda')

    def close(self):
        self.lib.tfnas_path_destroy(self.ctx)

    def plan(self, cells, soft, start_res, efree_mask=0, path_flags=1):
        """return code of tfnas_path_plan for one stage of ``cells`` (unplanned descriptors); path_flags: TFNAS_PATH_EXTENDED"""
        lb = self._lib
        pd, ws = lb.TfnasPathDesc(), lb.TfnasPathWs()
        pd.ncell, pd.nstage, pd.soft, pd.need_dx0, pd.efree_mask_lo = len(cells), 1, int(soft), 1, efree_mask
        pd.path_flags = path_flags
        pd.stage[0].ncell, pd.stage[0].start_res = len(cells), start_res
        pd.stage[0].betas = self.betas.data_ptr()
        for i, d in enumerate(cells):
            pd.cell[i] = d
        return self.lib.tfnas_path_plan(self.ctx, C.byref(pd), C.byref(ws)), ws
