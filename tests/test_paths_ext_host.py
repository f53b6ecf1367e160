"""CPU-side checks of ``model_search.Network(..., extended_paths=...)``: the keyword defaults to off and then changes nothing -- a
default network and an extended one built without it report what they always did --, it is a routing switch of the Network alone
(not handed down, not in state_dict), and the ONE descriptor filler (functions.fill_cell_desc, shared by the per-cell route and
path.PathRunner._template) gives, field for field, the descriptor the per-cell route builds -- restated from the blocks alone in
tests/_pathsext.py -- for one cell of each kind and for a mixed cell with a skip.  (tfnas_path_create needs a device: the plan rules
are tested in tests/test_gpu_paths_ext.py.)"""
import ctypes as C
import inspect
import os

import pytest
import torch

import _pathsext as px


@pytest.fixture(scope='module')
def lib():
    from tfnas_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


def test_keyword_defaults_to_off_and_is_the_networks_alone():
    from tfnas_amd import Network, geometry
    from tfnas_amd.model_search import MixedOP, MixedStage
    sig = inspect.signature(Network.__init__)
    assert sig.parameters['extended_paths'].default is False
    assert 'extended_paths' not in inspect.signature(MixedStage.__init__).parameters
    assert 'extended_paths' not in inspect.signature(MixedOP.__init__).parameters
    plain = Network(100, geometry.initial_mc_num_dddict(), px.lut())
    assert plain.extended_paths is False and plain.plain_candidates() and plain.path_capable()
    assert plain._use_paths(torch.zeros(1)) is False                 # (a CPU tensor never takes the path level)


def test_networks_built_without_the_keyword_report_what_they_always_did():
    from tfnas_amd import Network, geometry
    plain = Network(100, geometry.initial_mc_num_dddict(), px.lut())
    m = px.model(cuda=False)                                          # the extended network, no keyword
    on = px.model(True, cuda=False)
    off = px.model(False, cuda=False)
    assert m.extended_paths is False and off.extended_paths is False and on.extended_paths is True
    for net in (m, on, off):
        assert net.plain_candidates() is False                        # keeps its meaning and its value
        assert net._use_paths(torch.zeros(1)) is False
    assert m.path_capable() is False and off.path_capable() is False and on.path_capable() is True
    assert list(m.state_dict()) == list(on.state_dict()) == list(off.state_dict())
    assert not any('extended' in k for k in on.state_dict())
    # (outside the cells the extended network has the default network's keys)
    assert [k for k in m.state_dict() if not k.startswith('stage')] == [k for k in plain.state_dict() if not k.startswith('stage')]
    assert not any(hasattr(mod, 'extended_paths') for mod in on.modules() if mod is not on)
    names = [op.name for c in on.cells() for op in c.m_ops]
    assert names.count('IdentityLayer') == 12


# one cell of each kind (a plain, a Fused-MBConv, a dilated expand-free, a MixConv, an SE expand-free, a 7 x 7 candidate), the
# soft cell of a non-residual position and the mixed-with-skip soft cell of a residual one
CASES = [('stage3', 'block2', (0,)), ('stage3', 'block2', (1,)), ('stage3', 'block2', (2,)), ('stage3', 'block2', (3,)),
         ('stage2', 'block1', (4,)), ('stage4', 'block3', (5,)), ('stage5', 'block1', (6,)), ('stage6', 'block1', (7,)),
         ('stage3', 'block1', tuple(range(8))), ('stage3', 'block3', tuple(range(8)))]


@pytest.mark.parametrize('stage,block,idxs', CASES, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_shared_filler_gives_the_per_cell_routes_descriptor(lib, stage, block, idxs):
    from tfnas_amd import _lib, functions
    m = px.model(True, cuda=False)
    cell = getattr(getattr(m, stage), block)
    N, H, W = 2, 6, 5
    plan = cell._plan(idxs)
    got = functions.fill_cell_desc(_lib.TfnasCellDesc(), plan, N, H, W)
    params = plan.params()
    plan.bind(got, params)
    want = px.expected_desc(cell, idxs, N, H, W, functions.ENV_ROUTE)
    a, b = px.desc_words(got), px.desc_words(want)
    assert a == b, {k: (a[k], b[k]) for k in a if a[k] != b[k]}
    if len(idxs) == 8 and (stage, block) == ('stage3', 'block3'):
        assert got.flags & _lib.CELL_SKIP and got.g[7].kind == _lib.GROUP_SKIP and got.g[7].w_proj is None
    # ... it is what CellPlan.desc plans (the per-cell route's own call), and the library accepts it
    d, ws = plan.desc(N, H, W)
    plan.bind(d, params)
    assert lib.tfnas_cell_plan(C.byref(got)) == 0
    assert px.desc_words(got) == px.desc_words(d)


def test_pass_through_descriptor_is_refused_by_the_per_cell_plan(lib):
    from tfnas_amd import _lib, functions
    d = functions.fill_pass_desc(_lib.TfnasCellDesc(), 80, 2, 4, 4)
    assert d.G == 1 and d.flags == _lib.CELL_KINDS | _lib.CELL_SKIP and d.g[0].kind == _lib.GROUP_SKIP
    assert (d.ic, d.oc, d.stride, d.has_res) == (80, 80, 1, 1)
    assert lib.tfnas_cell_plan(C.byref(d)) == -1                      # TFNAS_EINVAL: an all-skip descriptor has nothing to launch
