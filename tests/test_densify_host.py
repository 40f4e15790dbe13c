"""Host-side tests of the densification layer (no GPU): the wrappers refuse wrong dtypes, shapes and devices and a
parameter that is not the single member of an optimizer group, before anything is launched; the ctypes signatures and the
mirrored struct and constants are the header's; the workspace size is the header's formula."""
import ctypes
import os
import re

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, densify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'exa_raster.h')


def _inputs(P=5, **over):
    t = dict(grad_accum=torch.zeros(P, 1), track_cnt=torch.ones(P, 1), scale=torch.zeros(P, 3), opacity=torch.zeros(P, 1),
             extent=torch.ones(1))
    t.update(over)
    return [t[k] for k in ('grad_accum', 'track_cnt', 'scale', 'opacity', 'extent')]


@pytest.mark.parametrize('over,error,match', [
    (dict(scale=torch.zeros(5, 3, dtype=torch.float64)), ValueError, 'scale must be float32'),
    (dict(grad_accum=torch.zeros(5, 1, dtype=torch.float16)), ValueError, 'grad_accum must be float32'),
    (dict(opacity=torch.zeros(5, 1, dtype=torch.int32)), ValueError, 'opacity must be float32'),
    (dict(scale=[0.0] * 15), TypeError, 'scale must be a tensor'),
    (dict(scale=torch.zeros(5, 4)), ValueError, r'scale must be \[P, 3\]'),
    (dict(track_cnt=torch.ones(4, 1)), ValueError, 'track_cnt must hold 5 rows'),
    (dict(opacity=torch.zeros(5, 2)), ValueError, 'opacity must hold 5 rows of 1'),
    (dict(extent=torch.ones(2)), ValueError, 'extent must be a device tensor with one element'),
    (dict(), RuntimeError, 'ROCm device only'),
])
def test_densify_plan_refuses(over, error, match):
    with pytest.raises(error, match=match):
        densify.densify_plan(*_inputs(**over), grad_thr=0.0002)


def test_densify_plan_refuses_a_split_factor_outside_1_to_8():
    for sf in (0, 9):
        with pytest.raises(ValueError, match='split_factor must be in 1 .. 8'):
            densify.densify_plan(*_inputs(), grad_thr=0.0002, split_factor=sf)


def test_prune_plan_refuses():
    with pytest.raises(TypeError, match='must be a tensor'):
        densify.prune_plan([True, False])
    with pytest.raises(RuntimeError, match='ROCm device only'):
        densify.prune_plan(torch.zeros(4, dtype=torch.bool))


def _plan(P0=5, totals=(3, 1, 1, 2)):
    return densify.DensifyPlan(torch.empty(densify.workspace_size(P0), dtype=torch.uint8), P0, 2, totals, torch.device('cpu'))


def test_a_plan_exposes_its_counts():
    plan = _plan()
    assert (plan.n_keep, plan.n_clone, plan.n_split, plan.n_cand, plan.n_out) == (3, 1, 1, 2, 6)
    assert 'n_cand=2' in repr(plan)


@pytest.mark.parametrize('kw,error,match', [
    (dict(tensors=[torch.zeros(5, 2, dtype=torch.float64)]), ValueError, r'tensors\[0\] must be float32'),
    (dict(tensors=[torch.zeros(4, 2)]), ValueError, r'tensors\[0\] must hold 5 rows'),
    (dict(tensors=[torch.zeros(5, 0)]), ValueError, 'rows of no elements'),
    (dict(tensors=[], mean=torch.zeros(5, 4), scale=torch.zeros(5, 3), rotation=torch.zeros(5, 6)), ValueError,
     'mean must hold 5 rows of 3'),
    (dict(tensors=[], mean=torch.zeros(5, 3), scale=torch.zeros(5, 3), rotation=torch.zeros(5, 4)), ValueError,
     'rotation must hold 5 rows of 6'),
    (dict(tensors=[], mean=torch.zeros(5, 3)), ValueError, 'mean needs scale and rotation'),
    (dict(tensors=[], mean=torch.zeros(5, 3), scale=torch.zeros(5, 3), rotation=torch.zeros(5, 6)), ValueError,
     r'noise \[4, 3\] is needed'),
    (dict(tensors=[], mean=torch.zeros(5, 3), scale=torch.zeros(5, 3), rotation=torch.zeros(5, 6), noise=torch.zeros(2, 3)),
     ValueError, r'noise must be \[split_factor \* n_cand, 3\]'),
    (dict(tensors=[], states=[torch.zeros(5, dtype=torch.int64)]), ValueError, r'states\[0\] must be float32'),
    (dict(tensors=[torch.zeros(5, 2)]), RuntimeError, 'ROCm device only'),
])
def test_densify_apply_refuses(kw, error, match):
    with pytest.raises(error, match=match):
        densify.densify_apply(_plan(), kw.pop('tensors'), **kw)


def test_densify_apply_refuses_what_is_no_plan():
    with pytest.raises(TypeError, match='plan must be a DensifyPlan'):
        densify.densify_apply((3, 1, 1, 2), [torch.zeros(5, 2)])


def _scene(P=6):
    scene = exa.SceneGaussian()
    scene.init_from_point_num(P, device='cpu')
    return scene


def test_scene_gaussian_refuses_a_parameter_that_is_not_the_single_member_of_a_group():
    scene = _scene()
    groups = scene.get_optimizable_params()
    assert [g['name'] for g in groups] == ['mean_scene', 'feature_dc_scene', 'feature_rest_scene', 'opacity_scene', 'scale_scene',
                                           'rotation_scene']
    shared = torch.optim.Adam([{'params': [scene.mean, scene.scale], 'name': 'both'}] + groups[1:4] + groups[5:], lr=0.0)
    do_prune = torch.zeros(6, dtype=torch.bool)
    for call in (lambda: scene.densify_and_prune(None, shared), lambda: scene.prune_points(do_prune, shared)):
        with pytest.raises(ValueError, match='mean must be the single member of its optimizer group'):
            call()
    partial = torch.optim.Adam(groups[:5], lr=0.0)
    with pytest.raises(ValueError, match='rotation is in no group of the optimizer'):
        scene.densify_and_prune(20, partial)
    with pytest.raises(ValueError, match='do_prune has 5 entries for 6 points'):
        scene.prune_points(torch.zeros(5, dtype=torch.bool), torch.optim.Adam(groups, lr=0.0))
    assert scene.mean.shape[0] == 6 and int(scene.point_num[0]) == 6      # nothing changed


def test_scene_gaussian_keeps_the_references_names_and_defaults():
    scene = _scene()
    assert list(scene.state_dict()) == ['mean', 'scale', 'rotation', 'feature_dc', 'feature_rest', 'opacity', 'point_num',
                                        'active_sh_degree', 'radius_max', 'xyz_grad_accum', 'track_cnt', 'cam_dist_trans',
                                        'cam_dist_radius']
    assert (scene.max_sh_degree, scene.increase_sh_degree_interval, scene.densify_grad_thr, scene.opacity_min,
            scene.dense_percent_thr) == (3, 1000, 0.0002, 0.005, 0.01)
    assert tuple(scene.feature_rest.shape) == (6, 15, 3) and scene.point_num.dtype == torch.int64
    scene.cam_dist_radius[:] = 2.0
    lrs = {g['name']: g['lr'] for g in scene.get_optimizable_params()}
    assert lrs == {'mean_scene': 0.00016 * 2.0, 'feature_dc_scene': 0.0025, 'feature_rest_scene': 0.0025 / 20.0,
                   'opacity_scene': 0.05, 'scale_scene': 0.005, 'rotation_scene': 0.001}
    for itr, deg in ((0, 0), (999, 0), (1000, 1), (2500, 2), (3000, 3), (99999, 3)):
        scene.set_sh_degree(itr)
        assert scene._sh_degree == deg and float(scene.active_sh_degree[0]) == deg
    other = _scene()
    other.load_state_dict(scene.state_dict())
    assert other._sh_degree == 3


def test_reset_opacity_is_the_references_expression_and_zeroes_the_moments():
    scene = _scene()
    with torch.no_grad():
        scene.opacity.copy_(torch.tensor([[-9.0], [-5.0], [-4.0], [0.0], [3.0], [9.0]]))
    opt = torch.optim.Adam(scene.get_optimizable_params(), lr=0.0, eps=1e-15)
    old = scene.opacity
    opt.state[old] = {'step': torch.tensor(4.0), 'exp_avg': torch.ones(6, 1), 'exp_avg_sq': torch.ones(6, 1)}
    want = torch.minimum(torch.sigmoid(old.detach()), torch.ones(6, 1) * 0.01)
    want = torch.log(want / (1 - want))
    scene.reset_opacity(opt)
    assert torch.equal(scene.opacity.detach(), want) and scene.opacity is not old and old not in opt.state
    st = opt.state[scene.opacity]
    assert float(st['step']) == 4.0 and not st['exp_avg'].any() and not st['exp_avg_sq'].any()
    assert opt.param_groups[3]['params'][0] is scene.opacity


# ---- the binding against the header ----------------------------------------------------------------------------------
CTYPES = {'int32_t': ctypes.c_int32, 'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double}


def _header():
    src = open(HEADER).read()
    return src, re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def test_the_signatures_are_the_headers():
    _, code = _header()
    protos = dict(re.findall(r'\bint (exa_raster_densify_\w+)\s*\(([^()]*)\)\s*;', code))
    del protos['exa_raster_densify_stats']               # the statistics call, older than this layer
    assert sorted(protos) == ['exa_raster_densify_move', 'exa_raster_densify_plan', 'exa_raster_densify_workspace_size']
    for name, params in protos.items():
        res, args = _lib.RASTER.signatures[name]
        assert res is ctypes.c_int
        want = []
        for p in (x.strip() for x in params.split(',')):
            if p.startswith('uint64_t*'):
                want.append(ctypes.POINTER(ctypes.c_uint64))
            elif 'ExaRasterDensifySegment*' in p:
                want.append(ctypes.POINTER(_lib.ExaRasterDensifySegment))
            elif '*' in p:
                want.append(ctypes.c_void_p)
            else:
                want.append(CTYPES[p.split()[0]])
        assert list(args) == want, name


def test_the_constants_and_the_struct_are_the_headers():
    _, code = _header()
    defines = {k: int(v) for k, v in re.findall(r'#define (EXA_RASTER_DENSIFY_\w+) (\d+)', code)}
    mine = {'MAX_SEGMENTS': _lib.DENSIFY_MAX_SEGMENTS, 'BLOCK': _lib.DENSIFY_BLOCK, 'SCAN': _lib.DENSIFY_SCAN,
            'KEEP': _lib.DENSIFY_KEEP, 'CLONE': _lib.DENSIFY_CLONE, 'SPLIT': _lib.DENSIFY_SPLIT, 'CAND': _lib.DENSIFY_CAND,
            'COPY': _lib.DENSIFY_COPY, 'STATE': _lib.DENSIFY_STATE, 'MEAN': _lib.DENSIFY_MEAN, 'SCALE': _lib.DENSIFY_SCALE}
    assert defines == {'EXA_RASTER_DENSIFY_' + k: v for k, v in mine.items()}
    assert (densify.BLOCK, densify.SCAN_WIDTH, densify.MAX_SEGMENTS) == (mine['BLOCK'], mine['SCAN'], mine['MAX_SEGMENTS'])
    body = re.search(r'typedef struct ExaRasterDensifySegment \{(.*?)\}', code, flags=re.S).group(1)
    fields = [f.strip().split()[-1] for f in body.split(';') if f.strip()]
    assert fields == [f[0] for f in _lib.ExaRasterDensifySegment._fields_]
    assert ctypes.sizeof(_lib.ExaRasterDensifySegment) == 40
    assert ctypes.sizeof(_lib.ExaRasterDensifySegment) * mine['MAX_SEGMENTS'] + 128 <= 4096      # the argument block


@pytest.mark.parametrize('P0', (0, 1, 15, 16, 17, 255, 256, 257, 700, 65793, 2 ** 31 - 1))
def test_the_workspace_size_is_the_headers_formula(P0):
    blocks = -(-P0 // densify.BLOCK)
    assert densify.workspace_size(P0) == 16 + 16 * blocks + 16 * (-(-P0 // 16))
    assert densify.workspace_size(P0) >= 16 + 16 * blocks + P0


def test_the_size_query_refuses_on_the_host():
    lib = _lib.load()
    assert lib.exa_raster_densify_workspace_size(-1, ctypes.byref(ctypes.c_uint64())) == -1
    assert lib.exa_raster_densify_workspace_size(4, None) == -2
    with pytest.raises(RuntimeError, match='negative P0'):
        densify.workspace_size(-3)
