"""The reference's own calling code at the boundary: ``class GaussianRenderer`` (reference
avatar/common/nets/module.py:588-647).  ``tests/golden/ref_renderer.npz`` holds what that class -- exec'd unchanged by
``tests/golden/make_golden_renderer.py`` -- builds and returns for two scenes (settings tuple, keyword arguments, the six-key
output dict, ``mean_2d.grad``, the gradients) with the CPU oracle behind it.  Here: this package's renderer builds the same
settings bit for bit, the oracle's twin of the renderer reproduces the outputs, and ``exa.GaussianRenderer`` itself returns
what the reference's class returned."""
import os

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import rasterizer, renderer
from oracle import raster_oracle as ro

@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ref_renderer.npz'))


@pytest.fixture(autouse=True)
def _one_thread():
    """The fixture was generated with one CPU thread (make_golden_renderer.py): the oracle's reductions round differently when
    PyTorch splits them over threads, and the comparisons below are bitwise."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _case(golden, name):
    p = name + '_'
    assets = {k[len(p) + 6:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith(p + 'asset_')}
    cam = {k[len(p) + 4:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith(p + 'cam_')}
    shape = tuple(int(v) for v in golden[p + 'shape'])
    bg = torch.from_numpy(golden[p + 'bg']) if bool(golden[p + 'bg_given']) else None
    return assets, shape, cam, bg


def _oracle_rasterize(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                      densify_stats=None):
    """``rasterizer.rasterize_gaussians`` with the CPU oracle behind it (this container has no GPU)."""
    s = raster_settings
    so = ro.OracleSettings(image_height=int(s.image_height), image_width=int(s.image_width), tanfovx=s.tanfovx, tanfovy=s.tanfovy,
                           bg=s.bg, scale_modifier=s.scale_modifier, viewmatrix=s.viewmatrix, projmatrix=s.projmatrix,
                           sh_degree=s.sh_degree, campos=s.campos, prefiltered=s.prefiltered, debug=s.debug)
    return ro.rasterize(means3D=means3D, means2D=means2D, opacities=opacities, shs=sh, colors_precomp=colors_precomp, scales=scales,
                        rotations=rotations, cov3D_precomp=cov3Ds_precomp, settings=so)


@pytest.mark.parametrize('name', ['c1', 'w540'])
def test_this_packages_renderer_builds_the_reference_callers_settings(golden, name):
    assets, shape, cam, bg = _case(golden, name)
    p = name + '_'
    job = renderer._raster_job(assets, shape, cam, bg)
    s = job['raster_settings']
    assert type(s).__name__ == 'GaussianRasterizationSettings' and s._fields == (
        'image_height', 'image_width', 'tanfovx', 'tanfovy', 'bg', 'scale_modifier', 'viewmatrix', 'projmatrix', 'sh_degree',
        'campos', 'prefiltered', 'debug')
    want = golden[p + 'settings_scalars']
    got = np.array([s.image_height, s.image_width, s.tanfovx, s.tanfovy, s.scale_modifier, s.sh_degree, float(s.prefiltered),
                    float(s.debug)], dtype=np.float64)
    assert np.array_equal(got, want)                                        # tan(fov / 2): the same Python floats
    assert bool(golden[p + 'settings_tan_is_float']) and isinstance(s.tanfovx, float) and isinstance(s.tanfovy, float)
    assert np.array_equal(s.viewmatrix.numpy(), golden[p + 'viewmatrix'])
    assert np.array_equal(s.projmatrix.numpy(), golden[p + 'projmatrix'])
    assert np.array_equal(s.campos.numpy(), golden[p + 'campos'])
    assert np.array_equal(s.bg.numpy(), golden[p + 'bg'])                  # incl. the default white one
    # the keyword arguments the reference passes (module.py:632-640) are the ones this package's forward takes
    passed = sorted(k for k in job if k not in ('raster_settings', 'densify_stats', 'frozen'))
    assert passed == list(golden[p + 'kwargs'])
    assert job['means2D'].is_leaf and job['means2D'].requires_grad and bool(golden[p + 'mean_2d_is_leaf'])
    assert tuple(job['means2D'].shape) == (assets['mean_3d'].shape[0], 3) and float(job['means2D'].detach().abs().max()) == 0.0


@pytest.mark.parametrize('name', ['c1', 'w540'])
def test_the_oracles_renderer_twin_reproduces_the_reference_callers_outputs(golden, name):
    assets, shape, cam, bg = _case(golden, name)
    p = name + '_'
    a = {k: v.clone().requires_grad_(True) for k, v in assets.items()}
    out = ro.render(a, shape, cam, bg)
    (out['img'] * torch.from_numpy(golden[p + 'G'])).sum().backward()
    assert sorted(out) == ['depthmap', 'img', 'is_vis', 'mask', 'mean_2d', 'radius']
    for k in ('img', 'depthmap', 'mask', 'radius', 'is_vis'):
        assert np.array_equal(out[k].detach().numpy(), golden[p + k]), k
    assert np.array_equal(out['mean_2d'].grad.numpy(), golden[p + 'mean_2d_grad'])
    for k in assets:
        assert np.array_equal(a[k].grad.numpy(), golden[p + 'grad_' + k]), k


@pytest.mark.parametrize('name', ['c1', 'w540'])
def test_this_packages_renderer_returns_what_the_reference_renderer_returned(golden, name, monkeypatch):
    """"``GaussianRenderer.forward`` from module.py:592-647 runs unmodified against it".  The fixture
    holds what the reference's class, exec'd unchanged by ``tests/golden/make_golden_renderer.py``, returned for these inputs
    with the CPU oracle behind the rasterizer; here ``exa.GaussianRenderer`` gets the same inputs with the rasterizer's device
    call replaced by the same oracle (no GPU here; on the GPU box tests/test_gpu_reference_renderer.py holds the HIP path
    against the fixture) and must return the same six keys, bit for bit, and the same gradients."""
    monkeypatch.setattr(rasterizer, 'rasterize_gaussians', _oracle_rasterize)
    monkeypatch.setattr(renderer, 'rasterize_gaussians', _oracle_rasterize)
    assets, shape, cam, bg = _case(golden, name)
    p = name + '_'
    a = {k: v.clone().requires_grad_(True) for k, v in assets.items()}
    rend = exa.GaussianRenderer()
    out = rend(a, shape, cam) if bg is None else rend(a, shape, cam, bg)
    (out['img'] * torch.from_numpy(golden[p + 'G'])).sum().backward()
    assert sorted(out) == ['depthmap', 'img', 'is_vis', 'mask', 'mean_2d', 'radius']
    for k in ('img', 'depthmap', 'mask', 'radius', 'is_vis'):
        assert np.array_equal(out[k].detach().numpy(), golden[p + k]), k
    assert out['mean_2d'].is_leaf and out['mean_2d'].requires_grad and bool(golden[p + 'mean_2d_is_leaf'])
    assert np.array_equal(out['mean_2d'].grad.numpy(), golden[p + 'mean_2d_grad'])
    for k in assets:
        assert np.array_equal(a[k].grad.numpy(), golden[p + 'grad_' + k]), k
