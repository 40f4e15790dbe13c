"""CPU tests of the scene-Gaussian stage's host side: the two entry points are exported and bound, every invalid argument
fails with its negative status and its message before any GPU work, and the Python surface refuses what it does not
support, in the package's order.  The ABI itself (include/exa_raster.h against its binding) is checked by
tests/test_abi.py."""
import ctypes
import sys

import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from exavatar_release_amd.scene_assets import KEYS, REST_ROWS

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2


def test_the_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name, n_args in (('exa_raster_scene_assets_forward', 16), ('exa_raster_scene_assets_backward', 22)):
        assert name in _lib.RASTER.signatures
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    assert lib.exa_raster_version() == 139
    assert build.SOURCES['scene_assets.hip'] == ['-ffp-contract=off']
    module = sys.modules['exavatar_release_amd.scene_assets']
    assert 'scene_assets' in exa.__all__ and exa.scene_assets is module.scene_assets
    assert KEYS == ('mean_3d', 'opacity', 'scale', 'rotation', 'rgb') and REST_ROWS == (0, 3, 8, 15)


def _fwd(lib, P=5, Mr=15, deg=3, **null):
    names = ('mean', 'opacity', 'scale', 'rotation', 'dc', 'rest', 'R', 't', 'o_opacity', 'o_scale', 'o_rotation', 'o_rgb')
    return lib.exa_raster_scene_assets_forward(P, Mr, deg, *[None if null.get(n) else BAD for n in names], None)


def _bwd(lib, P=5, Mr=15, deg=3, **null):
    names = ('mean', 'rotation', 'dc', 'rest', 'R', 't', 'y_opacity', 'y_scale', 'c_opacity', 'c_scale', 'c_rotation',
             'c_rgb', 'g_mean', 'g_opacity', 'g_scale', 'g_rotation', 'g_dc', 'g_rest')
    return lib.exa_raster_scene_assets_backward(P, Mr, deg, *[None if null.get(n) else BAD for n in names], None)


@pytest.mark.parametrize('call', [_fwd, _bwd], ids=['forward', 'backward'])
def test_a_negative_P_and_bad_sizes_are_rejected_on_the_host(call):
    lib = _lib.load()
    err = lib.exa_raster_last_error
    assert call(lib, P=-1) < 0
    assert err().startswith(b'exa_raster: ') and b'P < 0' in err()
    for Mr in (-1, 1, 2, 4, 7, 9, 14, 16, 24):
        assert call(lib, Mr=Mr, deg=0) == INVALID and b'Mr (rows of feature_rest) must be 0, 3, 8 or 15' in err()
    for deg in (-1, 4):
        assert call(lib, deg=deg) == INVALID and b'sh_degree must be 0 .. 3' in err()
    for Mr, deg in ((0, 1), (3, 2), (8, 3), (0, 3)):
        assert call(lib, Mr=Mr, deg=deg) == INVALID and b'(sh_degree + 1)^2 <= 1 + Mr' in err()
    assert call(lib, P=0) == 0                      # nothing to do
    assert call(lib, P=0, Mr=5) == INVALID          # the sizes are still checked


def test_forward_rejects_null_arrays():
    lib = _lib.load()
    err = lib.exa_raster_last_error
    for n in ('mean', 'opacity', 'scale', 'rotation', 'dc', 'rest'):
        assert _fwd(lib, **{n: True}) == NULLPTR and b'a parameter array is NULL' in err(), n
    for n in ('R', 't'):
        assert _fwd(lib, **{n: True}) == NULLPTR and b'cam_R / cam_t is NULL' in err(), n
    for n in ('o_opacity', 'o_scale', 'o_rotation', 'o_rgb'):
        assert _fwd(lib, **{n: True}) == NULLPTR and b'an output array is NULL' in err(), n


def test_backward_rejects_what_a_requested_gradient_needs():
    lib = _lib.load()
    err = lib.exa_raster_last_error
    nothing = dict(g_mean=True, g_opacity=True, g_scale=True, g_rotation=True, g_dc=True, g_rest=True)
    assert _bwd(lib, **nothing) == 0                                      # no gradient wanted: a successful no-op
    assert _bwd(lib, Mr=0, deg=0, **dict(nothing, g_rest=False)) == 0     # Mr = 0: grad_feature_rest has no elements
    only = lambda keep, **null: _bwd(lib, **dict({k: v for k, v in nothing.items() if k != keep}, **null))      # noqa: E731
    assert only('g_opacity', y_opacity=True) == NULLPTR and b'grad_opacity needs opacity_out' in err()
    assert only('g_scale', y_scale=True) == NULLPTR and b'grad_scale needs scale_out' in err()
    assert only('g_rotation', rotation=True) == NULLPTR and b'grad_rotation needs rotation' in err()
    for g in ('g_mean', 'g_dc', 'g_rest'):
        for n in ('mean', 'dc', 'rest', 'R', 't'):
            assert only(g, **{n: True}) == NULLPTR and b'the colour gradients need' in err(), (g, n)


def _args(P=6, Mr=15):
    z = torch.zeros
    return dict(mean=z(P, 3), opacity=z(P, 1), scale=z(P, 3), rotation=z(P, 6), feature_dc=z(P, 1, 3),
                feature_rest=z(P, Mr, 3), sh_degree=3 if Mr == 15 else 0, cam_param={'R': torch.eye(3), 't': z(3)})


def test_python_surface_raises_as_specified():
    sa = exa.scene_assets
    with pytest.raises(RuntimeError, match=r'scene_assets runs on a ROCm device only \(no CPU path\)'):
        sa(**_args())
    for name in ('mean', 'opacity', 'scale', 'rotation', 'feature_dc', 'feature_rest'):
        a = _args()
        with pytest.raises(TypeError, match='scene_assets: %s must be a tensor' % name):
            sa(**dict(a, **{name: a[name].numpy()}))
        with pytest.raises(ValueError, match=r'scene_assets: %s must be float32 \(it is torch.float64\)' % name):
            sa(**dict(a, **{name: a[name].double()}))
    for bad in (torch.tensor(3), 3.0, True, None):
        with pytest.raises(TypeError, match='scene_assets: sh_degree must be a host int'):
            sa(**dict(_args(), sh_degree=bad))
    for bad in (None, {'R': torch.eye(3)}, {'t': torch.zeros(3)}):
        with pytest.raises(TypeError, match="scene_assets: cam_param must be a dict with 'R' and 't'"):
            sa(**dict(_args(), cam_param=bad))
    with pytest.raises(TypeError, match=r"scene_assets: cam_param\['R'\] must be a tensor"):
        sa(**dict(_args(), cam_param={'R': torch.eye(3).numpy(), 't': torch.zeros(3)}))
    with pytest.raises(ValueError, match=r"scene_assets: cam_param\['t'\] must be float32"):
        sa(**dict(_args(), cam_param={'R': torch.eye(3), 't': torch.zeros(3).double()}))
    with pytest.raises(ValueError, match=r'scene_assets: mean must be \[P, 3\] \(it has \(6, 2\)\)'):
        sa(**dict(_args(), mean=torch.zeros(6, 2)))
    with pytest.raises(ValueError, match=r'scene_assets: opacity must be \[P, 1\] with P = 6 \(it has \(6,\)\)'):
        sa(**dict(_args(), opacity=torch.zeros(6)))
    with pytest.raises(ValueError, match=r'scene_assets: scale must be \[P, 3\] with P = 6'):
        sa(**dict(_args(), scale=torch.zeros(5, 3)))
    with pytest.raises(ValueError, match=r'scene_assets: rotation must be \[P, 6\] with P = 6 \(it has \(6, 4\)\)'):
        sa(**dict(_args(), rotation=torch.zeros(6, 4)))
    with pytest.raises(ValueError, match=r'scene_assets: feature_dc must be \[P, 1, 3\] with P = 6'):
        sa(**dict(_args(), feature_dc=torch.zeros(6, 3)))
    for shape in ((6, 14, 3), (6, 15, 4), (5, 15, 3), (6, 45)):
        with pytest.raises(ValueError, match=r'scene_assets: feature_rest must be \[P, Mr, 3\] with P = 6 and Mr in '
                                             r'\(0, 3, 8, 15\)'):
            sa(**dict(_args(), feature_rest=torch.zeros(shape)))
    for bad in (-1, 4):
        with pytest.raises(ValueError, match=r'scene_assets: sh_degree must be 0 .. 3 \(it is %d\)' % bad):
            sa(**dict(_args(), sh_degree=bad))
    with pytest.raises(ValueError, match=r'scene_assets: sh_degree 2 needs 8 rows of feature_rest \(it has 3\)'):
        sa(**dict(_args(Mr=3), sh_degree=2))
    with pytest.raises(ValueError, match=r"scene_assets: cam_param\['R'\] must be \[3, 3\] \(it has \(4, 4\)\)"):
        sa(**dict(_args(), cam_param={'R': torch.eye(4), 't': torch.zeros(3)}))
    with pytest.raises(ValueError, match=r"scene_assets: cam_param\['t'\] must hold 3 elements"):
        sa(**dict(_args(), cam_param={'R': torch.eye(3), 't': torch.zeros(4)}))
    for key in ('R', 't'):
        cam = {'R': torch.eye(3), 't': torch.zeros(3)}
        cam[key] = cam[key].requires_grad_(True)
        with pytest.raises(ValueError, match=r"scene_assets: cam_param\['%s'\] is camera data in the reference and gets no "
                                             r'gradient; detach it' % key):
            sa(**dict(_args(), cam_param=cam))


def test_checks_run_in_the_packages_order():
    """Tensor before dtype before shape before the device: an argument wrong in several ways reports the first."""
    sa = exa.scene_assets
    a = _args()
    with pytest.raises(TypeError, match='rotation must be a tensor'):                   # a later argument's type ...
        sa(**dict(a, mean=torch.zeros(6, 2), rotation=None))                            # ... before an earlier one's shape
    with pytest.raises(ValueError, match='scale must be float32'):
        sa(**dict(a, mean=torch.zeros(6, 2), scale=a['scale'].half()))
    with pytest.raises(ValueError, match=r'mean must be \[P, 3\]'):                     # the shape before the device
        sa(**dict(a, mean=torch.zeros(6, 2)))
