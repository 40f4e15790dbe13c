"""CPU tests of the LPIPS module's host side: the entry points are exported and bound, both state-dict dialects map onto
the thirteen convolutions, every refusal is raised before the device check (tensor, dtype, shape, then the device), the
C ABI fails invalid arguments on the host, and the transposed, rotated weights of the backward give autograd's input
gradient.  The ABI itself (include/exa_raster.h against its binding) is checked by tests/test_abi.py."""
import ctypes
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from exavatar_release_amd import lpips as lp
from tests import lpips_case as lc

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first
INVALID, NULLPTR = -1, -2
ENTRY_POINTS = (('exa_lpips_workspace_size', 4), ('exa_lpips_tap_layout', 6), ('exa_lpips_trunk_forward', 11),
                ('exa_lpips_trunk_backward', 11), ('exa_lpips_normalize', 5), ('exa_lpips_head_blocks', 1),
                ('exa_lpips_head_forward', 9), ('exa_lpips_head_reduce', 6), ('exa_lpips_head_backward', 9))


def _lpips_state_dict(dialect, duplicate_lins=False, scaling=True):
    convs, lins = lc.weights()
    sd = {}
    for (kw, kb), (w, b) in zip(lp.state_dict_keys(dialect), convs):
        sd[kw], sd[kb] = torch.from_numpy(np.array(w)), torch.from_numpy(np.array(b))
    for t, x in enumerate(lins):
        x = torch.from_numpy(np.array(x)).view(1, -1, 1, 1)
        sd[('lins.%d.model.1.weight' if duplicate_lins else 'lin%d.model.1.weight') % t] = x
    if scaling:
        sd['scaling_layer.shift'] = torch.tensor([-.03, -.088, -.188]).view(1, 3, 1, 1)
        sd['scaling_layer.scale'] = torch.tensor([.458, .448, .45]).view(1, 3, 1, 1)
    return sd


def test_the_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name, n_args in ENTRY_POINTS:
        assert name in _lib.RASTER.signatures
        assert len(getattr(lib, name).argtypes) == n_args
    assert lib.exa_raster_version() == 139
    assert build.SOURCES['lpips.hip'] == ['-ffp-contract=off']
    module = sys.modules['exavatar_release_amd.lpips']
    for name in ('LPIPS', 'lpips_distance'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(module, name)
    assert 'lpips' not in sys.modules and 'torchvision' not in sys.modules


def test_the_workspace_is_the_headers():
    """13 activations (270 floats per crop pixel, pooled sizes floored), the mapped input and two 64-channel gradient
    buffers, every section rounded up to 256 bytes."""
    def want(B, h, w):
        up = lambda n: (n + 63) // 64 * 64      # noqa: E731
        blocks = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
        total = sum(up(B * (h >> blocks[l]) * (w >> blocks[l]) * co) for l, (_, co) in enumerate(lp.CHANNELS))
        return 4 * (total + up(B * h * w * 3) + 2 * up(B * h * w * 64))
    for B, h, w in ((1, 16, 16), (1, 17, 23), (2, 41, 55), (1, 800, 500)):
        assert _lib.lpips_workspace_size(B, h, w) == want(B, h, w)
    assert 107.9e6 < (want(1, 800, 500) // 4 - 131 * 400000) < 108.1e6      # the activations of the 500 x 800 frame
    lib = _lib.load()
    off, shape = ctypes.c_uint64(), (ctypes.c_int32 * 3)()
    assert lib.exa_lpips_tap_layout(1, 17, 23, 4, ctypes.byref(off), shape) == 0 and list(shape) == [1, 1, 512]
    assert lib.exa_lpips_tap_layout(1, 17, 23, 1, ctypes.byref(off), shape) == 0 and list(shape) == [8, 11, 128]
    assert off.value == 4 * (2 * 17 * 23 * 64 + 8 * 11 * 128)
    assert lib.exa_lpips_tap_layout(1, 17, 23, 5, ctypes.byref(off), shape) == INVALID


def test_the_c_abi_checks_its_arguments_on_the_host():
    lib = _lib.load()
    err = lib.exa_raster_last_error
    size = ctypes.c_uint64()
    assert lib.exa_lpips_workspace_size(1, 15, 16, ctypes.byref(size)) == INVALID and b'smaller than 16 x 16' in err()
    assert lib.exa_lpips_workspace_size(1, 16, 15, ctypes.byref(size)) == INVALID
    assert lib.exa_lpips_workspace_size(-1, 16, 16, ctypes.byref(size)) == INVALID and b'negative size' in err()
    assert lib.exa_lpips_workspace_size(1, 16, 16, None) == NULLPTR
    crop = (ctypes.c_int32 * 4)(0, 0, 16, 16)
    ss = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    ptrs = (ctypes.c_void_p * 13)(*[0x1000] * 13)
    big = 1 << 40
    fwd = lambda **k: lib.exa_lpips_trunk_forward(k.get('B', 1), 20, 20, k.get('crop', crop), k.get('img', BAD),      # noqa: E731
                                                  k.get('ss', ss), k.get('w', ptrs), ptrs, BAD, k.get('bytes', big), None)
    assert fwd(crop=None) == NULLPTR and b'crop is NULL' in err()
    assert fwd(crop=(ctypes.c_int32 * 4)(5, 0, 16, 16)) == INVALID and b'crop window outside the image' in err()
    assert fwd(crop=(ctypes.c_int32 * 4)(0, 0, 15, 16)) == INVALID and b'smaller than 16 x 16' in err()
    assert fwd(bytes=1000) == INVALID and b'workspace is smaller' in err()
    assert fwd(img=None) == NULLPTR and b'lpips: NULL argument' in err()
    assert fwd(w=(ctypes.c_void_p * 13)(*([0x1000] * 12 + [None]))) == NULLPTR and b'NULL weight' in err()
    assert fwd(ss=(ctypes.c_float * 6)(0, 0, 0, 1, 0, 1)) == INVALID and b'scale of the input map' in err()
    assert fwd(B=0) == 0
    bwd = lambda **k: lib.exa_lpips_trunk_backward(1, 20, 20, crop, ss, ptrs, k.get('hg', (ctypes.c_void_p * 5)(*[0x1000] * 5)),      # noqa: E731
                                                   BAD, k.get('bytes', big), k.get('dimg', BAD), None)
    assert bwd(bytes=1000) == INVALID
    assert bwd(dimg=None) == NULLPTR
    assert bwd(hg=(ctypes.c_void_p * 5)(0x1000, 0x1000, None, 0x1000, 0x1000)) == NULLPTR and b'NULL head gradient' in err()
    assert lib.exa_lpips_head_forward(1, 15, 6, BAD, BAD, BAD, None, BAD, None) == INVALID and b'multiple of 4' in err()
    assert lib.exa_lpips_head_forward(1, -1, 8, BAD, BAD, BAD, None, BAD, None) == INVALID
    assert lib.exa_lpips_head_forward(1, 15, 8, BAD, BAD, BAD, None, None, None) == NULLPTR
    assert lib.exa_lpips_head_forward(0, 15, 8, None, None, None, None, None, None) == 0
    assert lib.exa_lpips_head_backward(1, 15, 8, BAD, BAD, BAD, None, BAD, None) == NULLPTR
    assert lib.exa_lpips_normalize(4, 7, BAD, BAD, None) == INVALID
    assert lib.exa_lpips_normalize(4, 8, None, BAD, None) == NULLPTR
    assert lib.exa_lpips_head_blocks(257) == 2 and lib.exa_lpips_head_blocks(0) == 0
    one = (ctypes.c_void_p * 1)(0x1000)
    assert lib.exa_lpips_head_reduce(1, 9, one, (ctypes.c_int64 * 1)(4), BAD, None) == INVALID
    assert lib.exa_lpips_head_reduce(1, 1, one, (ctypes.c_int64 * 1)(0), BAD, None) == INVALID
    assert lib.exa_lpips_head_reduce(1, 1, one, (ctypes.c_int64 * 1)(4), None, None) == NULLPTR


@pytest.mark.parametrize('dialect', ['lpips', 'torchvision'])
@pytest.mark.parametrize('duplicate_lins', [False, True])
def test_both_state_dict_dialects_map_onto_the_thirteen_convolutions(dialect, duplicate_lins):
    convs, lins = lc.weights()
    m = exa.LPIPS.from_state_dict(_lpips_state_dict(dialect, duplicate_lins, scaling=dialect == 'lpips'))
    for l, (w, b) in enumerate(convs):
        assert np.array_equal(getattr(m, 'conv%d_weight' % l).numpy(), w) and np.array_equal(getattr(m, 'conv%d_bias' % l).numpy(), b)
    for t, x in enumerate(lins):
        assert np.array_equal(getattr(m, 'lin%d' % t).numpy(), x)
    assert m.shift.tolist() == pytest.approx([-.03, -.088, -.188]) and m.scale.tolist() == pytest.approx([.458, .448, .45])
    keys = lp.state_dict_keys(dialect)
    assert len(keys) == 13
    assert keys[0][0] == ('net.slice1.0.weight' if dialect == 'lpips' else 'features.0.weight')
    assert keys[12][1] == ('net.slice5.28.bias' if dialect == 'lpips' else 'features.28.bias')
    assert keys[4][0] == ('net.slice3.10.weight' if dialect == 'lpips' else 'features.10.weight')
    # the weights are buffers: state_dict carries them (and none of the re-laid copies), .to() converts them
    own = m.state_dict()
    assert len(own) == 13 * 2 + 5 + 2 and not any(k.startswith('_packed') for k in own)
    m2 = exa.LPIPS.from_arrays(*lc.zero_weights())
    m2.load_state_dict(own)
    assert np.array_equal(m2.conv5_weight.numpy(), convs[5][0])


def test_from_state_dict_refuses_by_name():
    sd = _lpips_state_dict('lpips')
    with pytest.raises(KeyError, match='net.slice3.12.bias is missing'):
        exa.LPIPS.from_state_dict({k: v for k, v in sd.items() if k != 'net.slice3.12.bias'})
    with pytest.raises(KeyError, match='lin2.model.1.weight is missing'):
        exa.LPIPS.from_state_dict({k: v for k, v in sd.items() if k != 'lin2.model.1.weight'})
    with pytest.raises(ValueError, match=r'net.slice2.5.weight must be \[128, 64, 3, 3\] \(it has \[128, 64, 3, 1\]\)'):
        exa.LPIPS.from_state_dict(dict(sd, **{'net.slice2.5.weight': sd['net.slice2.5.weight'][..., :1]}))
    with pytest.raises(ValueError, match=r'net.slice1.0.weight must be float32 \(it is torch.float64\)'):
        exa.LPIPS.from_state_dict(dict(sd, **{'net.slice1.0.weight': sd['net.slice1.0.weight'].double()}))
    with pytest.raises(ValueError, match=r'lin4.model.1.weight must be float32'):
        exa.LPIPS.from_state_dict(dict(sd, **{'lin4.model.1.weight': sd['lin4.model.1.weight'].half()}))
    with pytest.raises(ValueError, match=r'scaling_layer.scale must be \[1, 3, 1, 1\]'):
        exa.LPIPS.from_state_dict(dict(sd, **{'scaling_layer.scale': torch.ones(3)}))
    with pytest.raises(TypeError, match='net.slice1.0.bias must be a tensor'):
        exa.LPIPS.from_state_dict(dict(sd, **{'net.slice1.0.bias': sd['net.slice1.0.bias'].numpy()}))
    convs, lins = lc.weights()
    with pytest.raises(ValueError, match=r'convs\[3\] weight must be float32'):
        exa.LPIPS.from_arrays([(w.astype(np.float64), b) if l == 3 else (w, b) for l, (w, b) in enumerate(convs)], lins)
    with pytest.raises(ValueError, match='13 .* pairs and 5 lin weights'):
        exa.LPIPS.from_arrays(convs[:12], lins)


@pytest.fixture(scope='module')
def module():
    return exa.LPIPS.from_arrays(*lc.weights())


def test_forward_refuses_before_the_device_check(module):
    z = torch.zeros
    with pytest.raises(TypeError, match='LPIPS: img_out must be a tensor'):
        module(np.zeros((1, 3, 16, 16), np.float32), z(1, 3, 16, 16))
    with pytest.raises(ValueError, match=r'LPIPS: img_out must be float32 \(it is torch.float64\)'):
        module(z(1, 3, 16, 16).double(), z(1, 3, 16, 16))
    with pytest.raises(ValueError, match=r'LPIPS: img_out must be \[B, 3, H, W\]'):
        module(z(1, 4, 16, 16), z(1, 4, 16, 16))
    with pytest.raises(ValueError, match=r'LPIPS: the crop is 15 x 16 \(h x w\); LPIPS needs at least 16 x 16'):
        module(z(1, 3, 15, 16), z(1, 3, 15, 16))
    with pytest.raises(ValueError, match=r'LPIPS: the crop is 40 x 9 \(h x w\)'):
        module(z(1, 3, 40, 40), z(1, 3, 40, 40), bbox=torch.tensor([[31, 0, 30, 40]]))
    with pytest.raises(ValueError, match=r'LPIPS: img_target must be float32'):
        module(z(1, 3, 16, 16), z(1, 3, 16, 16).half())
    with pytest.raises(ValueError, match='LPIPS: img_target must have the shape of img_out'):
        module(z(1, 3, 16, 16), z(1, 3, 16, 17))
    with pytest.raises(ValueError, match='LPIPS: img_target is data in the reference and gets no gradient; detach it'):
        module(z(1, 3, 16, 16), z(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(ValueError, match='LPIPS: pass img_target or target, not both'):
        module(z(1, 3, 16, 16), z(1, 3, 16, 16), target=[z(1)] * 5)
    with pytest.raises(ValueError, match=r'LPIPS: target\[1\] must be \[1, 8, 8, 128\], the tap of this crop'):
        module(z(1, 3, 16, 16), None, target=[z(1, 16, 16, 64), z(1, 8, 8, 64), z(1, 4, 4, 256), z(1, 2, 2, 512), z(1, 1, 1, 512)])
    with pytest.raises(RuntimeError, match=r'LPIPS runs on a ROCm device only \(no CPU path\)'):
        module(z(1, 3, 16, 16), z(1, 3, 16, 16))
    with pytest.raises(ValueError, match=r'LPIPS.target_features: the crop is 16 x 12'):
        module.target_features(z(1, 3, 16, 12))
    with pytest.raises(ValueError, match='LPIPS.target_features: img_target is data'):
        module.target_features(z(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(RuntimeError, match='ROCm device only'):
        module.target_features(z(1, 3, 16, 16))


def test_lpips_distance_refuses_before_the_device_check():
    f, w = torch.zeros(2, 8, 3, 5), torch.ones(8)
    with pytest.raises(ValueError, match='1 .. 8 taps'):
        exa.lpips_distance([], [], [])
    with pytest.raises(TypeError, match=r'lpips_distance: feats_target\[0\] must be a tensor'):
        exa.lpips_distance([f], [f.numpy()], [w])
    with pytest.raises(ValueError, match=r'lpips_distance: feats_out\[0\] must be float32'):
        exa.lpips_distance([f.double()], [f], [w])
    with pytest.raises(ValueError, match=r'feats_out\[0\] must be \[B, C, h, w\] with C a multiple of 4'):
        exa.lpips_distance([f[:, :6]], [f[:, :6]], [w[:6]])
    with pytest.raises(ValueError, match=r'feats_target\[0\] must have the shape of feats_out\[0\]'):
        exa.lpips_distance([f], [f[:, :, :2]], [w])
    with pytest.raises(ValueError, match=r'lins\[0\] must have 8 elements'):
        exa.lpips_distance([f], [f], [torch.ones(4)])
    with pytest.raises(ValueError, match=r'feats_target\[0\] is data'):
        exa.lpips_distance([f], [f.clone().requires_grad_(True)], [w])
    with pytest.raises(RuntimeError, match=r'lpips_distance runs on a ROCm device only'):
        exa.lpips_distance([f], [f], [w])


@pytest.mark.parametrize('ci,co', [(3, 64), (64, 128)])
def test_the_gradient_weights_give_autograds_input_gradient(ci, co):
    """conv2d(dL/dout, grad_weights(w), padding 1) is autograd's input gradient of conv2d(x, w, padding 1), 5 x 7, to
    float64 round-off: 9 co products of magnitude <= max|g| max|w| per element, each sum reordered at most."""
    rng = np.random.RandomState(7 + ci)
    w = torch.from_numpy(rng.uniform(-1, 1, (co, ci, 3, 3)))
    x = torch.from_numpy(rng.uniform(-1, 1, (2, ci, 5, 7))).requires_grad_(True)
    g = torch.from_numpy(rng.uniform(-1, 1, (2, co, 5, 7)))
    F.conv2d(x, w, padding=1).backward(g)
    wt = lp.grad_weights(w)
    assert tuple(wt.shape) == (ci, co, 3, 3)
    got = F.conv2d(g, wt, padding=1)
    assert (got - x.grad).abs().max().item() <= 9 * co * 2.0 ** -52 * 4


def test_the_packed_image_is_the_headers():
    """[Cout / 64][Cin / 16][tap][g][co][p]: the element at p is input channel 16 chunk + 8 g + 2 (p & 3) + (p >> 2)."""
    co, ci = 128, 32
    w = torch.arange(co * ci * 9, dtype=torch.float32).reshape(co, ci, 3, 3)
    img = lp.pack_weights(w)
    assert tuple(img.shape) == (2, 2, 9, 2, 64, 8)
    for ct, ck, tap, g, o, p in ((0, 0, 0, 0, 0, 0), (1, 1, 5, 1, 17, 6), (0, 1, 8, 0, 63, 3), (1, 0, 2, 1, 1, 4)):
        c = 16 * ck + 8 * g + 2 * (p & 3) + (p >> 2)
        assert img[ct, ck, tap, g, o, p] == w[64 * ct + o, c, tap // 3, tap % 3]
    w1 = torch.arange(64 * 27, dtype=torch.float32).reshape(64, 3, 3, 3)
    assert lp.pack_first(w1)[5, 2, 40] == w1[40, 2, 1, 2]
