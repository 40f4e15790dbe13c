"""GPU test of the gradient arrays the Python autograd nodes hand out, for every pattern of inputs that ask for one.

The backward of a render carves the gradients it was asked for out of one arena and gives the kernels a null pointer for
every other one (``rasterizer._grad_arena``), so which inputs require grad decides the layout of the memory the kernels
write.  What they write must not depend on it: with ONE input requiring grad, its gradient is the one the run with EVERY
input requiring grad returned, bit for bit, and no other input receives one.  Checked for the four kinds of input a render
takes (colours or SH with scales / rotations, colours with a precomputed covariance, and a loss that reads colour, depth
and alpha instead of colour alone), on a single render, a K = 2 batch of different Gaussians and a composite of a
``keep_keys`` pair with its gradients folded into source B's backward or summed by autograd."""
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import rasterizer as rz
from exavatar_release_amd import scenes
from exavatar_release_amd.camera import make_raster_matrices

pytestmark = pytest.mark.gpu

P, H, W, F = 64, 32, 48, 40.0
KINDS = ('colors', 'sh', 'cov', 'planes')      # 'planes': the inputs of 'colors', the loss reads colour + depth + alpha


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from exavatar_release_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _cov6(scale, q):
    """Upper triangle (xx, xy, xz, yy, yz, zz) of R diag(scale)^2 R^T, quaternion (r, x, y, z)."""
    r, x, y, z = q.unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), 1).view(-1, 3, 3)
    M = R * scale[:, None, :]
    S = M @ M.transpose(1, 2)
    return torch.stack((S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]), 1).contiguous()


def _inputs(kind, seed, dev):
    """The eight tensor arguments of one render (``rz._IN_NAMES``), None for the ones this kind does not pass."""
    a = scenes.dist_a_random(P, H, W, seed=seed, focal=F)
    d = dict.fromkeys(rz._IN_NAMES)
    d['means3D'], d['opacities'] = a['mean_3d'], a['opacity']
    d['means2D'] = torch.zeros(P, 3)
    if kind == 'sh':
        d['shs'] = scenes.sh_from_rgb(a['rgb'], 1, seed=seed)
    else:
        d['colors_precomp'] = a['rgb']
    if kind == 'cov':
        d['cov3D_precomp'] = _cov6(a['scale'], a['rotation'])
    else:
        d['scales'], d['rotations'] = a['scale'], a['rotation']
    return {n: None if t is None else t.to(dev) for n, t in d.items()}


def _settings(kind, dev):
    tanx, tany, view, proj, campos = make_raster_matrices(scenes.neutral_camera(H, W, focal=F), (H, W))
    bg = torch.rand(3, generator=torch.Generator().manual_seed(5)).to(dev)
    return exa.GaussianRasterizationSettings(H, W, tanx, tany, bg, 1.0, view.to(dev), proj.to(dev), 1 if kind == 'sh' else 0,
                                             campos.to(dev), False, False)


def _single(sets, st):
    (a,) = sets
    return [exa.GaussianRasterizer(st)(means3D=a['means3D'], means2D=a['means2D'], opacities=a['opacities'], shs=a['shs'],
                                       colors_precomp=a['colors_precomp'], scales=a['scales'], rotations=a['rotations'],
                                       cov3D_precomp=a['cov3D_precomp'])]


def _batch(sets, st):
    return rz.rasterize_gaussians_batch([dict(raster_settings=st, **a) for a in sets])


def _composite(sets, st):
    a, b, probe = sets
    outs, handles = rz.rasterize_gaussians_batch([dict(raster_settings=st, **a), dict(raster_settings=st, **b)], keep_keys=True)
    comp = rz.rasterize_composites([(handles[0], handles[1])], [dict(raster_settings=st, **dict(b, means2D=probe['means2D']))],
                                   token=handles.token)
    return outs + comp


def _run(sets, on, render, st, planes, G):
    """Gradient (or None) of every input of ``sets`` after one forward + backward in which the inputs ``on`` require grad."""
    leaves = [{n: None if t is None else t.clone().requires_grad_((s, n) in on) for n, t in d.items()} for s, d in enumerate(sets)]
    outs, grads = [], []
    for k, (color, _radii, depth, alpha) in enumerate(render(leaves, st)):
        for img, g in ((color, G[k, :3]), (depth, G[k, 3:4]), (alpha, G[k, 4:5]))[:3 if planes else 1]:
            if img.requires_grad:             # (a render none of whose inputs asks for a gradient is a constant)
                outs.append(img)
                grads.append(g)
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    return {(s, n): t.grad for s, d in enumerate(leaves) for n, t in d.items() if t is not None}


SURFACES = {'single': (_single, 1), 'batch': (_batch, 2), 'composite_folded': (_composite, 2), 'composite_summed': (_composite, 2)}


@pytest.mark.parametrize('surface', list(SURFACES))
@pytest.mark.parametrize('kind', KINDS)
def test_one_input_alone_gets_the_gradient_of_the_all_on_run(dev, kind, surface):
    exa.config.compiled_node = 'off'
    exa.config.fold_composite_grads = surface != 'composite_summed'
    render, n_sets = SURFACES[surface]
    inputs_kind = 'colors' if kind == 'planes' else kind
    sets = [_inputs(inputs_kind, 11 + s, dev) for s in range(n_sets)]
    if render is _composite:
        sets.append({'means2D': torch.zeros(P, 3, device=dev)})        # the composite's own screen-space probe
    st = _settings(kind, dev)
    G = torch.randn(3, 5, H, W, generator=torch.Generator().manual_seed(7)).to(dev)
    present = [(s, n) for s, d in enumerate(sets) for n, t in d.items() if t is not None]
    full = _run(sets, set(present), render, st, kind == 'planes', G)
    assert all(full[k] is not None and full[k].shape == sets[k[0]][k[1]].shape for k in present)
    assert all(float(full[k].abs().sum()) > 0 for k in present)          # real gradients, every one of them
    singles = present
    if render is _composite:
        # the composite's own inputs: source B's tensors and its probe.  (With only an input of the plain batch on -- source
        # A's, or a probe of the batch -- the composite stores no context, yet its image requires grad through the token of
        # the batch and its backward refuses to run: such a loss does not read the composite; the 'batch' surface covers
        # those inputs.)
        singles = [(s, n) for s, n in present if (s == 1 and n != 'means2D') or s == 2]
    for one in singles:
        got = _run(sets, {one}, render, st, kind == 'planes', G)
        for k in present:
            if k == one:
                assert torch.equal(got[k], full[k]), (one,)
            else:
                assert got[k] is None, (one, k)
