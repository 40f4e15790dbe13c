"""Generates tests/golden/ref_mlp.npz by EXECUTING the reference's own ``make_linear_layers``.

``make_linear_layers`` (reference ``avatar/common/nets/layer.py:9-20``) builds the four MLPs of ``HumanGaussian``
(``module.py:279-287``) that ``exavatar_release_amd.FusedMLP`` replaces.  ``layer.py`` cannot be imported here
(pytorch3d, the training config), so the function is cut out of the file with ``ast`` and exec'd UNCHANGED in a
namespace holding ``torch.nn``, as the other golden generators do.  The nets are built at their real widths with it,
given non-trivial GroupNorm affines and float32-representable parameters, and run in float64 on the CPU on small
inputs as the reference calls them (``module.py:459-509, 524-528``: the pose row repeated and concatenated, the heads
applied to the trunk's output); autograd gives every gradient.  The fixture keeps the two nets with a shared pose
block, geo_offset_net (two heads) and rgb_offset_net (a trailing Linear and a per-row normal block), the parameters as
float32 (exact), and of every weight gradient a fixed random sample of entries (shared columns included).  Only inputs,
parameters and results are written -- nothing of the reference's text.

    python tests/golden/make_golden_mlp.py --reference PATH_TO_EXAVATAR_RELEASE
"""
import argparse
import ast
import os
import textwrap

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
TRI, POSE, NORMAL = 96, 126, 3
N = 64
SAMPLES = 2048                    # weight-gradient entries kept per matrix (the fixture stays small)


def reference_make_linear_layers(ref_root):
    path = os.path.join(ref_root, 'avatar', 'common', 'nets', 'layer.py')
    src = open(path).read()
    lines = src.splitlines()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name == 'make_linear_layers':
            ns = {'nn': nn, 'torch': torch}
            exec(textwrap.dedent('\n'.join(lines[node.lineno - 1:node.end_lineno])), ns)
            return ns['make_linear_layers']
    raise RuntimeError('make_linear_layers was not found in ' + path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the ExAvatar_RELEASE checkout')
    args = ap.parse_args()
    mll = reference_make_linear_layers(args.reference)
    torch.manual_seed(0)
    nets = {   # module.py:279-287
        'geo': (mll([TRI, 128, 128, 128], use_gn=True), [mll([128, 3], relu_final=False), mll([128, 1], relu_final=False)],
                ('tri',)),
        'geo_offset': (mll([TRI + POSE, 128, 128, 128], use_gn=True),
                       [mll([128, 3], relu_final=False), mll([128, 1], relu_final=False)], ('tri', 'pose')),
        'rgb': (mll([TRI, 128, 128, 128, 3], relu_final=False, use_gn=True), [], ('tri',)),
        'rgb_offset': (mll([TRI + POSE + NORMAL, 128, 128, 128, 3], relu_final=False, use_gn=True), [],
                       ('tri', 'pose', 'normal')),
    }
    out = {}
    # all four are built, in the reference's order, so that the two kept draw the parameters a full build gives them
    for name in ('geo', 'rgb'):
        del nets[name]
    for name, (trunk, heads, blocks) in nets.items():
        trunk.float()
        for h in heads:
            h.float()
        trunk.double()
        for h in heads:
            h.double()
        for m in trunk:
            if isinstance(m, nn.GroupNorm):
                with torch.no_grad():
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.2, 0.2)
                    m.weight.copy_(m.weight.float().double())
                    m.bias.copy_(m.bias.float().double())
        g = torch.Generator().manual_seed(len(name))
        data = {'tri': torch.randn(N, TRI, generator=g, dtype=torch.float64),
                'pose': torch.randn(1, POSE, generator=g, dtype=torch.float64).repeat(N, 1),
                'normal': torch.nn.functional.normalize(torch.randn(N, NORMAL, generator=g, dtype=torch.float64), dim=1)}
        feat = torch.cat([data[b] for b in blocks], 1).requires_grad_(True)
        h = trunk(feat)
        y = torch.cat([hd(h) for hd in heads], 1) if heads else h
        gout = torch.randn(y.shape, generator=g, dtype=torch.float64)
        y.backward(gout)
        col, per_row, shared = 0, [], []
        for b in blocks:
            w = {'tri': TRI, 'pose': POSE, 'normal': NORMAL}[b]
            (shared if b == 'pose' else per_row).extend(range(col, col + w))
            col += w
        lins = [m for m in trunk if isinstance(m, nn.Linear)]
        gns = [m for m in trunk if isinstance(m, nn.GroupNorm)]
        hl = [m for hd in heads for m in hd if isinstance(m, nn.Linear)] if heads else [lins.pop()]
        f = {'n_layers': len(gns), 'groups': gns[0].num_groups, 'eps': gns[0].eps,
             'per_row_cols': np.array(per_row), 'shared_cols': np.array(shared, dtype=np.int64),
             'x': feat.detach()[:, per_row].numpy(), 'p': data['pose'][0].numpy(), 'gout': gout.numpy(),
             'out': y.detach().numpy(), 'grad_x': feat.grad.numpy(),
             'Wh': torch.cat([m.weight for m in hl]).detach().float().numpy(),
             'bh': torch.cat([m.bias for m in hl]).detach().float().numpy(),
             'grad_Wh': torch.cat([m.weight.grad for m in hl]).numpy(), 'grad_bh': torch.cat([m.bias.grad for m in hl]).numpy()}
        for l, (lin, gn) in enumerate(zip(lins, gns)):
            f['W%d' % l] = lin.weight.detach().float().numpy()
            f['b%d' % l] = lin.bias.detach().float().numpy()
            f['gamma%d' % l] = gn.weight.detach().float().numpy()
            f['beta%d' % l] = gn.bias.detach().float().numpy()
            gW = lin.weight.grad.numpy()
            idx = np.sort(np.random.default_rng(l).choice(gW.size, SAMPLES, replace=False))
            f['grad_W%d_idx' % l] = idx.astype(np.int32)
            f['grad_W%d_val' % l] = gW.ravel()[idx]
            f['grad_b%d' % l] = lin.bias.grad.numpy()
            f['grad_gamma%d' % l] = gn.weight.grad.numpy()
            f['grad_beta%d' % l] = gn.bias.grad.numpy()
        for k, v in f.items():
            out[name + '/' + k] = np.asarray(v)
    path = os.path.join(HERE, 'ref_mlp.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
