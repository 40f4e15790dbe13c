"""One densification of the scene set on the MI355X, by HIP events: the single-pass plan and move of csrc/densify.hip
against the two torch expressions a user has today, all on the same device over the same tensors.

  sizes        the bench's scene size (100 000 Gaussians) and one ten times larger, SH degree 3: the six parameters (rows of
               3, 3, 45, 1, 3 and 6 floats) and their twelve Adam moments.
  row mix      ASSUMED, in the proportions the soak test sees on its synthetic scene, not measured on a capture: 6 % of the
               rows cloned, 6 % split (a tenth of them too wide to keep their children), 4 % transparent, the rest kept.
  hip_plan     densify_plan: classify + scan, between two events (its read-back of 16 bytes is outside the events).
  hip_move     densify_apply over the eighteen tensors: one launch.
  hip_wall     host clock of SceneGaussian.densify_and_prune as a whole (plan, the one synchronisation, noise, move, the
               optimizer's re-keying), ending in a device synchronise.
  three_pass   the reference's expression restated in torch on the device: clone, split and prune one after the other with
               boolean masks and cat over the eighteen tensors (avatar/common/nets/module.py:17-56,159-245, without its
               empty_cache()), between two events and by the host clock.
  restated     exavatar_release_amd.densify.densify_and_prune (the torch restatement the soak test uses; quaternions).

Every figure is the median of --reps runs with its min and max; every run starts from a fresh copy of the same state.
The comparison is between these expressions on one device in one process, never against an earlier run of this code.
Prints one JSON line; --out writes it to a file too.

    python tools/gpu_densify_times.py [--reps 9] [--out densify_times.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import exavatar_release_amd as exa                              # noqa: E402
from exavatar_release_amd import densify, p3d_standins          # noqa: E402

PARAMS = ('mean', 'feature_dc', 'feature_rest', 'opacity', 'scale', 'rotation')
SHAPES = {'mean': (3,), 'feature_dc': (1, 3), 'feature_rest': (15, 3), 'opacity': (1,), 'scale': (3,), 'rotation': (6,)}
MIX = {'clone': 0.06, 'split': 0.06, 'transparent': 0.04}      # ASSUMED (module docstring)
EXTENT, GRAD_THR, SCREEN = 5.0, 0.0002, 20


def make_state(P, seed=0):
    rs = np.random.RandomState(seed)
    u = rs.rand(P)
    clone, split = u < MIX['clone'], (u >= MIX['clone']) & (u < MIX['clone'] + MIX['split'])
    top = np.where(split, np.where(rs.rand(P) < 0.1, rs.uniform(0.9, 2.0, P), rs.uniform(0.06, 0.45, P)), rs.uniform(0.01, 0.04, P))
    frac = rs.uniform(0.05, 1.0, (P, 3))
    frac[np.arange(P), rs.randint(0, 3, P)] = 1.0
    f = lambda x: torch.from_numpy(np.asarray(x, np.float32))      # noqa: E731
    state = {'scale': f(np.log(top[:, None] * frac)),
             'opacity': f(np.where(rs.rand(P) < MIX['transparent'], -7.0, rs.uniform(-4, 5, P)))[:, None],
             'xyz_grad_accum': f(np.where(clone | split, 0.001, 0.00005))[:, None], 'track_cnt': torch.ones(P, 1),
             'radius_max': f(rs.randint(0, 41, P))}
    for k in PARAMS:
        if k not in state:
            state[k] = torch.randn((P,) + SHAPES[k])
        state['exp_avg_' + k], state['exp_avg_sq_' + k] = torch.randn_like(state[k]), torch.rand_like(state[k])
    return state


def fresh_scene(state, dev, hip):
    P = state['mean'].shape[0]
    scene = exa.SceneGaussian()
    scene.init_from_point_num(P, device=dev)
    with torch.no_grad():
        for k in PARAMS:
            getattr(scene, k).copy_(state[k])
        for k in ('xyz_grad_accum', 'track_cnt', 'radius_max'):
            getattr(scene, k).copy_(state[k])
        scene.cam_dist_radius[:] = EXTENT
    opt = (exa.Adam if hip else torch.optim.Adam)(scene.get_optimizable_params(), lr=0.0, eps=1e-15)
    for k in PARAMS:
        opt.state[getattr(scene, k)] = {'step': torch.tensor(5.0), 'exp_avg': state['exp_avg_' + k].to(dev),
                                        'exp_avg_sq': state['exp_avg_sq_' + k].to(dev)}
    return scene, opt


def three_pass(scene, opt, noise_gen):
    """The reference's clone_points, split_points and final prune, restated: masks, cat and boolean indexing per tensor."""
    names = {k + '_scene': k for k in PARAMS}

    def cat(new):
        for g in opt.param_groups:
            k = names[g['name']]
            st = opt.state.pop(g['params'][0])
            st['exp_avg'] = torch.cat((st['exp_avg'], torch.zeros_like(new[k])))
            st['exp_avg_sq'] = torch.cat((st['exp_avg_sq'], torch.zeros_like(new[k])))
            g['params'][0] = torch.nn.Parameter(torch.cat((g['params'][0], new[k])).requires_grad_(True))
            opt.state[g['params'][0]] = st
            setattr(scene, k, g['params'][0])
        n = scene.mean.shape[0]
        dev = scene.mean.device
        scene.radius_max, scene.xyz_grad_accum, scene.track_cnt = (torch.zeros(n, device=dev), torch.zeros(n, 1, device=dev),
                                                                   torch.zeros(n, 1, device=dev))

    def prune(drop):
        valid = ~drop
        for g in opt.param_groups:
            k = names[g['name']]
            st = opt.state.pop(g['params'][0])
            st['exp_avg'], st['exp_avg_sq'] = st['exp_avg'][valid], st['exp_avg_sq'][valid]
            g['params'][0] = torch.nn.Parameter(g['params'][0][valid].requires_grad_(True))
            opt.state[g['params'][0]] = st
            setattr(scene, k, g['params'][0])
        scene.radius_max, scene.xyz_grad_accum, scene.track_cnt = (scene.radius_max[valid], scene.xyz_grad_accum[valid],
                                                                   scene.track_cnt[valid])

    with torch.no_grad():
        grad = torch.nan_to_num(scene.xyz_grad_accum / scene.track_cnt)
        P0 = grad.shape[0]
        mask = (grad[:, 0] >= GRAD_THR) & (torch.max(torch.exp(scene.scale), 1).values <= 0.01 * scene.cam_dist_radius)
        cat({k: getattr(scene, k)[mask] for k in PARAMS})
        padded = torch.zeros(scene.mean.shape[0], device=grad.device)
        padded[:P0] = grad[:, 0]
        mask = (padded >= GRAD_THR) & (torch.max(torch.exp(scene.scale), 1).values > 0.01 * scene.cam_dist_radius)
        std = torch.exp(scene.scale)[mask, :].repeat(2, 1)
        samples = torch.randn(std.shape, generator=noise_gen, device=std.device) * std
        R = p3d_standins.rotation_6d_to_matrix(scene.rotation[mask, :]).repeat(2, 1, 1)
        new = {k: getattr(scene, k)[mask].repeat(2, *([1] * (getattr(scene, k).dim() - 1))) for k in PARAMS}
        new['mean'] = torch.bmm(R, samples[:, :, None])[:, :, 0] + scene.mean[mask, :].repeat(2, 1)
        new['scale'] = torch.log(torch.exp(scene.scale)[mask, :].repeat(2, 1) / (0.8 * 2))
        n_new = new['mean'].shape[0]
        cat(new)
        prune(torch.cat((mask, torch.zeros(n_new, dtype=torch.bool, device=mask.device))))
        drop = (torch.sigmoid(scene.opacity) < 0.005)[:, 0]
        drop = drop | (scene.radius_max > SCREEN) | (torch.max(torch.exp(scene.scale), 1).values > 0.1 * scene.cam_dist_radius)
        prune(drop)
    return scene.mean.shape[0]


def restated(state, dev, gen):
    """densify.densify_and_prune over a plain dict with quaternions, as the soak test calls it."""
    params = {k: torch.nn.Parameter(state[k].to(dev)) for k in PARAMS if k != 'rotation'}
    params['rotation'] = torch.nn.Parameter(torch.randn(state['mean'].shape[0], 4, device=dev))
    opt = torch.optim.Adam([{'params': [p], 'name': k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for k, p in params.items():
        opt.state[p] = {'step': torch.tensor(5.0), 'exp_avg': torch.randn_like(p), 'exp_avg_sq': torch.rand_like(p)}
    accum, cnt = state['xyz_grad_accum'].to(dev), state['track_cnt'].to(dev)

    def call():
        new, *_ = densify.densify_and_prune(params, opt, accum, cnt, grad_thr=GRAD_THR, extent=EXTENT, prune_big=True,
                                            generator=gen)
        return new['mean'].shape[0]
    return call


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), (time.perf_counter() - t0) * 1e3, out


def stats(values):
    v = sorted(values)
    return {'median': round(v[len(v) // 2], 4), 'min': round(v[0], 4), 'max': round(v[-1], 4)}


def measure(P, reps, dev):
    state = make_state(P)
    gen = densify.synchronised_generator(7, dev)
    res = {k: [] for k in ('hip_plan_ms', 'hip_move_ms', 'hip_wall_ms', 'three_pass_event_ms', 'three_pass_wall_ms',
                           'restated_event_ms', 'restated_wall_ms')}
    n_out = {}
    for rep in range(reps + 1):                 # the first run of each warms up and is dropped
        scene, opt = fresh_scene(state, dev, hip=True)
        args = (scene.xyz_grad_accum, scene.track_cnt, scene.scale, scene.opacity, scene.cam_dist_radius)
        kw = dict(grad_thr=GRAD_THR, prune_big=True)
        ev, _, plan = timed(lambda: densify.densify_plan(*args, **kw))
        noise = torch.randn(2 * plan.n_cand, 3, generator=gen, device=dev)
        moments = [opt.state[getattr(scene, k)][m] for k in PARAMS for m in ('exp_avg', 'exp_avg_sq')]
        mv, _, _ = timed(lambda: densify.densify_apply(plan, [scene.feature_dc, scene.feature_rest, scene.opacity],
                                                       mean=scene.mean, scale=scene.scale, rotation=scene.rotation,
                                                       noise=noise, states=moments))
        _, wall, p = timed(lambda: scene.densify_and_prune(SCREEN, opt, generator=gen))
        n_out['hip'] = p.n_out
        scene, opt = fresh_scene(state, dev, hip=False)
        t_ev, t_wall, n_out['three_pass'] = timed(lambda: three_pass(scene, opt, gen))
        r_ev, r_wall, n_out['restated'] = timed(restated(state, dev, gen))
        if rep:
            for k, v in zip(res, (ev, mv, wall, t_ev, t_wall, r_ev, r_wall)):
                res[k].append(v)
        del scene, opt
    out = {k: stats(v) for k, v in res.items()}
    floats = sum(int(np.prod(SHAPES[k])) for k in PARAMS) * 3
    out.update(P=P, n_out=n_out, plan={'n_keep': plan.n_keep, 'n_clone': plan.n_clone, 'n_split': plan.n_split,
                                       'n_cand': plan.n_cand},
               move_bytes_per_s=round((P + plan.n_out) * floats * 4 / (out['hip_move_ms']['median'] * 1e-3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--sizes', type=int, nargs='*', default=[100_000, 1_000_000])
    ap.add_argument('--out')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    result = {'tool': 'gpu_densify_times', 'row_mix_ASSUMED': MIX, 'reps': a.reps,
              'sizes': [measure(P, a.reps, dev) for P in a.sizes]}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
