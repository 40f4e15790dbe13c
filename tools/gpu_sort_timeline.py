"""Developer probe (library built with -DEXA_PROBE_SORTLINE): start / end of every workgroup of the sort launch (100 MHz
clock) against the length of its list(s); the ordering workgroups come first.  C3, forward only.
Usage: python tools/gpu_sort_timeline.py [--wave-keys 0|256|512] [view ...]     (--wave-keys: the EXA_WAVE_KEYS of the library;
0 = one workgroup per sub-tile, sort_subtiles_kernel; otherwise the grid of sort_subtiles_quads_kernel: ordering workgroups,
quads of four one-wave lists, tail workgroups: one per WAVE_KEYS / 64 + 1 batch slots, one long list at most each)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch, numpy as np
import exavatar_release_amd as exa
from exavatar_release_amd import scenes
from exavatar_release_amd.rasterizer import GaussianRasterizationSettings, rasterize_gaussians, _debug_last
from exavatar_release_amd.camera import make_raster_matrices
from _layout import tile_offsets, bin_offsets
OW = 32          # ORDER_WGS of csrc/render_fwd.hip
argv = sys.argv[1:]
WK = 512         # EXA_WAVE_KEYS of csrc/common.h
if argv and argv[0] == '--wave-keys':
    WK = int(argv[1]); argv = argv[2:]
dev = torch.device('cuda:0'); H = W = 1024; P = 150000
assets = scenes.dist_b_avatar(P, seed=0)
params = [assets[k].to(dev) for k in ('mean_3d', 'scale', 'rotation', 'opacity', 'rgb')]
exa.config.mode = 'exact'; exa.config.keep_debug = True
lay = tile_offsets(P, W, H); cells = lay['cells']; nsub = cells * 64


def pct(v, qs):
    return [np.percentile(v, q) for q in qs]


for k in [int(v) for v in (argv or [0, 50])]:
    tanx, tany, view, proj, cpos = make_raster_matrices(scenes.ring_camera(H, W, k, 200), (H, W))
    st = GaussianRasterizationSettings(H, W, tanx, tany, torch.ones(3, device=dev), 1.0, view.to(dev), proj.to(dev), 0, cpos.to(dev), False, False)
    m3, sc, rot, op, rgb = params
    with torch.no_grad():
        for _ in range(3):
            rasterize_gaussians(m3, torch.zeros(P, 3, device=dev), None, rgb, op, sc, rot, None, st)
    torch.cuda.synchronize()
    tile = _debug_last['tile']; cap = int(_debug_last['capacity'])
    quads = nsub // 4
    S = WK // 64 + 1                     # batch slots per tail workgroup
    tail = (cap // 64 + S - 1) // S if WK else 0
    nwg = OW + (quads + tail if WK else nsub)
    assert nwg <= nsub + OW, 'the stamps of the ordering workgroups lie behind those of %d workgroups' % (nsub + OW)
    desc = tile[lay['cell_desc'][0]: lay['cell_desc'][0] + lay['cell_desc'][1]].view(torch.int32).view(-1, 4).cpu().numpy().astype(np.int64)
    rng = tile[lay['ranges'][0]: lay['ranges'][0] + nsub * 8].view(torch.int32).view(-1, 2).cpu().numpy().astype(np.int64)
    tt = tile[lay['part_cnt'][0]: lay['part_cnt'][0] + nwg * 8].view(torch.int32).view(-1, 2).cpu().numpy().astype(np.int64) & 0xffffffff
    start, end = tt[:, 0] * 0.01, tt[:, 1] * 0.01
    # in cell_desc order: entry w is sub-tile (w & 63) of the cell of rank (w >> 6)
    wg = np.arange(nsub)
    stile = desc[wg >> 6, 0] * 64 + (wg & 63)
    n_all = rng[:, 1] - rng[:, 0]
    n = n_all[stile]
    if WK:        # a quad works when one of its four lists fits a wave; tail workgroup t when batch slot t * S is the first
        #           such slot of a list longer than WK (the owner records of the bin workspace say whose slot it is)
        o = bin_offsets(cap)['owner'][0]
        owner = _debug_last['bin'][o: o + (cap // 64 + 1) * 16].view(torch.int32).view(-1, 4).cpu().numpy().astype(np.int64)[0:cap // 64:S]
        n4 = n.reshape(-1, 4)
        own = (n4 > 0) & (n4 <= WK)
        qwork, qkeys = own.any(1), (n4 * own).max(1)
        twork = (owner[:, 0] != 0) & (owner[:, 2] > WK) & (np.arange(tail) * S - owner[:, 1] // 64 < S)
        tkeys = owner[:, 2] * twork
        work, keys = np.concatenate([qwork, twork]), np.concatenate([qkeys, tkeys])
    else:
        work, keys = n > 0, n
    t0 = min(start[:OW].min(), start[OW:][work].min())
    start -= t0; end -= t0
    so, eo = start[:OW], end[:OW]
    print('view %d: ordering workgroups start %.2f..%.2f end %.2f..%.2f us' % (k, so.min(), so.max(), eo.min(), eo.max()))
    ph = tile[lay['part_cnt'][0] + (nsub + OW) * 8: lay['part_cnt'][0] + (nsub + OW) * 8 + OW * 8 * 4].view(torch.int32).view(OW, 8).cpu().numpy().astype(np.int64) & 0xffffffff
    ph = ph[:, :6] * 0.01 - t0
    print('   phases of the ordering workgroups (mean end, us after the first start): entry %.2f | histogram %.2f | prefixes %.2f | ranks %.2f | '
          'reservations %.2f | records %.2f' % tuple(ph.mean(0)))
    s_, e_ = start[OW:], end[OW:]
    d = e_ - s_
    groups = [('quad', slice(0, quads)), ('tail', slice(quads, quads + tail))] if WK else [('sorting', slice(0, nsub))]
    for name, sl in groups:
        w_, sg, eg, dg, kg = work[sl], s_[sl], e_[sl], d[sl], keys[sl]
        if not w_.any():
            print('   no %s workgroup with a list (of %d)' % (name, len(w_)))
            continue
        print('   %d %s workgroups with a list (of %d): starts p50 %.2f p90 %.2f max %.2f; ends p50 %.2f p90 %.2f p99 %.2f LAST %.2f us' % (
            w_.sum(), name, len(w_), *pct(sg[w_], (50, 90, 100)), *pct(eg[w_], (50, 90, 99, 100))))
        for lo, hi in ((1, 64), (65, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 1 << 20)):
            m = w_ & (kg >= lo) & (kg <= hi)
            if m.any():
                print('      longest list in [%4d,%5d]: %5d workgroups, duration mean %5.2f max %5.2f us, start mean %5.2f' % (
                    lo, min(hi, kg.max()), m.sum(), dg[m].mean(), dg[m].max(), sg[m].mean()))
        last = np.argsort(-(eg * w_))[:5]
        print('      last to end: ' + '; '.join('%s %d n %d start %.2f dur %.2f' % (name, i, kg[i], sg[i], dg[i]) for i in last))
        idle = ~w_ & (eg > 0)
        print('      without a list: %d, last start %.2f us' % ((~w_).sum(), sg[idle].max() if idle.any() else -1))
