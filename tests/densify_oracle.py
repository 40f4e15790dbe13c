"""The reference's densification in numpy: the THREE passes of ``SceneGaussian.densify_and_prune`` (clone, split, prune;
``avatar/common/nets/module.py:159-245`` with the state surgery of ``:17-56``) carried out one after the other with
concatenation and boolean indexing, as the reference does -- not the single pass of ``csrc/densify.hip``, which the tests
compare with this.  Decisions and copied rows are float32; the children's transcendentals are evaluated in float32 and in
float64, and :func:`margins` gives every row's distance from its thresholds in float64.
"""
import numpy as np

F32 = np.float32


def rot6d_to_matrix(a):
    """pytorch3d's rotation_6d_to_matrix in the dtype of ``a`` [N, 6]: rows b1, b2, b3."""
    a1, a2 = a[:, :3], a[:, 3:]
    eps = a.dtype.type(1e-12)
    b1 = a1 / np.maximum(np.sqrt((a1 * a1).sum(1, keepdims=True)), eps)
    c = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    b2 = c / np.maximum(np.sqrt((c * c).sum(1, keepdims=True)), eps)
    return np.stack((b1, b2, np.cross(b1, b2)), 1)


def _grad(accum, cnt):
    with np.errstate(divide='ignore', invalid='ignore'):
        g = accum.reshape(-1).astype(F32) / cnt.reshape(-1).astype(F32)
    return np.nan_to_num(g, nan=0.0, posinf=np.finfo(F32).max, neginf=np.finfo(F32).min).astype(F32)


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))


def margins(scale, opacity, extent, *, dense_percent=0.01, opacity_min=0.005, prune_big=False, split_factor=2):
    """Per row, the smallest relative distance of a transcendental-dependent decision (big, low, and with ``prune_big``
    wide and wide_child) from its threshold, everything but the float32 thresholds themselves evaluated in float64."""
    s = scale.astype(np.float64)
    m = np.exp(s).max(1)
    ext = F32(extent)
    thr_big = np.float64(F32(dense_percent) * ext)
    out = np.abs(m - thr_big) / thr_big
    omin = np.float64(F32(opacity_min))
    out = np.minimum(out, np.abs(_sigmoid(opacity.reshape(-1).astype(np.float64)) - omin) / omin)
    if prune_big:
        thr_wide = np.float64(F32(0.1) * ext)
        out = np.minimum(out, np.abs(m - thr_wide) / thr_wide)
        mc = np.exp(np.log(np.exp(s) / np.float64(F32(0.8 * split_factor)))).max(1)
        out = np.minimum(out, np.abs(mc - thr_wide) / thr_wide)
    return out


def children(mean, scale, rotation, noise, split_factor, dtype):
    """Lines 196-202 of the reference for the candidate rows given (already gathered), in ``dtype``: the means and the
    scales of ``split_factor`` tiled copies.  The divisor is the float32 the reference's tensor division rounds it to."""
    mean, scale, rotation, noise = (x.astype(dtype) for x in (mean, scale, rotation, noise))
    std = np.tile(np.exp(scale), (split_factor, 1))
    samples = noise * std
    R = np.tile(rot6d_to_matrix(rotation), (split_factor, 1, 1))
    mean_new = np.einsum('nij,nj->ni', R, samples) + np.tile(mean, (split_factor, 1))
    scale_new = np.log(std / dtype(F32(0.8 * split_factor)))
    return mean_new, scale_new


def three_passes(params, states, accum, cnt, extent, noise, *, grad_thr, dense_percent=0.01, opacity_min=0.005,
                 screen_size_max=None, split_factor=2, radius_max=None, reference_radius_reset=True, child_dtype=F32):
    """``params``: dict name -> float32 [P0, ...] with 'mean', 'scale', 'rotation', 'opacity' among them; ``states``:
    dict name -> float32 [P0, ...] of optimizer moments (zeros for every row a pass appends).  ``noise``
    [split_factor * n_cand, 3].  Returns ``(new_params, new_states, info)``; ``info`` holds the counts, ``n_cand`` and the
    ``radius_max`` that survives (zeros in the reference's mode), and for every output row its provenance, carried through
    the passes like a parameter: ``source`` (the row of the input it descends from) and ``kind`` (0 an original, 1 a
    clone, 2 + c copy c of a split row).  The children's mean and scale are evaluated in ``child_dtype`` and returned in
    it; everything else is float32."""
    P = {k: np.asarray(v, F32) for k, v in params.items()}
    S = {k: np.asarray(v, F32) for k, v in states.items()}
    ext = F32(extent)
    P0 = P['mean'].shape[0]
    if child_dtype is not F32:
        P['mean'], P['scale'] = P['mean'].astype(child_dtype), P['scale'].astype(child_dtype)
    g = _grad(accum, cnt)
    radius = np.zeros(P0, F32) if (reference_radius_reset or radius_max is None) else np.asarray(radius_max, F32).reshape(-1)

    source, kind = np.arange(P0), np.zeros(P0, np.int64)

    def max_scale():
        return np.exp(P['scale'].astype(F32)).max(1)

    def append(new):
        for k in P:
            P[k] = np.concatenate((P[k], new[k].astype(P[k].dtype)))
        for k in S:
            n = new['mean'].shape[0]
            S[k] = np.concatenate((S[k], np.zeros((n,) + S[k].shape[1:], F32)))

    def prune(drop):
        for k in P:
            P[k] = P[k][~drop]
        for k in S:
            S[k] = S[k][~drop]

    # clone_points
    with np.errstate(invalid='ignore'):
        hot = g >= F32(grad_thr)
        mask = hot & (max_scale() <= F32(dense_percent) * ext)
    n_clone_all = int(mask.sum())
    append({k: v[mask] for k, v in P.items()})
    radius = np.concatenate((radius, np.zeros(n_clone_all, F32)))
    source, kind = np.concatenate((source, source[mask])), np.concatenate((kind, np.ones(n_clone_all, np.int64)))
    # split_points
    padded = np.zeros(P['mean'].shape[0], F32)
    padded[:P0] = g
    with np.errstate(invalid='ignore'):
        mask = (padded >= F32(grad_thr)) & (max_scale() > F32(dense_percent) * ext)
    n_cand = int(mask.sum())
    noise = np.asarray(noise, F32).reshape(split_factor * n_cand, 3)
    mean_new, scale_new = children(P['mean'][mask], P['scale'][mask], P['rotation'][mask], noise, split_factor, child_dtype)
    new = {k: np.tile(v[mask], (split_factor,) + (1,) * (v.ndim - 1)) for k, v in P.items()}
    new['mean'], new['scale'] = mean_new, scale_new
    append(new)
    radius = np.concatenate((radius, np.zeros(split_factor * n_cand, F32)))
    cand_rows = source[mask]
    source = np.concatenate((source, np.tile(cand_rows, split_factor)))
    kind = np.concatenate((kind, 2 + np.repeat(np.arange(split_factor), n_cand)))
    drop = np.concatenate((mask, np.zeros(split_factor * n_cand, bool)))
    prune(drop)
    radius, source, kind = radius[~drop], source[~drop], kind[~drop]
    # the final prune
    drop = _sigmoid(P['opacity'].reshape(-1).astype(F32)) < F32(opacity_min)
    if screen_size_max:
        with np.errstate(invalid='ignore'):
            drop = drop | (radius > F32(screen_size_max)) | (max_scale() > F32(0.1) * ext)
    n_before = drop.shape[0]
    prune(drop)
    radius, source, kind = radius[~drop], source[~drop], kind[~drop]
    info = {'source': source, 'kind': kind, 'cand_rows': cand_rows, 'n_keep': int((kind == 0).sum()),
            'n_clone': int((kind == 1).sum()), 'n_split': int((kind == 2).sum()), 'n_cand': n_cand,
            'n_clone_all': n_clone_all, 'n_pruned': int(drop.sum()), 'n_before_prune': n_before,
            'n_out': P['mean'].shape[0], 'radius_max': radius}
    return P, S, info


KEEP, CLONE, SPLIT, CAND = 1, 2, 4, 8


def codes(accum, cnt, scale, opacity, extent, *, grad_thr, dense_percent=0.01, opacity_min=0.005, prune_big=False,
          split_factor=2, radius_max=None, screen_size_max=None):
    """The decision table of include/exa_raster.h per SOURCE row, float32: what csrc/densify.hip classifies."""
    ext = F32(extent)
    e = np.exp(np.asarray(scale, F32))
    m = e.max(1)
    with np.errstate(invalid='ignore'):
        hot = _grad(accum, cnt) >= F32(grad_thr)
        big = m > F32(dense_percent) * ext
        low = _sigmoid(np.asarray(opacity, F32).reshape(-1)) < F32(opacity_min)
        wide = wide_child = screen = np.zeros(m.shape, bool)
        if prune_big:
            wide = m > F32(0.1) * ext
            wide_child = np.exp(np.log(e / F32(0.8 * split_factor))).max(1) > F32(0.1) * ext
            if radius_max is not None and screen_size_max:
                screen = np.asarray(radius_max, F32).reshape(-1) > F32(screen_size_max)
    return (KEEP * (~(hot & big) & ~low & ~wide & ~screen) + CLONE * (hot & ~big & ~low & ~wide)
            + SPLIT * (hot & big & ~low & ~wide_child) + CAND * (hot & big)).astype(np.uint8)


def single_pass(code, split_factor=2):
    """(source, kind, candidate rank of every output row or -1) of the output the move writes from the codes."""
    rows = np.arange(code.shape[0])
    keep, clone, split = (rows[(code & b) != 0] for b in (KEEP, CLONE, SPLIT))
    cand_rank = np.cumsum((code & CAND) != 0) - 1
    source = np.concatenate([keep, clone] + [split] * split_factor)
    kind = np.concatenate([np.zeros(keep.size, np.int64), np.ones(clone.size, np.int64)]
                          + [np.full(split.size, 2 + c, np.int64) for c in range(split_factor)])
    rank = np.concatenate([np.full(keep.size + clone.size, -1)] + [cand_rank[split]] * split_factor)
    return source, kind, rank
