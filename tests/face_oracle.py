"""The face composite and the face-composited L1 term (include/exa_raster.h, ``exa_face_l1_*`` / ``exa_composite_*``)
restated operation by operation in numpy: in float32, where every array must equal the kernels' bit for bit, and in
float64, where the mean is the exact value the float32 mean is held against.

Arrays: ``img``, ``target`` [B, C, H, W]; ``face`` [B, C + 1, H, W] (C colour planes, one coverage plane); ``crop`` =
(x0, y0, w, h), the clamped bbox.  Also the header's work split as plain functions (``blocks``, ``mean_depth``) and the
small random cases of the GPU test."""
import numpy as np

RUN, BLOCK = 4, 256


def crop_window(bbox, H, W):
    """(x0, y0, w, h) of the reference's clamp (loss.py:19-24), the whole image for None; bbox = (xmin, ymin, w, h)."""
    if bbox is None:
        return 0, 0, W, H
    xmin, ymin, width, height = [int(v) for v in bbox]
    x0, y0 = max(xmin, 0), max(ymin, 0)
    x1, y1 = min(x0 + width, W), min(y0 + height, H)
    return x0, y0, max(x1 - x0, 0), max(y1 - y0, 0)


def _cut(a, crop):
    x0, y0, w, h = crop
    return a[:, :, y0:y0 + h, x0:x0 + w]


def is_face(face):
    """[B, C, H, W] bool: the colour is not -1 and the coverage is 1."""
    C = face.shape[1] - 1
    return (face[:, :C] != -1) & (face[:, C:] == 1)


def hard(img, face):
    """f ? face_c : img_c."""
    return np.where(is_face(face), face[:, :face.shape[1] - 1], img)


def l1_map(img, face, target, crop, dtype=np.float32):
    """[B, C, h, w]: |v - target| over the window, v the hard composite."""
    img, face, target = (np.asarray(a, dtype=dtype) for a in (img, face, target))
    return np.abs(_cut(hard(img, face), crop) - _cut(target, crop))


def l1_mean64(img, face, target, crop):
    m = l1_map(img, face, target, crop, np.float64)
    return float(m.mean()) if m.size else float('nan')


def l1_grads(img, face, target, crop, g_map=None, g_mean=None, reciprocal=True):
    """(dL_dimg [B, C, H, W], dL_dface [B, C + 1, H, W]) in float32 for a cotangent of the map (``g_map`` [B, C, h, w]) or
    of the mean (``g_mean``, a float32 scalar).  The mean's: ``reciprocal`` = True is the header's and the kernel's
    g = g_mean * (1 / float32(n)), what torch's backward of ``.mean()`` forms on the device; False is g = g_mean / float32(n),
    what it forms on the CPU.  The two can differ in the last bit."""
    assert (g_map is None) != (g_mean is None)
    x0, y0, w, h = crop
    B, C = img.shape[:2]
    f = _cut(is_face(face), crop)
    d = _cut(hard(img, face), crop) - _cut(target, crop)
    s = (d > 0).astype(np.float32) - (d < 0).astype(np.float32)
    if g_map is None:
        with np.errstate(divide='ignore', invalid='ignore'):
            n = np.float32(B * C * w * h)
            g = np.float32(g_mean) * (np.float32(1) / n) if reciprocal else np.float32(g_mean) / n
    else:
        g = np.asarray(g_map, dtype=np.float32)
    sg, f = (s * g).astype(np.float32), f.astype(np.float32)
    d_img, d_face = np.zeros(img.shape, np.float32), np.zeros(face.shape, np.float32)
    # the header's `f ? 0 : s g` and `f ? s g : 0`, written as the reference's products: the same numbers, and its zeros' signs
    d_img[:, :, y0:y0 + h, x0:x0 + w] = sg * (np.float32(1) - f)
    d_face[:, :C, y0:y0 + h, x0:x0 + w] = sg * f
    return d_img, d_face


def hard_grads(face, g):
    """The two selections of dL_dout, the coverage plane zero."""
    f = is_face(face)
    d_face = np.zeros(face.shape, np.float32)
    d_face[:, :face.shape[1] - 1] = np.where(f, g, np.float32(0))
    return np.where(f, np.float32(0), g).astype(np.float32), d_face


def soft(img, face):
    """w = (face_c != -1 ? 1 : 0) * coverage; img * (1 - w) + face_c * w, every operation rounded to float32."""
    C = face.shape[1] - 1
    fc = face[:, :C]
    w = ((fc != -1).astype(np.float32) * face[:, C:]).astype(np.float32)
    return ((img * (np.float32(1) - w)).astype(np.float32) + (fc * w).astype(np.float32)).astype(np.float32)


def foreground(fg, mask, bg, thr=0.9):
    return np.where(mask > np.float32(thr), fg, bg)


# ---- the header's work split ---------------------------------------------------------------------------------------------
def blocks(B, C, w, h):
    """exa_face_l1_blocks: the workgroups (partial sums) of the forward."""
    if B <= 0 or C <= 0 or w <= 0 or h <= 0:
        return 0
    return (B * h * ((w + 6) // RUN) + BLOCK - 1) // BLOCK


def mean_depth(B, C, w, h):
    """The additions an element passes through on its way into the mean, by the header's rule: 4 C in its thread, 6 in its
    wave and 3 in its workgroup; then ceil(partials / 256) in a thread of the reduction and the same 6 + 3."""
    n = blocks(B, C, w, h)
    return RUN * C + 9 + (n + BLOCK - 1) // BLOCK + 9


# ---- small random cases -----------------------------------------------------------------------------------------------
def make_case(seed, B, H, W, crop, C=3):
    """dict of float32 arrays: img, target, face [B, C + 1, H, W], fg_mask [B, 1, H, W].  The face render has background
    pixels (-1 in every channel, coverage 0), channels at -1 here and there and coverage drawn from {0, 0.5, 1}.  Whatever
    the draw gives, the first four pixels of the crop in row-major order (a crop that has four) are: a pixel with channel 1
    alone at -1 and coverage 1, coloured pixels with coverage 0.5 and 0, and a pixel with every channel a face's."""
    rs = np.random.RandomState(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    out = {'img': f32(rs.uniform(0.02, 0.98, (B, C, H, W))), 'target': f32(rs.uniform(0.02, 0.98, (B, C, H, W))),
           'fg_mask': f32(rs.choice([0.0, 0.5, 0.9, 0.95, 1.0], (B, 1, H, W)))}
    rgb = rs.uniform(0.02, 0.98, (B, C, H, W))
    cov = rs.choice([0.0, 0.5, 1.0], (B, 1, H, W), p=[0.3, 0.2, 0.5])
    rgb = np.where(cov == 0, -1.0, rgb)
    rgb = np.where(rs.uniform(size=(B, C, H, W)) < 0.15, -1.0, rgb)
    x0, y0, w, h = crop
    if w * h >= 4:
        spot = [(y0 + i // w, x0 + i % w) for i in range(4)]
        for (y, x), c in zip(spot, (1.0, 0.5, 0.0, 1.0)):
            rgb[:, :, y, x], cov[:, 0, y, x] = rs.uniform(0.02, 0.98, (B, C)), c
        rgb[:, 1 % C, spot[0][0], spot[0][1]] = -1.0
    out['face'] = f32(np.concatenate([rgb, cov], 1))
    return out
