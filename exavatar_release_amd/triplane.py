"""HIP triplane feature lookup: a drop-in for ExAvatar's ``HumanGaussian.extract_tri_feature``.

* ``TriplaneFeatures(pos_enc_mesh, is_face)(triplane, triplane_face)`` -- reference ``avatar/common/nets/module.py:424-457``:
  the per-vertex features of the body triplane, overwritten for the face vertices by those of the face triplane,
  ``[N, 3C]``.  Its values are the reference's ``tri_feat``; the gradients reach both triplanes, bit-reproducibly.

The kernels are ``csrc/triplane.hip`` behind ``include/exa_triplane.h``; ROCm device tensors only, no CPU path.  The CPU
restatement that pins them is ``tests/triplane_oracle.py``.

Semantics
---------
The constructor normalises the coordinates once, with torch and exactly as the reference does: the body coordinates are
``pos_enc_mesh`` minus its mean, divided by ``shape_3d / 2``; those of the face rows are ``pos_enc_mesh[is_face]`` minus
their own mean, divided by ``face_shape_3d / 2``.  Plane k of a row's set is sampled at ``(gx, gy)``, ``(gx, gz)``,
``(gy, gz)`` by ``F.grid_sample`` (bilinear, zero padding, ``align_corners=False``), evaluated operation by operation in
fp32 without fused multiply-adds; output column ``k * C + c`` holds plane k, channel c.

The backward sums, for every texel and channel, the products ``g * w`` of the rows whose taps land there in ascending row
order, cut into segments of ``seg_len`` entries (two-level: sequential partials, then the partials in order; see the
header).  No atomics, so the same inputs give the same bits.  The coordinates are constants (``pos_enc_mesh`` is a buffer
in the reference) and get no gradient.

The plan -- which rows' taps land on which texel, in which order -- depends on the coordinates alone, so it is built once,
in the constructor, for one plane shape ``triplane_shape = (C, H, W)`` (the reference's ``cfg.triplane_shape``).  After
that ``forward`` allocates its outputs and launches one kernel each way; it does not synchronise and can be captured
into a hipGraph.
"""
import numpy as np
import torch

from . import _lib
from ._device import _ptr, grad_in, launch, need_rocm

BWD_BLOCK = 1024          # threads of a backward workgroup (csrc/triplane.hip)
MAX_LDS = 65536           # EXA_TRIPLANE_MAX_LDS
MIN_SEG_LEN = 32


def normalize_coords(pos_enc_mesh, is_face, shape_3d=(2, 2, 2), face_shape_3d=(0.3, 0.3, 0.3)):
    """[N, 3] coordinates of every row in its own set's frame (module.py:427-447): the body rows centred on the mean of all
    vertices and divided by ``shape_3d / 2``, the face rows on the mean of the face vertices and ``face_shape_3d / 2``."""
    def frame(xyz, ext):
        xyz = xyz - torch.mean(xyz, 0)[None, :]
        return torch.stack((xyz[:, 0] / (ext[0] / 2), xyz[:, 1] / (ext[1] / 2), xyz[:, 2] / (ext[2] / 2)), 1)

    coords = frame(pos_enc_mesh, shape_3d)
    if bool(is_face.any()):
        coords[is_face] = frame(pos_enc_mesh[is_face, :], face_shape_3d)
    return coords.contiguous()


def segment_length(max_list, C):
    """The plan's segment length S: 32, doubled until the longest texel list fits one workgroup's LDS partials."""
    cap = MAX_LDS // (4 * C)
    S = MIN_SEG_LEN
    while -(-max_list // S) > cap:
        S *= 2
    return S


def pack_workgroups(nseg, C):
    """Greedy packing of consecutive texels into backward workgroups: up to one pass of the workgroup's threads worth of
    segments and a bounded number of texels each; a texel with more segments than that gets a workgroup of its own.
    Returns (wg_tex [num_wg + 1] int32 numpy, max_wg_segments)."""
    G = C // 4 if C % 4 == 0 else C
    slots = max(1, BWD_BLOCK // G)
    tex_max = max(1, 32768 // C)
    bounds = [0]
    cur_seg = cur_tex = 0
    most = 1
    for t, s in enumerate(nseg.tolist()):
        if cur_tex and (cur_seg + s > slots or cur_tex >= tex_max):
            bounds.append(t)
            most = max(most, cur_seg)
            cur_seg = cur_tex = 0
        cur_seg += s
        cur_tex += 1
    bounds.append(len(nseg))
    most = max(most, cur_seg)
    return np.asarray(bounds, dtype=np.int32), most


def plan_tables(keys, T, C):
    """Steps 2-4 of the plan (include/exa_triplane.h) from the step-1 keys [N * 12] int32, on the keys' device: the
    stable sort, the per-texel CSR, the segments and the workgroups.  Returns a dict of int32 tensors (entries, seg_entry,
    tex_seg, wg_tex) and ints (seg_len, num_wg, max_wg_segments), plus the list lengths [T]."""
    dev = keys.device
    sorted_keys, order = torch.sort(keys, stable=True)
    offsets = torch.searchsorted(sorted_keys, torch.arange(T + 1, dtype=torch.int32, device=dev), out_int32=True)
    counts = (offsets[1:] - offsets[:-1]).long()
    seg_len = segment_length(int(counts.max()), C)
    nseg = (counts + seg_len - 1) // seg_len
    tex_seg = torch.cat([nseg.new_zeros(1), torch.cumsum(nseg, 0)])
    seg_tex = torch.repeat_interleave(torch.arange(T, device=dev), nseg)
    starts = offsets.long()[seg_tex] + (torch.arange(seg_tex.numel(), device=dev) - tex_seg[seg_tex]) * seg_len
    wg_tex, most = pack_workgroups(nseg.cpu().numpy(), C)
    return {'entries': order.to(torch.int32), 'seg_entry': torch.cat([starts, offsets[-1:].long()]).to(torch.int32),
            'tex_seg': tex_seg.to(torch.int32), 'wg_tex': torch.from_numpy(wg_tex).to(dev), 'seg_len': seg_len,
            'num_wg': len(wg_tex) - 1, 'max_wg_segments': most, 'list_lengths': counts}


class _Plan:
    """The backward's texel-major lists (include/exa_triplane.h, steps 1-4), on the device."""

    def __init__(self, coords, is_face_u8, C, H, W):
        dev = coords.device
        N = coords.shape[0]
        keys = torch.empty(N * 12, dtype=torch.int32, device=dev)
        if N:
            launch(_lib.TRIPLANE, 'exa_triplane_plan_keys', dev, N, H, W, _ptr(coords), _ptr(is_face_u8), _ptr(keys))
        self.keys = keys
        for k, v in plan_tables(keys, 6 * H * W, C).items():
            setattr(self, k, v)


class _TriplaneLookup(torch.autograd.Function):
    """body, face [3, C, H, W] (float32, contiguous) -> [N, 3C]."""

    @staticmethod
    def forward(ctx, body, face, tf):
        C, H, W = body.shape[1:]
        N = tf.num_rows
        out = torch.empty((N, 3 * C), dtype=torch.float32, device=body.device)
        if N:
            launch(_lib.TRIPLANE, 'exa_triplane_forward', body.device, N, C, H, W, _ptr(body), _ptr(face),
                   _ptr(tf.coords), _ptr(tf.is_face_u8), _ptr(out))
        ctx.tf = tf
        ctx.shape = (C, H, W)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        tf, (C, H, W) = ctx.tf, ctx.shape
        p = tf.plan
        grad_out = grad_in(grad_out)
        dev = grad_out.device
        grad_body = torch.empty((3, C, H, W), dtype=torch.float32, device=dev)
        grad_face = torch.empty((3, C, H, W), dtype=torch.float32, device=dev)
        launch(_lib.TRIPLANE, 'exa_triplane_backward', dev, tf.num_rows, C, H, W, _ptr(tf.coords), _ptr(grad_out),
               _ptr(p.entries), _ptr(p.seg_entry), _ptr(p.tex_seg), _ptr(p.wg_tex), p.num_wg, p.max_wg_segments,
               _ptr(grad_body), _ptr(grad_face))
        return grad_body, grad_face, None


class TriplaneFeatures:
    """The triplane lookup of one model's vertices (module docstring).

    ``pos_enc_mesh`` [N, 3] float32 and ``is_face`` [N] bool on the ROCm device; ``shape_3d`` / ``face_shape_3d`` are the
    reference's ``cfg.triplane_shape_3d`` / ``cfg.triplane_face_shape_3d`` and ``triplane_shape`` its
    ``cfg.triplane_shape`` (C, H, W), the shape of both plane sets."""

    def __init__(self, pos_enc_mesh, is_face, shape_3d=(2, 2, 2), face_shape_3d=(0.3, 0.3, 0.3),
                 triplane_shape=(32, 128, 128)):
        if pos_enc_mesh.dim() != 2 or pos_enc_mesh.shape[1] != 3:
            raise ValueError('TriplaneFeatures: pos_enc_mesh must be [N, 3]')
        if is_face.shape != (pos_enc_mesh.shape[0],) or is_face.dtype != torch.bool:
            raise ValueError('TriplaneFeatures: is_face must be a bool [N] tensor')
        if pos_enc_mesh.dtype != torch.float32:
            raise ValueError('TriplaneFeatures: float32 coordinates only')
        if pos_enc_mesh.requires_grad:
            raise ValueError('TriplaneFeatures: the coordinates are constants (no gradient to pos_enc_mesh); detach them')
        C, H, W = (int(s) for s in triplane_shape)
        if not (1 <= C <= 1024 and H >= 1 and W >= 1):
            raise ValueError('TriplaneFeatures: triplane_shape must be (C, H, W) with 1 <= C <= 1024, H, W >= 1')
        need_rocm(pos_enc_mesh.device, 'TriplaneFeatures')
        need_rocm(is_face.device, 'TriplaneFeatures')
        if pos_enc_mesh.device != is_face.device:
            raise ValueError('TriplaneFeatures: pos_enc_mesh and is_face are on different devices')
        self.triplane_shape = (C, H, W)
        self.num_rows = int(pos_enc_mesh.shape[0])
        self.device = pos_enc_mesh.device
        with torch.no_grad():
            self.coords = normalize_coords(pos_enc_mesh, is_face, shape_3d, face_shape_3d)
        self.is_face_u8 = is_face.to(torch.uint8).contiguous()
        self.plan = _Plan(self.coords, self.is_face_u8, C, H, W)

    def _check_planes(self, triplane, triplane_face):
        want = (3,) + self.triplane_shape
        for name, t in (('triplane', triplane), ('triplane_face', triplane_face)):
            need_rocm(t.device, 'TriplaneFeatures')
            if t.device != self.device:
                raise ValueError('TriplaneFeatures: %s is not on the device of the coordinates' % name)
            if t.dtype != torch.float32:
                raise ValueError('TriplaneFeatures: float32 planes only (%s is %s)' % (name, t.dtype))
            if tuple(t.shape) != want:
                raise ValueError('TriplaneFeatures: %s has shape %s; the plan was built for %s'
                                 % (name, tuple(t.shape), want))

    def forward(self, triplane, triplane_face):
        """``[N, 3C]`` features of ``triplane`` / ``triplane_face`` ``[3, C, H, W]``, differentiable in both."""
        self._check_planes(triplane, triplane_face)
        return _TriplaneLookup.apply(triplane.contiguous(), triplane_face.contiguous(), self)

    __call__ = forward
