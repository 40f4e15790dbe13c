"""CPU tests of the offset regularisers' host side: the entry points are exported and bound, the pairs and the constant
weights are the reference's, every invalid argument of the C calls fails with its negative status and its message before
any GPU work, and the Python surface refuses what it does not support.  The ABI itself (include/exa_mesh.h against its
binding) is checked by tests/test_abi.py."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import exavatar_release_amd as exa
from exavatar_release_amd import _lib, build
from tests import loss_case as lc
from tests import offset_oracle as oo

BAD = ctypes.c_void_p(0x1000)      # never dereferenced: every call below fails validation first, or has nothing to do
INVALID, NULLPTR = -1, -2
ENTRY_POINTS = (('exa_mesh_offset_regs_blocks', 2), ('exa_mesh_offset_regs_pair_table', 5),
                ('exa_mesh_offset_regs_vertex_forward', 13), ('exa_mesh_offset_regs_joint_forward', 14),
                ('exa_mesh_offset_regs_backward', 25))
module = sys.modules['exavatar_release_amd.offset_regs']      # the package's `offset_regs` is the function


def test_the_entry_points_are_exported_and_bound():
    lib = _lib.load()
    for name, n_args in ENTRY_POINTS:
        assert name in _lib.MESH.signatures
        assert len(getattr(lib, name).argtypes) == n_args
    assert lib.exa_mesh_offset_regs_blocks.restype is ctypes.c_int64
    assert lib.exa_mesh_version() == 100 and _lib.MESH.version == 100 and len(_lib.ABIS) == 6
    assert build.SOURCES['offset_regs.hip'] == ['-ffp-contract=off']
    for name in ('OffsetRegs', 'offset_regs', 'JointOffsetSymmetricReg', 'symmetric_joint_pairs', 'loss_weights'):
        assert name in exa.__all__ and getattr(exa, name) is getattr(module, name)
    assert 'OffsetRegs' in exa.__doc__ and module.TERMS == oo.TERMS and module.ROWS == oo.BLOCK


def test_the_number_of_partials_is_the_headers():
    lib = _lib.load()
    for B, V in ((1, 1), (1, 255), (1, 256), (1, 257), (2, 3202), (1, 65537), (1, 167281), (0, 5), (5, 0), (-1, 5), (5, -1)):
        assert lib.exa_mesh_offset_regs_blocks(B, V) == oo.blocks(B, V), (B, V)
    assert lib.exa_mesh_offset_regs_blocks(1 << 15, 1 << 15) == 0                      # beyond the 2^30 elements


# ---- the pairs and the weights --------------------------------------------------------------------------------------------
def test_symmetric_joint_pairs_on_the_smplx_names():
    right, left = exa.symmetric_joint_pairs(lc.JOINTS_NAME)
    want_r = [j for j in range(lc.J) if lc.JOINTS_NAME[j][:2] == 'R_']
    want_l = [lc.JOINTS_NAME.index('L_' + lc.JOINTS_NAME[j][2:]) for j in want_r]      # the lists loss_case.HipLoss builds
    assert len(right) == 24 and right == want_r and left == want_l
    assert right == sorted(right) and not set(right) & set(left)
    assert exa.symmetric_joint_pairs(['Pelvis', 'Neck']) == ([], [])
    with pytest.raises(ValueError, match="'L_Knee' is not in list"):
        exa.symmetric_joint_pairs(['Pelvis', 'R_Knee', 'L_Hip'])
    m = exa.JointOffsetSymmetricReg(lc.JOINTS_NAME)
    assert m.pair_right.tolist() == want_r and m.pair_left.tolist() == want_l and m.pair_right.dtype == torch.int32
    table = m.joint_pair.tolist()
    assert all(table[r] == 2 * p and table[l] == 2 * p + 1 for p, (r, l) in enumerate(zip(want_r, want_l)))
    assert sum(t == -1 for t in table) == lc.J - 48 and not m.state_dict()


def test_loss_weights_are_the_blocks():
    case = lc.build_case()
    masks = {k: torch.from_numpy(np.array(case[k])) for k in lc.MASKS}
    want = lc.vertex_weights(masks, torch.ones((1, lc.V, 1)))
    got = exa.loss_weights(*[masks[k] for k in lc.MASKS], joint_part=lc.JOINT_PART, joint_num=lc.J)
    assert list(got) == ['gaussian_mean_reg', 'gaussian_scale_reg', 'lap_mean', 'lap_scale', 'lap_rgb', 'joint_offset_reg']
    for k, w in want.items():
        assert got[k].dtype == torch.float32 and got[k].shape == (1, lc.V, 1)
        assert torch.equal(got[k].view(torch.int32), w.view(torch.int32)), k
    assert torch.equal(got['joint_offset_reg'].view(torch.int32), lc.joint_weight(torch.ones((lc.J, 3))).view(torch.int32))
    assert 'joint_offset_reg' not in exa.loss_weights(*[masks[k] for k in lc.MASKS])
    # the order of the assignments decides a vertex in two masks: face_expr over face, cavity over face_expr
    both = masks['is_face'] & masks['is_face_expr']
    assert both.any() and bool((got['gaussian_mean_reg'][0, both, 0] == 10).all())
    assert bool((got['gaussian_scale_reg'][0, masks['is_cavity'], 0] == 0).all())
    with pytest.raises(ValueError, match='loss_weights: is_face must be a bool \\[V\\] tensor with V = %d' % lc.V):
        exa.loss_weights(masks['is_rhand'], masks['is_lhand'], masks['is_face'][:-1], masks['is_face_expr'], masks['is_cavity'])
    with pytest.raises(ValueError, match='loss_weights: is_cavity must be a bool'):
        exa.loss_weights(*[masks[k] for k in lc.MASKS[:4]], masks['is_cavity'].float())
    with pytest.raises(ValueError, match='loss_weights: joint_num must be given with joint_part'):
        exa.loss_weights(*[masks[k] for k in lc.MASKS], joint_part=lc.JOINT_PART)
    with pytest.raises(ValueError, match=r"loss_weights: joint_part\['rhand'\] names a joint outside \[0, 40\)"):
        exa.loss_weights(*[masks[k] for k in lc.MASKS], joint_part=lc.JOINT_PART, joint_num=40)


# ---- the C calls' argument checks -----------------------------------------------------------------------------------------
def ints(*v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


def _pairs(lib, J, right, left, table=True):
    out = ints(*([7] * J))
    rc = lib.exa_mesh_offset_regs_pair_table(J, len(right), ints(*right), ints(*left), out if table else None)
    return rc, list(out)[:J]


def test_the_pair_table_checks_the_pairs_on_the_host():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    assert _pairs(lib, 6, [1, 4], [0, 5]) == (0, [1, 0, -1, -1, 2, 3])
    assert _pairs(lib, 3, [], []) == (0, [-1, -1, -1]) and _pairs(lib, 0, [], [], table=False) == (0, [])
    for right, left in (([6], [0]), ([0], [6]), ([-1], [0]), ([0], [-1])):
        assert _pairs(lib, 6, right, left)[0] == INVALID and err() == b'exa_mesh: a pair index is outside [0, J)'
    for right, left in (([1, 1], [0, 5]), ([1, 4], [0, 1]), ([2], [2])):
        assert _pairs(lib, 6, right, left)[0] == INVALID and err() == b'exa_mesh: a joint belongs to more than one pair'
    assert lib.exa_mesh_offset_regs_pair_table(-1, 0, None, None, None) == INVALID and b'negative size' in err()
    assert lib.exa_mesh_offset_regs_pair_table(4, -1, None, None, ints(0, 0, 0, 0)) == INVALID and b'negative size' in err()
    assert lib.exa_mesh_offset_regs_pair_table((1 << 20) + 1, 0, None, None, None) == INVALID and b'J exceeds 2^20' in err()
    assert _pairs(lib, 4, [1], [0], table=False)[0] == NULLPTR and b'joint_pair is NULL' in err()
    assert lib.exa_mesh_offset_regs_pair_table(4, 1, None, ints(0), ints(0, 0, 0, 0)) == NULLPTR
    assert b'pair_r / pair_l is NULL' in err()
    with pytest.raises(RuntimeError, match='exa_mesh: a joint belongs to more than one pair'):
        _lib.MESH.check(_pairs(lib, 6, [2], [2])[0])


def _vertex(lib, B=1, V=8, C=1, maps=True, partials=False, **null):
    ins = [None if null.get(n) else BAD for n in ('mean_offset', 'mean_offset_offset', 'scale', 'scale_offset', 'w_mean',
                                                   'w_scale')]
    m = [BAD if maps and not null.get(n) else None for n in ('mean_map', 'scale_map')]
    return lib.exa_mesh_offset_regs_vertex_forward(B, V, C, *ins, *m, BAD if partials else None, None)


def test_the_vertex_forward_checks_its_arguments():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    assert _vertex(lib, B=-1) == INVALID and err() == b'exa_mesh: negative size'
    assert _vertex(lib, V=-1) == INVALID and err() == b'exa_mesh: negative size'
    assert _vertex(lib, B=1 << 15, V=1 << 15) == INVALID and b'B * V * 3 exceeds 2^30' in err()
    for C in (0, 2, 4, -1):
        assert _vertex(lib, C=C) == INVALID and b'scale_offset must have 1 or 3 channels' in err(), C
    assert _vertex(lib, partials=True) == INVALID and b'pass exactly one of the maps / partials' in err()       # both
    assert _vertex(lib, maps=False) == INVALID and b'pass exactly one of the maps / partials' in err()           # neither
    assert _vertex(lib, scale_map=True) == INVALID and b'pass both maps or neither' in err()
    for n in ('mean_offset', 'mean_offset_offset', 'scale', 'scale_offset', 'w_mean', 'w_scale'):
        assert _vertex(lib, **{n: True}) == NULLPTR and b'w_mean / w_scale is NULL' in err(), n
    for zero in (dict(B=0), dict(V=0)):                                                                          # nothing to do
        assert _vertex(lib, **zero) == 0 and _vertex(lib, maps=False, partials=True, C=3, **zero) == 0


def _joint(lib, B=1, V=8, J=6, P=2, maps=True, means=False, partials=True, **null):
    ins = [None if null.get(n) else BAD for n in ('joint_offset', 'joint_ref', 'w_joint', 'pair_r', 'pair_l')]
    m = [BAD if maps and not null.get(n) else None for n in ('joint_map', 'sym_map')]
    return lib.exa_mesh_offset_regs_joint_forward(B, V, J, P, *ins, *m, BAD if partials else None, BAD if means else None, None)


def test_the_joint_forward_checks_its_arguments():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    for size in ('B', 'V', 'J', 'P'):
        assert _joint(lib, **{size: -1}) == INVALID and err() == b'exa_mesh: negative size', size
    assert _joint(lib, J=(1 << 20) + 1) == INVALID and b'J exceeds 2^20' in err()
    assert _joint(lib, J=5, P=3) == INVALID and b'n_pairs exceeds J / 2' in err()
    assert _joint(lib, means=True) == INVALID and b'pass exactly one of the maps / means' in err()               # both
    assert _joint(lib, maps=False) == INVALID and b'pass exactly one of the maps / means' in err()               # neither
    assert _joint(lib, maps=False, means=True, partials=False) == NULLPTR and b'partials is NULL' in err()
    assert _joint(lib, joint_map=True) == NULLPTR and b'joint_map / sym_map is NULL' in err()
    assert _joint(lib, sym_map=True) == NULLPTR and b'joint_map / sym_map is NULL' in err()
    for n in ('joint_offset', 'joint_ref', 'w_joint'):
        assert _joint(lib, **{n: True}) == NULLPTR and b'joint_offset / joint_ref / w_joint is NULL' in err(), n
    for n in ('pair_r', 'pair_l'):
        assert _joint(lib, **{n: True}) == NULLPTR and b'pair_r / pair_l is NULL' in err(), n
    assert _joint(lib, P=0, pair_r=True, pair_l=True, sym_map=True, J=0, joint_offset=True, joint_ref=True, w_joint=True,
                  joint_map=True, maps=True) == INVALID                                                          # neither
    assert lib.exa_mesh_offset_regs_joint_forward(0, 0, 0, 0, None, None, None, None, None, BAD, None, None, None, None) == 0


def ptrs(*v):
    return (ctypes.c_void_p * 4)(*v)


def _bwd(lib, B=1, V=8, C=1, J=6, P=2, g_maps=(1, 1, 1, 1), g_means=None, outs=(1, 1, 1, 1, 1), **null):
    names = ('mean_offset', 'mean_offset_offset', 'scale', 'scale_offset', 'w_mean', 'w_scale', 'joint_offset', 'joint_ref',
             'w_joint', 'pair_r', 'pair_l', 'joint_pair')
    ins = [None if null.get(n) else BAD for n in names]
    cot = [None if g is None else ptrs(*[0x1000 if x else None for x in g]) for g in (g_maps, g_means)]
    return lib.exa_mesh_offset_regs_backward(B, V, C, J, P, *ins, *cot, *[BAD if o else None for o in outs], None)


def test_the_backward_checks_its_arguments():
    lib = _lib.load()
    err = lib.exa_mesh_last_error
    for size in ('B', 'V', 'J', 'P'):
        assert _bwd(lib, **{size: -1}) == INVALID and err() == b'exa_mesh: negative size', size
    assert _bwd(lib, C=2) == INVALID and b'scale_offset must have 1 or 3 channels' in err()
    assert _bwd(lib, J=5, P=3) == INVALID and b'n_pairs exceeds J / 2' in err()
    word = b'cotangents of the maps or of the means, not both or neither'
    assert _bwd(lib, g_means=(1, 0, 0, 0)) == INVALID and word in err()                                          # both kinds
    assert _bwd(lib, g_maps=(1, 0, 0, 0), g_means=(0, 1, 0, 0)) == INVALID and word in err()                     # mixed
    assert _bwd(lib, g_maps=None) == INVALID and word in err()                                                   # neither
    assert _bwd(lib, g_maps=(0, 0, 0, 0), g_means=(0, 0, 0, 0)) == INVALID and word in err()
    with pytest.raises(RuntimeError, match='exa_mesh: offset_regs backward: pass cotangents of the maps or of the means'):
        _lib.MESH.check(_bwd(lib, g_maps=None))
    for n in ('mean_offset', 'mean_offset_offset', 'w_mean'):
        assert _bwd(lib, g_maps=None, g_means=(1, 0, 0, 0), **{n: True}) == NULLPTR and b'w_mean / w_scale is NULL' in err(), n
    for n in ('scale', 'scale_offset', 'w_scale'):
        assert _bwd(lib, g_maps=(0, 1, 0, 0), **{n: True}) == NULLPTR and b'w_mean / w_scale is NULL' in err(), n
    for n in ('joint_offset', 'joint_ref', 'w_joint'):
        assert _bwd(lib, g_maps=(0, 0, 1, 0), **{n: True}) == NULLPTR and b'joint_offset / joint_ref / w_joint is NULL' in err()
    for n in ('joint_offset', 'pair_r', 'pair_l', 'joint_pair'):
        assert _bwd(lib, g_maps=(0, 0, 0, 1), **{n: True}) == NULLPTR and b'pair_r / pair_l / joint_pair is NULL' in err(), n
    assert _bwd(lib, outs=(0, 0, 0, 0, 0)) == 0                                                                  # nothing wanted
    assert _bwd(lib, B=0, J=0, P=0) == 0 and _bwd(lib, V=0, outs=(1, 1, 1, 1, 0)) == 0                          # nothing to do


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def _args(B=2, V=5, J=6, ch=1):
    z = torch.zeros
    return dict(mean_offset=z(B, V, 3), mean_offset_offset=z(B, V, 3), scale=z(B, V, 3), scale_offset=z(B, V, ch),
                joint_offset=z(J, 3), mean_weight=z(1, V, 1), scale_weight=z(V), joint_offset_ref=z(J, 3),
                joint_weight=z(J, 3), sym_pairs=([1, 4], [0, 5]))


CONSTANTS = ('mean_weight', 'scale_weight', 'joint_offset_ref', 'joint_weight')


def test_offset_regs_raises_as_specified():
    f = exa.offset_regs
    for reduce in (None, 'mean'):
        with pytest.raises(ValueError, match=r'offset_regs: joint_offset must be on a ROCm device \(it is on cpu; there is no CPU'):
            f(**_args(), reduce=reduce)
    with pytest.raises(ValueError, match="offset_regs: reduce must be None or 'mean'"):
        f(**_args(), reduce='sum')
    tensors = [k for k in _args() if k != 'sym_pairs']
    for name in tensors:
        a = _args()
        with pytest.raises(TypeError, match='offset_regs: %s must be a tensor' % name):
            f(**dict(a, **{name: a[name].numpy()}))
        for other in (torch.float64, torch.float16):
            with pytest.raises(ValueError, match=r'offset_regs: %s must be float32 \(it is %s\)' % (name, other)):
                f(**dict(a, **{name: a[name].to(other)}))
    z = torch.zeros
    for name, bad, text in (('mean_offset', z(2, 5), r'\[B, V, 3\]'), ('mean_offset', z(2, 5, 2), r'\[B, V, 3\]'),
                            ('mean_offset_offset', z(2, 6, 3), r'\[2, 5, 3\], the shape of mean_offset'),
                            ('scale', z(1, 5, 3), r'\[2, 5, 3\], the shape of mean_offset'),
                            ('scale_offset', z(2, 5, 2), r'\[2, 5, 1\] or \[2, 5, 3\]'), ('scale_offset', z(2, 5), r'\[2, 5, 1\] or'),
                            ('joint_offset', z(6, 2), r'\[J, 3\]'), ('mean_weight', z(6), r'\[V\], \[V, 1\] or \[1, V, 1\] with V = 5'),
                            ('scale_weight', z(1, 5), r'\[V\], \[V, 1\] or \[1, V, 1\] with V = 5'),
                            ('joint_offset_ref', z(5, 3), r'\[J, 3\] with J = 6'), ('joint_weight', z(6), r'\[J, 3\] with J = 6')):
        with pytest.raises(ValueError, match='offset_regs: %s must be %s' % (name, text)):
            f(**dict(_args(), **{name: bad}))
    for name in CONSTANTS:
        a = _args()
        with pytest.raises(ValueError, match='offset_regs: %s is data in the reference and gets no gradient; detach it' % name):
            f(**dict(a, **{name: a[name].clone().requires_grad_(True)}))
    f_meta = dict(_args(), joint_offset=torch.zeros(6, 3, device='meta'))
    with pytest.raises(ValueError, match=r'offset_regs: joint_offset must be on a ROCm device \(it is on meta'):
        f(**f_meta)


def test_the_pairs_are_checked_when_they_are_built():
    a = {k: v for k, v in _args().items() if k in CONSTANTS}
    for pairs, text in ((([1, 4], [0]), 'must hold as many left as right joints'), (([6], [0]), r'names joint 6 outside \[0, 6\)'),
                        (([1, 1], [0, 5]), 'names a joint twice'), (([2], [2]), 'names a joint twice'),
                        ((['a'], [0]), r'must be \(right indices, left indices\)'), (5, r'must be \(right indices, left indices\)')):
        with pytest.raises(ValueError, match='OffsetRegs: sym_pairs ' + text):
            exa.OffsetRegs(sym_pairs=pairs, **a)
    m = exa.OffsetRegs(sym_pairs=None, **a)
    assert m.pair_right.shape == (0,) and m.joint_pair.tolist() == [-1] * 6


def test_the_module_holds_its_constants_as_buffers():
    a = _args()
    m = exa.OffsetRegs(*[a[k] for k in CONSTANTS], a['sym_pairs'])
    assert not m.state_dict() and not list(m.parameters())
    assert sorted(n for n, _ in m.named_buffers()) == ['joint_offset_ref', 'joint_pair', 'joint_weight', 'mean_weight',
                                                       'pair_left', 'pair_right', 'scale_weight']
    assert m.mean_weight.shape == (5,) and m.scale_weight.shape == (5,) and m.joint_pair.tolist() == [1, 0, -1, -1, 2, 3]
    with pytest.raises(ValueError, match='OffsetRegs: scale_weight must be'):
        exa.OffsetRegs(a['mean_weight'], torch.zeros(4), a['joint_offset_ref'], a['joint_weight'], None)
    with pytest.raises(ValueError, match=r'OffsetRegs: joint_weight must be \[J, 3\] with J = 6'):
        exa.OffsetRegs(a['mean_weight'], a['scale_weight'], a['joint_offset_ref'], torch.zeros(5, 3), None)
    with pytest.raises(ValueError, match='OffsetRegs: mean_weight is data in the reference'):
        exa.OffsetRegs(a['mean_weight'].clone().requires_grad_(True), a['scale_weight'], a['joint_offset_ref'],
                       a['joint_weight'], None)
    inputs = {k: v for k, v in a.items() if k not in CONSTANTS and k != 'sym_pairs'}
    with pytest.raises(ValueError, match=r'offset_regs: joint_offset must be on a ROCm device'):
        m(**inputs)
    with pytest.raises(ValueError, match=r'offset_regs: mean_weight must be \[V\], \[V, 1\] or \[1, V, 1\] with V = 4'):
        m(**dict(inputs, **{k: torch.zeros(2, 4, 3 if k != 'scale_offset' else 1)
                            for k in ('mean_offset', 'mean_offset_offset', 'scale', 'scale_offset')}))
    s = exa.JointOffsetSymmetricReg(lc.JOINTS_NAME)
    with pytest.raises(ValueError, match=r'JointOffsetSymmetricReg: joint_offset must be \[J, 3\] with J = 55'):
        s(torch.zeros(54, 3))
    with pytest.raises(ValueError, match='JointOffsetSymmetricReg: joint_offset must be on a ROCm device'):
        s(torch.zeros(55, 3))
