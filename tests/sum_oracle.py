"""The fixed-order sums of ``exavatar_release_amd/csrc/fixed_sum.h`` restated in numpy, one function per order, for the
oracles that hold the kernels to their bits.  Every function adds in the dtype of its argument (float32: the kernels'
roundings; float64: the exact semantics); lanes and threads lie on the trailing axis, leading axes are batched."""
import numpy as np

WAVE, BLOCK = 64, 256
DISTANCES = (32, 16, 8, 4, 2, 1)


def butterfly(s):
    """[..., 64] -> [..., 64]: for d = 32 .. 1, s = s + s[lane ^ d]; every lane ends with the wave's sum."""
    s, lane = np.asarray(s), np.arange(WAVE)
    for d in DISTANCES:
        s = s + s[..., lane ^ d]
    return s


def tree(q):
    """[..., 64] -> [...]: lane 0 of the tree, for d = 32 .. 1, q = q + q[lane + d] (only the lanes below d feed it)."""
    q = np.asarray(q)
    for d in DISTANCES:
        q = q[..., :d] + q[..., d:2 * d]
    return q[..., 0]


def waves(w):
    """[..., 4] -> [...]: ((wave 0 + wave 1) + wave 2) + wave 3."""
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def wg_sum(s):
    """[..., 256] -> [...]: the workgroup sum, the butterfly in each wave of 64 consecutive threads, then ``waves``."""
    s = np.asarray(s)
    return waves(butterfly(s.reshape(s.shape[:-1] + (BLOCK // WAVE, WAVE)))[..., 0])


def strided_sum(x):
    """flat [n] -> [256]: thread j adds x[j], x[j + 256], .. in that order from +0; past the end it adds nothing."""
    x = np.asarray(x).reshape(-1)
    trips = (x.size + BLOCK - 1) // BLOCK
    pad = np.zeros(trips * BLOCK, x.dtype)
    pad[:x.size] = x
    live = (np.arange(trips * BLOCK) < x.size).reshape(trips, BLOCK)
    s = np.zeros(BLOCK, x.dtype)
    for t, row in enumerate(pad.reshape(trips, BLOCK)):
        s = np.where(live[t], s + row, s)
    return s
