"""Inputs for the densification tests, built class by class so that EVERY row keeps a wide margin from every threshold
that a transcendental decides (tests/test_densify_oracle.py asserts it on the CPU; no GPU test excludes a row).

One letter per source row, with ``screen_size_max`` truthy (every rule active) and the hyperparameters ``HYPER``:

    K  kept      cold, small                          C  cloned    hot, small: the original and a copy survive
    S  split     hot, big: two children survive       P  pruned    cold, transparent
    W  split     hot, big AND wide, the children not  X  candidate hot, too wide even for its children: nothing survives
    L  candidate hot, big, transparent: nothing       T  nothing   hot, small, transparent
    Z  pruned    cold, wide
"""
import numpy as np

F32 = np.float32
EXTENT = 5.0
HYPER = dict(grad_thr=0.0002, dense_percent=0.01, opacity_min=0.005)
#        hot, band of max exp(scale) (extent 5: big above 0.05, wide above 0.5, wide children above 0.8), transparent
CLASSES = {'K': (0, 0, 0), 'C': (1, 0, 0), 'S': (1, 1, 0), 'P': (0, 0, 1), 'W': (1, 2, 0), 'X': (1, 3, 0), 'L': (1, 1, 1),
           'T': (1, 0, 1), 'Z': (0, 2, 0)}
BANDS = [(0.01, 0.04), (0.06, 0.45), (0.55, 0.75), (0.9, 2.0)]
EXPECT = {'K': (1, 0, 0, 0), 'C': (1, 1, 0, 0), 'S': (0, 0, 1, 1), 'P': (0, 0, 0, 0), 'W': (0, 0, 1, 1), 'X': (0, 0, 0, 1),
          'L': (0, 0, 0, 1), 'T': (0, 0, 0, 0), 'Z': (0, 0, 0, 0)}      # keep, clone, split, cand per row


def build(pattern, seed=0, split_factor=2):
    """The required inputs for the rows of ``pattern`` (a string of class letters): 'xyz_grad_accum' / 'track_cnt' [P, 1],
    'scale' [P, 3], 'opacity' [P, 1], 'mean' [P, 3], 'rotation' [P, 6], 'radius_max' [P], and 'noise' for every
    candidate."""
    rng = np.random.RandomState(seed)
    P = len(pattern)
    spec = np.array([CLASSES[c] for c in pattern], np.int64).reshape(P, 3)
    top = np.array([rng.uniform(*BANDS[b]) for b in spec[:, 1]]).reshape(P)
    frac = rng.uniform(0.05, 1.0, (P, 3))
    frac[np.arange(P), rng.randint(0, 3, P)] = 1.0
    cnt = rng.randint(1, 6, P).astype(F32)
    g = np.where(spec[:, 0] == 1, rng.uniform(0.0003, 0.01, P), rng.uniform(0.0, 0.00015, P))
    n_cand = int(sum(EXPECT[c][3] for c in pattern))
    return {'xyz_grad_accum': (g * cnt).astype(F32)[:, None], 'track_cnt': cnt[:, None],
            'scale': np.log(top[:, None] * frac).astype(F32),
            'opacity': np.where(spec[:, 2] == 1, rng.uniform(-8.0, -6.0, P), rng.uniform(-4.0, 5.0, P)).astype(F32)[:, None],
            'mean': (2.0 * rng.randn(P, 3)).astype(F32), 'rotation': rng.randn(P, 6).astype(F32),
            'radius_max': rng.randint(0, 41, P).astype(F32), 'noise': rng.randn(split_factor * n_cand, 3).astype(F32)}


def random_pattern(P, seed, letters='KCSPWXLTZ'):
    rng = np.random.RandomState(seed)
    return ''.join(rng.choice(list(letters), P))


def expected_counts(pattern):
    """(n_keep, n_clone, n_split, n_cand) of a pattern with every rule active."""
    return tuple(int(sum(EXPECT[c][i] for c in pattern)) for i in range(4))
