"""The case table of the NetVLAD pooling tests (tests/test_vlad_mirror.py, tests/test_vlad_gpu.py): shapes, data and the crafted softmax
cases.  Everything is made once per process, shared, and never written to; the mirror's answer of a case is computed once as well.

Shapes (N positions, C channels, K kept, G ghost clusters), each within the limits ((K+G) * C <= 32768):
  positions 1, 63, 64, 65, 128, 130 and 30 x 47 = 1410: a ragged block, exact blocks, more blocks than one;
  channels 4, 252, 256, 260, 512, 1024: one ragged chunk of the float tree, a chunk short of / exactly / just over 256, two and four chunks
  (and 64-channel slices of the aggregation that are ragged: 4, 252, 260);
  (K, G) (1, 0), (16, 0), (64, 0), (8, 2), (126, 2): one cluster (a == 1), the default model, Relja's, ghosts, both score registers of a
  lane in use with the last group of eight clusters ragged (126 = 15 * 8 + 6)."""
from functools import lru_cache

import numpy as np

import np_mirror_vlad as M

SHAPES = [
    (1, 4, 1, 0),
    (63, 252, 16, 0),
    (64, 256, 8, 2),
    (65, 260, 16, 0),
    (128, 512, 64, 0),
    (130, 1024, 16, 0),
    (1410, 512, 16, 0),        # the default model: MobileNet conv_pw_7_relu at 30 x 47, K = 16 -> 8192
    (130, 256, 126, 2),
    (65, 4, 126, 2),
    (1410, 252, 1, 0),
    (130, 1024, 8, 2),
    (64, 260, 64, 0),
    (130, 512, 64, 0),         # Relja's shape kept small: 32768-D
]
CRAFTED = ["far_apart", "all_equal", "zero_position", "dead_cluster", "zero_map"]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def weights(C, K, G, seed=0):
    """(Wt, bias, centres): scores of a post-ReLU map spread over a few units, so that the softmax is neither flat nor one-hot"""
    rng = np.random.default_rng(1000 * C + 10 * K + G + seed)
    Wt = (rng.standard_normal((K + G, C)) * (2.0 / np.sqrt(C))).astype(np.float32)
    bias = (0.5 * rng.standard_normal(K + G)).astype(np.float32)
    centres = (0.3 * rng.standard_normal((K, C))).astype(np.float32)
    return _frozen(Wt, bias, centres)


@lru_cache(maxsize=None)
def fmap(N, C, seed=0):
    """a post-ReLU look: about half the values are zero"""
    rng = np.random.default_rng(77 * N + C + seed)
    (x,) = _frozen(np.maximum(rng.standard_normal((N, C)), 0).astype(np.float32))
    return x


@lru_cache(maxsize=None)
def shape_case(N, C, K, G):
    """(x, Wt, bias, centres, the mirror's answer)"""
    Wt, bias, centres = weights(C, K, G)
    x = fmap(N, C)
    return x, Wt, bias, centres, M.vlad(x, Wt, bias, centres)


@lru_cache(maxsize=None)
def crafted_case(name):
    """(x, Wt, bias, centres, the mirror's answer) of a crafted softmax case, all at N = 70 (a ragged second block), C = 8, K = 3, G = 1"""
    N, C, K, G = 70, 8, 3, 1
    Wt, bias, centres = (np.array(a) for a in weights(C, K, G, seed=5))
    x = np.array(fmap(N, C, seed=5))
    if name == "far_apart":            # scores more than 700 apart: exact zeros in a
        Wt[1] = 0
        bias[1] = 2000.0
        x[5] = 0                       # ... and a position whose scores are the bias alone
    elif name == "all_equal":          # every score equal: a == 1 / (K+G) exactly
        Wt[:] = 0
        bias[:] = 0.25
    elif name == "zero_position":      # a zero feature vector: a is the softmax of the bias
        x[0] = 0
        x[69] = 0
    elif name == "dead_cluster":       # a cluster whose weight is +0 at every position, zero centres: the epsilon gives an all-zero row
        Wt[2] = 0
        bias[2] = -3000.0
        centres[2] = 0
    elif name == "zero_map":           # the all-zero map with zero centres: the whole vector is zero
        x[:] = 0
        centres[:] = 0
    else:
        raise KeyError(name)
    _frozen(x, Wt, bias, centres)
    return x, Wt, bias, centres, M.vlad(x, Wt, bias, centres)
