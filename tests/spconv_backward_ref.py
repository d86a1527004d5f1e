"""What test_spconv_backward_host.py and test_gpu_spconv_backward.py share: float64 numpy restatements of the sparse
convolution's two gradients, the voxel sets the GPU cases run on, the geometry of one convolution of the U-Net as the
training executor resolves it (csrc/unet_train.hip: conv_geom) and the operands of the two legs.

Integer leg: sums of products of small integers are exact in fp32 whatever the order of summation, the MFMA shape or
the number and order of the atomics, as long as every partial sum stays below 2^24 -- so a kernel's result must EQUAL
the float64 restatement, and one dropped, doubled or misplaced row shows.  Gaussian leg: the same against a bound."""
import functools
import math
import zlib

import numpy as np

from tests.util import random_voxels

FEAT_LIM, W_LIM = 3, 2  # integer leg: features, output gradients, residuals and initial dW in [-3, 3], weights in [-2, 2]


def wgrad_ref(X, G, tbl, K, M_out):
    """dW[k] = sum_o X[tbl[k, o]]^T G[o] in float64; tbl int32 [K, ld] (None: K = 1, the rows themselves)."""
    dW = np.zeros((K, X.shape[1], G.shape[1]))
    if tbl is None:
        dW[0] = X[:M_out].astype(np.float64).T @ G[:M_out].astype(np.float64)
        return dW
    for k in range(K):
        o = np.nonzero(tbl[k, :M_out] >= 0)[0]
        dW[k] = X[tbl[k, o]].astype(np.float64).T @ G[o].astype(np.float64)
    return dW


def dgrad_ref(G, W, tbl, M_in, M_out):
    """dX[tbl[k, o]] += G[o] W[k]^T in float64 (tbl[k] is injective, so a plain indexed += is right)."""
    dX = np.zeros((M_in, W.shape[1]))
    if tbl is None:
        dX[:M_out] = G[:M_out].astype(np.float64) @ W[0].astype(np.float64).T
        return dX
    for k in range(W.shape[0]):
        o = np.nonzero(tbl[k, :M_out] >= 0)[0]
        dX[tbl[k, o]] += G[o].astype(np.float64) @ W[k].astype(np.float64).T
    return dX


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def rows_operand(rng, shape, leg):
    """Features, output gradients, residuals, initial dW."""
    if leg == "int":
        return rng.integers(-FEAT_LIM, FEAT_LIM + 1, shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


def weight_operand(rng, K, Cin, Cout, leg):
    if leg == "int":
        return rng.integers(-W_LIM, W_LIM + 1, (K, Cin, Cout)).astype(np.float32)
    return (rng.standard_normal((K, Cin, Cout)) / math.sqrt(max(K // 3, 1) * Cin)).astype(np.float32)


def _round16(n):
    return (int(n) + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def voxels(name):
    """(coords int32 [M, 4], spatial shape, batch) of a named voxel set."""
    if name == "big":  # 137 slices of 1024 rows: the weight gradient's XCD order, ragged last round of 8; step + flat tables
        c, shape, B = random_voxels(np.random.default_rng(3), 140_000, (200, 180, 120), 2, True), (200, 180, 120), 2
        assert c.shape[0] == 140_000
    elif name == "mid":  # a deep level's size, ragged tail (3001 % 16 == 9)
        c, shape, B = random_voxels(np.random.default_rng(3001), 3001, (40, 36, 30), 1, True), (40, 36, 30), 1
        assert c.shape[0] == 3001
    elif name == "dense":  # the block of test_index_build_any_row_order, raster order: every offset in nearly every group
        shape, B = (40, 33, 70), 1
        d = np.stack(np.meshgrid(np.arange(8, 20), np.arange(5, 25), np.arange(0, 70), indexing="ij"), -1).reshape(-1, 3)
        c = np.concatenate([np.zeros((d.shape[0], 1), np.int64), d], 1).astype(np.int32)
    elif name == "tiny1":  # one partial group of one row
        c, shape, B = np.array([[0, 77, 3, 127]], np.int32), (128, 128, 128), 1
    elif name == "tiny17":  # isolated voxels (only the centre offset present), one full group and one row
        i = np.arange(17)
        c = np.stack([0 * i, 3 + 7 * i, 2 + (11 * i) % 120, 1 + (29 * i) % 120], 1).astype(np.int32)
        shape, B = (128, 128, 128), 1
    elif name == "tiny40":  # three groups, the last of 8 rows: most (slice, offset) lists are empty or one group long
        c, shape, B = random_voxels(np.random.default_rng(40), 40, (8, 8, 8), 1, False), (8, 8, 8), 1
        assert c.shape[0] == 40
    else:
        raise KeyError(name)
    return c, shape, B


def geometry(kind, M, Mc):
    """One forward convolution over a level of M voxels whose down-sampled level has Mc: offsets, rows, the table it
    gathers through (`tbl`), the table its input gradient gathers through (`btbl`) and whether that one takes the
    offset-flipped weights -- csrc/unet_train.hip conv_geom with the leading dimensions sparse.down_rules gives."""
    ld = max(_round16(M), 16)
    if kind == "subm":
        return dict(K=27, rows_in=M, rows_out=M, tbl="nbr", btbl="nbr", ld=ld, bld=ld, flip=1)
    if kind == "down":
        return dict(K=8, rows_in=M, rows_out=Mc, tbl="child", btbl="up", ld=ld, bld=ld, flip=0)
    if kind == "inv":
        return dict(K=8, rows_in=Mc, rows_out=M, tbl="up", btbl="child", ld=ld, bld=ld, flip=0)
    if kind == "1x1":
        return dict(K=1, rows_in=M, rows_out=M, tbl=None, btbl=None, ld=0, bld=0, flip=0)
    raise KeyError(kind)
