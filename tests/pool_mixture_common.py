"""What the tests of the mixture-proposal weights share (tests/test_gpu_pool_mixture.py, tests/test_pool_mixture_cpu.py): the shapes at
which the row-tiled kernel takes another path, the long-double log-sum-exp, and the bound of the tiled kernel.  Plain NumPy.  Not
collected by pytest.

Shapes (J, d) of pf_pool_mixture_tiled_kernel: one row past a row tile (1025), a 32-row step into the second tile and one row past it
(1056, 1057), two full tiles and one row past them (2048, 2049), kpad 12 / 20 / 32 (J = 6 / 10 / 16), a ragged second tile (1500), and ten
tiles with a short last one (10 000).  Pools (N_r, K): one column, fewer columns than a 16-column tile, three tiles with a ragged last
one and three components.
"""
import math

import numpy as np

LD = np.longdouble
SHAPES = [(6, 1025), (6, 1056), (6, 1057), (6, 2048), (10, 2049), (16, 1500), (6, 10000)]
POOLS = [(1, 1), (5, 2), (37, 3)]
FLOOR = 1e-13            # the bound test_gpu_mixture_geometry.py asserts for the log-sum-exp of the component kernels
FACTOR = 4.0             # the tiled kernel adds a column's terms in another order, over up to 10 row tiles, than the lane route


def lse_ld(comp):
    """log sum_k exp(comp[k]) over axis 0 in long double (finite inputs)"""
    c = np.asarray(comp, dtype=LD)
    m = np.max(c, axis=0)
    return m + np.log(np.sum(np.exp(c - m), axis=0))


def rel_to_lse(got, ref):
    """|got - ref| / max(|ref|, 1), the largest over the columns"""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref) / np.maximum(np.abs(ref), 1)))


def tiled_bound(lane_err):
    """what the tiled kernel's error relative to max(|lse|, 1) may be, given the lane route's error on the same columns"""
    return max(FACTOR * lane_err, FLOOR)


def log_k(K):
    """the double the library subtracts: log(K) of the C library"""
    return math.log(K)
