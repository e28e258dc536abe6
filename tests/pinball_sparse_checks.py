"""Sparse constraint matrices for the tests of solver.pinball on matrix.sparse(method="constraint"): the problems of
tests/pinball_checks.py with most entries of A struck out.  The restatement is pinball_checks.solve on the resulting array;
structural zeros are exact zeros to it, so it is the reference of the sparse and of the dense route alike."""
import functools

import numpy as np

import pinball_checks as pc

# (m, d, kappa, pen, density, wide): d = 1 | rows of 0-5 entries | more than one wavefront of members | m < d | 15-17 KKT rounds,
# H appended 7 at a time (the rows-for-old-members launch) | the larger ns | rows of ~150 entries and one of 300: more than a
# wavefront and more than a tile per row
GRID = [(3, 1, None, 1.0, 1.0, False), (20, 5, None, 1.0, 0.4, False), (130, 40, None, 0.3, 0.1, False),
        (40, 100, None, 0.3, 0.05, False), (300, 64, 7, 0.1, 0.1, False), (2000, 100, None, 0.1, 0.03, False),
        (130, 300, None, 0.3, 0.5, True)]
GRID32 = [GRID[0], GRID[1], GRID[3]]
SEEDS = range(3)
GAP64 = 1e-9
GAP32 = 1e-3
EDGE_DENSITY = 0.5


def sgen(m, d, seed, pen, density, wide=False):
    """pinball_checks.gen(m, d, seed, pen) with A[i, j] kept where a seeded uniform draw is below `density`; for m > 4 row
    m // 2 is emptied; `wide` restores row 1 in full."""
    A, S, v, pneg, ppos = pc.gen(m, d, seed, pen)
    keep = np.random.RandomState(1000 + seed).uniform(size=(m, d)) < density
    As = np.where(keep, A, 0.0)
    if m > 4:
        As[m // 2] = 0
    if wide:
        As[1] = A[1]
    return As, S, v, pneg, ppos


def sedge(seed, density=EDGE_DENSITY):
    """pinball_checks.edge(seed) struck out the same way: the zero row, the repeated row and the infinite penalties stay."""
    A, S, v, pneg, ppos = pc.edge(seed)
    keep = np.random.RandomState(1000 + seed).uniform(size=A.shape) < density
    As = np.where(keep, A, 0.0)
    As[7] = As[6]
    return As, S, v, pneg, ppos


@functools.lru_cache(maxsize=None)
def cached_inputs(m, d, seed, pen, density, wide=False, round32=False):
    """sgen(...), or sedge(seed) when m is the string "edge"; `round32`: A, S, v rounded to float32 first."""
    A, S, v, pneg, ppos = sedge(seed, density) if m == "edge" else sgen(m, d, seed, pen, density, wide)
    if round32:
        A, S, v = A.astype(np.float32), np.asfortranarray(S.astype(np.float32)), v.astype(np.float32)
    for x in (A, S, v, pneg, ppos):
        x.setflags(write=False)
    return A, S, v, pneg, ppos


@functools.lru_cache(maxsize=None)
def cached_run(m, d, seed, pen, density, wide, kappa, dtype, round32=False, tol=1e-7):
    """The restatement on a generated problem (shared by the tests; nobody modifies the result)."""
    A, S, v, pneg, ppos = cached_inputs(m, d, seed, pen, density, wide, round32)
    return pc.solve(A, S, v, pneg, ppos, np.dtype(dtype), kappa=kappa, tol=tol)
