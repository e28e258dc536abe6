"""Host side of the covariance matrix kept sparse (adelie_amd/csrc/cov_csc_host.hpp) as a stand-alone program under the address
and undefined-behaviour sanitizers (no device, nothing loaded into Python; tests/native/cov_csc_main.cpp), the properties of
the generators the GPU tests rely on (tests/cov_sparse_checks.py), and the CPU oracle on every grid case."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import cov_sparse_checks as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

START = "sparse(): indptr must start at 0."
DECREASE = "sparse(): indptr must be non-decreasing."
COL_SORT = "sparse(): row indices must be sorted and distinct inside a column."
ROW_RANGE = "sparse(): row index out of range."


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    src = os.path.join(ROOT, "tests", "native", "cov_csc_main.cpp")
    out = str(tmp_path_factory.mktemp("cov_csc") / "cov_csc")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, src])
    return out


def run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    return out.stdout.strip()


def form(M, dtype=np.float64):
    """[indptr, indices, values] of M in scipy's canonical column-compressed form"""
    c = sp.csc_matrix(M, dtype=dtype)
    c.sum_duplicates()
    c.sort_indices()
    return [c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data.copy()]


def validate(exe, tmp_path, arrays, p):
    paths = []
    for k, a in enumerate(arrays):
        paths.append(str(tmp_path / f"a{k}.bin"))
        np.ascontiguousarray(a).tofile(paths[-1])
    return run(exe, ["validate", p] + paths)


def test_validator_accepts_canonical_forms(exe, tmp_path):
    A = cc.problem(cc.GRID[1])[0]
    for dtype in (np.float64, np.float32):
        assert validate(exe, tmp_path, form(A, dtype), 23) == "ok"
        assert validate(exe, tmp_path, form(np.array([[2.0]]), dtype), 1) == "ok"          # p = 1
    assert validate(exe, tmp_path, form(np.zeros((4, 4))), 4) == "ok"                      # no entries: the index arrays are empty
    assert validate(exe, tmp_path, form(np.zeros((1, 1))), 1) == "ok"
    assert validate(exe, tmp_path, form(np.diag([1.0, 0.0, 3.0])), 3) == "ok"              # columns of one entry and of none
    lone = cc.lone_diag_matrix()
    assert validate(exe, tmp_path, form(lone), lone.shape[0]) == "ok"


def test_validator_refuses_with_the_entry_points_messages(exe, tmp_path):
    A = cc.problem(cc.GRID[1])[0]
    p = 23
    good = form(A)
    cptr = good[0]
    assert cptr[6] - cptr[5] >= 3

    def damaged(edit):
        a = [x.copy() for x in good]
        edit(*a)
        return validate(exe, tmp_path, a, p)

    def swap(ptr, idx, val):
        k = cptr[5]
        idx[[k, k + 1]] = idx[[k + 1, k]]
        val[[k, k + 1]] = val[[k + 1, k]]

    def put(k, v):
        def f(ptr, idx, val):
            idx[k] = v
        return f

    def ptr_put(k, v):
        def f(ptr, idx, val):
            ptr[k] = v
        return f

    assert damaged(swap) == COL_SORT                                       # an unsorted column
    assert damaged(put(cptr[5] + 1, good[1][cptr[5]])) == COL_SORT         # a duplicate row in a column
    assert damaged(put(cptr[5], -1)) == ROW_RANGE                          # an index of -1
    assert damaged(put(cptr[6] - 1, p)) == ROW_RANGE                       # an index of p
    assert damaged(put(len(good[1]) - 1, p)) == ROW_RANGE                  # ... in the last entry of all
    assert damaged(ptr_put(0, 1)) == START
    assert damaged(ptr_put(5, cptr[6] + 1)) == DECREASE                    # indptr[5] > indptr[6]
    assert damaged(ptr_put(p, cptr[p - 1] - 1)) == DECREASE                # the entry count below the last column's start


def test_lane_choice_and_column_cover(exe):
    lanes = set()
    for nnz, p in [(0, 1), (1, 1), (8, 1), (9, 1), (64, 1), (65, 1), (5 * 10 ** 8, 10 ** 6), (17 * 250000, 250000), (3, 1000)]:
        L = int(run(exe, ["lanes", nnz, p]))
        assert L in (4, 16, 64)
        lanes.add(L)
    assert lanes == {4, 16, 64}
    assert int(run(exe, ["lanes", 8, 1])) == 4 and int(run(exe, ["lanes", 9, 1])) == 16
    assert int(run(exe, ["lanes", 64, 1])) == 16 and int(run(exe, ["lanes", 65, 1])) == 64
    for ncols in (1, 63, 64, 65, 100000):
        for L in (4, 16, 64):
            word, blocks, per_block = run(exe, ["cover", ncols, L]).split()
            assert word == "ok" and int(per_block) == 256 // L
            assert int(blocks) == -(-ncols // int(per_block))              # no block without a column


def test_generators_have_the_properties_the_gpu_tests_rely_on():
    for case in cc.GRID:
        n, p, w, G = case
        A, v = cc.problem(case)
        assert A.shape == (p, p) and v.shape == (p,) and np.array_equal(A, A.T)
        assert np.linalg.eigvalsh(A).min() > -1e-12                        # positive semi-definite
        i, j = np.nonzero(A)
        assert np.abs(i - j).max() <= w - 1                                # exact zeros outside the band of 2w - 1
        assert cc.col_counts(A).max() == min(2 * w - 1, p)
        assert p % G == 0
    assert cc.col_counts(cc.problem(cc.WIDE)[0]).max() > 256               # more than one pass of a 64-lane group
    assert np.all(cc.problem(cc.DENSE)[0] != 0)                            # fully dense
    lone = cc.lone_diag_matrix()
    assert cc.col_counts(lone)[cc.LONE] == 1 and lone[cc.LONE, cc.LONE] == 1.0 and np.array_equal(lone, lone.T)
    assert cc.col_counts(lone).max() > 1
    B, vb = cc.block_diag_matrix()
    assert B.shape == (sum(cc.BLOCKS),) * 2 and int((B != 0).sum()) == sum(q * q for q in cc.BLOCKS)
    assert np.linalg.eigvalsh(B).min() > 0


@pytest.mark.parametrize("case", cc.GRID)
def test_oracle_solves_every_grid_case(oracle, case):
    st = cc.oracle_path(case)
    assert st.error == "" and len(st.lmdas) == 30
    if case in (cc.GRID[3], cc.GROUPED):
        assert cc.screen_values(st, case) >= 256                           # the multi-CU Gram engines' range
