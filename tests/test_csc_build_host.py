"""Host side of the designs kept sparse (adelie_amd/csrc/csc_build_host.hpp) as a stand-alone program under the address and
undefined-behaviour sanitizers: no device, nothing loaded into Python.  The arrays are written here, every one sits in a heap
block of exactly its length inside the program (tests/native/csc_build_main.cpp), and what it prints is judged here."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAME = "sparse(): the two compressed forms must hold the same entries."
COL_SORT = "sparse(): row indices must be sorted and distinct inside a column."
ROW_SORT = "sparse(): column indices must be sorted and distinct inside a row."
ROW_RANGE = "sparse(): row index out of range."
COL_RANGE = "sparse(): column index out of range."
DISAGREE = "the row and column counts of the build disagree."


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    src = os.path.join(ROOT, "tests", "native", "csc_build_main.cpp")
    out = str(tmp_path_factory.mktemp("csc_build") / "csc_build")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, src])
    return out


def run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    return out.stdout.strip()


def forms(M, dtype=np.float64):
    """[indptr, indices, values, row_indptr, row_indices, row_values] of M in scipy's canonical forms"""
    c, r = sp.csc_matrix(M, dtype=dtype), sp.csr_matrix(M, dtype=dtype)
    for m in (c, r):
        m.sum_duplicates()
        m.sort_indices()
    return [c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data.copy(), r.indptr.astype(np.int64), r.indices.astype(np.int32), r.data.copy()]


def validate(exe, tmp_path, arrays, n, p):
    paths = []
    for k, a in enumerate(arrays):
        paths.append(str(tmp_path / f"a{k}.bin"))
        np.ascontiguousarray(a).tofile(paths[-1])
    return run(exe, ["validate", n, p, arrays[2].dtype.itemsize] + paths)


def random_case():
    rng = np.random.RandomState(4)
    n, p = 40, 13
    M = np.where(rng.uniform(size=(n, p)) < 0.2, rng.normal(size=(n, p)), 0.0)
    M[:, 5] = 0.0                                     # an empty column
    M[7, :] = 0.0                                     # an empty row
    M[[3, 11, 20], 2] = (1.5, -2.0, 0.25)             # a column and a row with three entries at least
    M[9, [1, 6, 12]] = (0.5, 4.0, -1.0)
    M[n - 1, 0] = 2.0                                 # the last row is not empty
    return M, n, p


def test_validator_accepts_canonical_pairs(exe, tmp_path):
    small = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 4.0]])
    M, n, p = random_case()
    for dtype in (np.float64, np.float32):
        assert validate(exe, tmp_path, forms(small, dtype), 3, 2) == "ok"
        assert validate(exe, tmp_path, forms(M, dtype), n, p) == "ok"
    assert validate(exe, tmp_path, forms(np.zeros((3, 2))), 3, 2) == "ok"      # no entries: the index arrays are empty


def test_validator_refuses_with_the_entry_points_messages(exe, tmp_path):
    M, n, p = random_case()
    good = forms(M)
    cptr, rptr = good[0], good[3]

    def damaged(which, edit):
        a = [x.copy() for x in good]
        edit(a[which + 1], a[which + 2])               # (the indices and the values of the form that starts at `which`)
        return validate(exe, tmp_path, a, n, p)

    def swap(k):
        def f(idx, val):
            idx[[k, k + 1]] = idx[[k + 1, k]]
            val[[k, k + 1]] = val[[k + 1, k]]
        return f

    def put(k, v):
        def f(idx, val):
            idx[k] = v
        return f

    assert cptr[3] - cptr[2] >= 3 and rptr[10] - rptr[9] >= 3
    assert damaged(0, swap(cptr[2])) == COL_SORT                               # an unsorted column
    assert damaged(0, put(cptr[2] + 1, good[1][cptr[2]])) == COL_SORT          # a duplicate row in a column
    assert damaged(0, put(cptr[3] - 1, n)) == ROW_RANGE                        # a row index equal to n
    assert damaged(0, put(cptr[2], -1)) == ROW_RANGE                           # a negative index
    assert damaged(3, swap(rptr[9])) == ROW_SORT                               # an unsorted row
    assert damaged(3, put(rptr[10] - 1, p)) == COL_RANGE                       # a column index equal to p
    assert damaged(3, put(rptr[9], -1)) == COL_RANGE

    def one_value(idx, val):
        val[len(val) // 2] += 1.0
    assert damaged(3, one_value) == SAME                                       # one value differing between the forms
    assert damaged(0, one_value) == SAME
    # equal totals, equal counts per column and per row, two entries swapped between columns: (i1, c1), (i2, c2) in the column
    # form against (i1, c2), (i2, c1) in the row form, all values equal -- only the checksum can tell
    B = (M != 0).astype(np.float64)
    i1, c1, i2, c2 = next((i1, c1, i2, c2) for i1 in range(n) for i2 in range(n) for c1 in range(p) for c2 in range(p)
                          if B[i1, c1] and B[i2, c2] and not B[i1, c2] and not B[i2, c1])
    B2 = B.copy()
    B2[i1, c1] = B2[i2, c2] = 0.0
    B2[i1, c2] = B2[i2, c1] = 1.0
    a, b = forms(B), forms(B2)
    assert np.array_equal(np.diff(a[0]), np.diff(b[0])) and np.array_equal(np.diff(a[3]), np.diff(b[3]))
    assert validate(exe, tmp_path, a[:3] + b[3:], n, p) == SAME
    # the pointer arrays
    bad = [x.copy() for x in good]
    bad[3][-1] -= 1
    assert validate(exe, tmp_path, bad, n, p) == SAME                          # (the totals differ)
    bad = [x.copy() for x in good]
    bad[0][0] = 1
    assert validate(exe, tmp_path, bad, n, p) == "sparse(): indptr must start at 0."


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("doubled", [False, True])
@pytest.mark.parametrize("counts", ["random", "zero", "row_off_by_one"])
def test_offsets_against_cumsum(exe, tmp_path, nt, doubled, counts):
    rng = np.random.RandomState(7)
    counted, n = 6, 11
    cols = counted * (2 if doubled else 1)
    col_cnt = np.zeros(counted * nt, dtype=np.int32) if counts == "zero" else rng.randint(0, 5, size=counted * nt).astype(np.int32)
    total = int(np.tile(col_cnt, cols // counted).sum())
    row_cnt = rng.multinomial(total, np.ones(n) / n).astype(np.int64)          # any split of the total over the rows
    if counts == "row_off_by_one":
        row_cnt[n // 2] += 1
    cpath, rpath, opath = (str(tmp_path / f) for f in ("c.bin", "r.bin", "o.bin"))
    col_cnt.tofile(cpath)
    row_cnt.tofile(rpath)
    msg = run(exe, ["offsets", counted, cols, nt, n, cpath, rpath, opath])
    assert msg == (DISAGREE if counts == "row_off_by_one" else "ok")
    got = np.fromfile(opath, dtype=np.int64)
    assert got.size == (cols + 1) + cols * nt + (n + 1) + 1
    cptr, col_pos, rptr, tot = np.split(got, [cols + 1, cols + 1 + cols * nt, cols + 1 + cols * nt + n + 1])
    starts = np.concatenate([[0], np.cumsum(np.tile(col_cnt, cols // counted).astype(np.int64))])
    assert np.array_equal(col_pos, starts[:-1]) and np.array_equal(cptr, starts[::nt]) and tot[0] == total == cptr[-1]
    assert np.array_equal(rptr, np.concatenate([[0], np.cumsum(row_cnt)]))
