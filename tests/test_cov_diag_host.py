"""Host side of the lambda-batched covariance product (adelie_amd/csrc/cov_batch_host.hpp: the checks of the caller's CSR rows,
the chunking of the rows and the union plan of the dense-storage kernel) as a stand-alone program under the address and
undefined-behaviour sanitizers (no device, nothing loaded into Python; tests/native/cov_batch_main.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB = 8

RANGE = "mul_batch: column index out of range."
ORDER = "mul_batch: column indices must be ascending and distinct inside a row."
START = "mul_batch: indptr must start at 0."
DECREASE = "mul_batch: indptr must be non-decreasing."


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    src = os.path.join(ROOT, "tests", "native", "cov_batch_main.cpp")
    out = str(tmp_path_factory.mktemp("cov_batch") / "cov_batch")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, src])
    return out


def run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    return out.stdout.strip()


def files(tmp_path, arrays):
    paths = []
    for k, a in enumerate(arrays):
        paths.append(str(tmp_path / f"a{k}.bin"))
        np.ascontiguousarray(a).tofile(paths[-1])
    return paths


def form(B):
    """[indptr, indices, values] of the canonical CSR form of B, as the entry point takes them"""
    c = sp.csr_matrix(B, dtype=np.float64)
    c.sum_duplicates()
    c.sort_indices()
    return [c.indptr.astype(np.int64), c.indices.astype(np.int64), c.data.astype(np.float64)]


def validate(exe, tmp_path, L, p, indptr, indices):
    return run(exe, ["validate", L, p] + files(tmp_path, [np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)]))


def plan(exe, tmp_path, B, p, elem=8):
    """The program's plan of B's rows as a list of chunks (l0, lc, [(columns, coef (n, LB))])"""
    text = run(exe, ["plan", B.shape[0], p, elem] + files(tmp_path, form(B)))
    lines = text.split("\n")
    assert lines[-1] == "done", text[-500:]
    chunks, k = [], 0
    while lines[k] != "done":
        word, l0, lc, nb = lines[k].split()
        assert word == "chunk"
        k += 1
        batches = []
        for _ in range(int(nb)):
            word, n = lines[k].split()
            assert word == "batch"
            rows = [lines[k + 1 + i].split() for i in range(int(n))]
            k += 1 + int(n)
            cols = np.array([int(r[0]) for r in rows], dtype=np.int64)
            coef = np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(int(n), LB)
            batches.append((cols, coef))
        chunks.append((int(l0), int(lc), batches))
    return chunks


def check_plan(chunks, B, chunk_rows):
    """Chunks tile the rows in order; every batch's columns are the ascending union of its rows' indices and its coefficient block
    holds the rows' values there and exact zeros elsewhere."""
    L = B.shape[0]
    D = np.asarray(B.todense())
    S = sp.csr_matrix(B)
    assert [c[0] for c in chunks] == list(range(0, L, chunk_rows))
    for l0, lc, batches in chunks:
        assert lc == min(chunk_rows, L - l0) and len(batches) == -(-lc // LB)
        for b, (cols, coef) in enumerate(batches):
            r0 = l0 + b * LB
            rows = min(LB, l0 + lc - r0)
            union = np.unique(np.concatenate([S[r].indices for r in range(r0, r0 + rows)] + [np.empty(0, dtype=np.int64)]))
            assert np.array_equal(cols, union)
            assert np.array_equal(coef[:, :rows], D[r0:r0 + rows][:, cols].T)
            assert np.all(coef[:, rows:] == 0)


def test_validator(exe, tmp_path):
    assert validate(exe, tmp_path, 0, 5, [], []) == "ok"                               # an empty batch: no rows, no arrays
    assert validate(exe, tmp_path, 3, 5, [0, 2, 2, 3], [1, 4, 0]) == "ok"              # a row with no entries
    assert validate(exe, tmp_path, 2, 5, [0, 0, 0], []) == "ok"                        # no entries at all
    assert validate(exe, tmp_path, 1, 1, [0, 1], [0]) == "ok"                          # p = 1
    assert validate(exe, tmp_path, 1, 5, [0, 5], [0, 1, 2, 3, 4]) == "ok"              # a fully dense row
    assert validate(exe, tmp_path, 2, 5, [0, 2, 3], [1, 5, 0]) == RANGE                # an index equal to p
    assert validate(exe, tmp_path, 2, 5, [0, 2, 3], [1, 4, 5]) == RANGE                # ... in the last entry of all
    assert validate(exe, tmp_path, 2, 5, [0, 2, 3], [-1, 4, 0]) == RANGE
    assert validate(exe, tmp_path, 2, 5, [0, 2, 3], [4, 1, 0]) == ORDER                # a descending pair
    assert validate(exe, tmp_path, 2, 5, [0, 2, 3], [1, 1, 0]) == ORDER                # a repeated index
    assert validate(exe, tmp_path, 2, 5, [0, 1, 3], [4, 1, 3]) == "ok"                 # descending across two rows is fine
    assert validate(exe, tmp_path, 2, 5, [1, 2, 3], [1, 4, 0]) == START
    assert validate(exe, tmp_path, 2, 5, [0, 2, 1], [1, 4, 0]) == DECREASE
    assert validate(exe, tmp_path, -1, 5, [], []) == "mul_batch: L must be >= 0."


def test_chunk_rows_are_whole_batches_within_the_bound(exe):
    for p, elem in [(1, 8), (37, 4), (20000, 8), (250000, 8), (10 ** 6, 8), (10 ** 6, 4), (5 * 10 ** 7, 8), (2 ** 31 - 1, 8)]:
        rows = int(run(exe, ["chunk", p, elem]))
        assert rows % LB == 0 and LB <= rows <= 16 * LB
        assert rows == LB or rows * p * elem <= 256 << 20                              # one batch, or within 256 MiB
    assert int(run(exe, ["chunk", 1, 8])) == 16 * LB and int(run(exe, ["chunk", 5 * 10 ** 7, 8])) == LB


def test_plan_of_an_empty_batch_and_of_single_rows(exe, tmp_path):
    assert plan(exe, tmp_path, sp.csr_matrix((0, 7)), 7) == []
    B = sp.csr_matrix(np.array([[0.0, 0.0, 0.0]]))
    chunks = plan(exe, tmp_path, B, 3)
    assert len(chunks) == 1 and len(chunks[0][2]) == 1 and len(chunks[0][2][0][0]) == 0   # a row with no entries: an empty union
    check_plan(plan(exe, tmp_path, sp.csr_matrix(np.array([[0.0, -2.5, 0.0, 1.0]])), 4), sp.csr_matrix(np.array([[0.0, -2.5, 0.0, 1.0]])), 128)


@pytest.mark.parametrize("L", [1, 7, 8, 9, 17, 130])
def test_plan_unions(exe, tmp_path, L):
    """L on both sides of a batch and of a chunk of 128 rows; an empty row, a fully dense row, unions larger than the batch."""
    p = 41
    rng = np.random.RandomState(L)
    D = rng.normal(size=(L, p)) * (rng.uniform(size=(L, p)) < 0.2)
    D[L // 2] = 0
    D[-1] = rng.normal(size=p)
    B = sp.csr_matrix(D)
    chunks = plan(exe, tmp_path, B, p)
    check_plan(chunks, B, 128)
    assert max(len(c) for _, _, bs in chunks for c, _ in bs) > min(LB, L)


def test_a_union_that_spans_several_chunks(exe, tmp_path):
    """p so large that a chunk is one batch: 20 rows are three chunks, and a column that every row has shows up in each of them."""
    p = 5 * 10 ** 7
    rng = np.random.RandomState(3)
    L = 20
    rows, cols, vals = [], [], []
    for l in range(L):
        c = np.unique(np.concatenate([[12345678], rng.randint(0, p, 5)]))
        rows += [l] * len(c)
        cols += list(c)
        vals += list(rng.normal(size=len(c)))
    B = sp.csr_matrix((vals, (rows, cols)), shape=(L, p))
    chunks = plan(exe, tmp_path, B, p)
    assert [(l0, lc) for l0, lc, _ in chunks] == [(0, 8), (8, 8), (16, 4)]
    S = B.tocsr()
    for l0, lc, batches in chunks:
        (cols_b, coef), = batches
        union = np.unique(np.concatenate([S[r].indices for r in range(l0, l0 + lc)]))
        assert np.array_equal(cols_b, union) and 12345678 in cols_b
        k = int(np.flatnonzero(cols_b == 12345678)[0])
        shared = [S[l0 + r].data[np.searchsorted(S[l0 + r].indices, 12345678)] for r in range(lc)]
        assert np.array_equal(coef[k, :lc], shared) and np.all(coef[k, lc:] == 0)
        for r in range(lc):
            row = S[l0 + r]
            assert np.array_equal(coef[np.searchsorted(cols_b, row.indices), r], row.data)
            assert np.count_nonzero(coef[:, r]) == np.count_nonzero(row.data)
