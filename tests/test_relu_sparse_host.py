"""Host-side logic of matrix.convex_relu over a sparse base: the scipy restatement of the expansion against the dense numpy
one, the stored-entry formula, the argument errors that need no device, the row tiles and mask words of the builder and the
structured sweep (adelie_amd/csrc/relu_sparse_shape.hpp) as a stand-alone program under the address and undefined-behaviour
sanitizers, its Python restatement, and the entry point's place in the ABI tables.  None of it needs a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy.sparse import csc_matrix

from adelie_amd import _abi
from adelie_amd import matrix as M
from relu_sparse_checks import make_inputs, stored_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dead_row", [False, True])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,d,m", [(1, 3, 1), (5, 3, 4), (257, 17, 19), (64, 2, 70)])
def test_sparse_expansion_equals_the_dense_one(n, d, m, dtype, gated, dead_row):
    Z, mask = make_inputs(n, d, m, dtype, dead_row=dead_row)
    if d >= 2:
        assert Z[:, 1].nnz == 0                                           # an empty column
    if n >= 2:
        assert Z[n // 2, :].nnz == 0                                      # an empty row
    if m >= 2:
        assert not mask[:, 0].any() and mask[:n - 1, m - 1].all()        # a mask column all false, one all true
    if dead_row:
        assert not mask[n - 1].any()                                     # a row with every gate false
    S = M._relu_expand_sparse(Z, mask, gated)
    E = csc_matrix(M._relu_expand(Z.toarray(), mask, gated))
    E.sort_indices()
    assert isinstance(S, csc_matrix) and S.dtype == dtype and S.shape == E.shape == (n, (1 if gated else 2) * m * d)
    assert S.has_sorted_indices and (S.data != 0).all()
    assert np.array_equal(S.indptr, E.indptr) and np.array_equal(S.indices, E.indices) and np.array_equal(S.data, E.data)
    assert S.nnz == stored_entries(Z, mask, gated)


def test_sparse_expansion_prunes_sums_and_selects():
    # duplicates are summed, explicit zeros dropped; a stored inf in a masked-out row leaves no entry, one in a masked-in row stays
    rows, cols, vals = [0, 0, 1, 2, 2], [0, 0, 1, 0, 1], [1.0, 2.0, 0.0, np.inf, np.inf]
    Z = csc_matrix((np.array(vals), (rows, cols)), shape=(3, 2))
    Z.sum_duplicates()
    assert Z.nnz == 4 and (Z.data == 0).any()   # (the explicit zero is stored)
    mask = np.array([[True, False], [True, True], [False, True]])
    S = M._relu_expand_sparse(Z, mask, False).toarray()
    E = np.zeros((3, 8))
    E[0, 0] = 3.0                     # gate 0: row 0 on
    E[2, 2], E[2, 3] = np.inf, np.inf  # gate 1: row 2 on, inf stays
    E[:, 4:] = -E[:, :4]
    assert np.array_equal(S, E)
    assert M._relu_expand_sparse(Z, mask, True).nnz == 3
    assert Z.nnz == 4                  # (the input is left as it was)


def test_argument_errors_need_no_device():
    import adelie_amd as ad

    Zs, mask = make_inputs(5, 3, 2, np.float64)
    with pytest.raises(ValueError, match="resident must be one of 'dense' or 'csc'"):
        ad.matrix.convex_relu(Zs, mask, resident="auto")
    with pytest.raises(ValueError, match="resident must be one of 'dense' or 'csc'"):
        ad.matrix.convex_relu(Zs.toarray(), mask, resident="sparse")
    with pytest.raises(RuntimeError, match="no compressed arrays"):
        ad.matrix.convex_relu(np.asfortranarray(Zs.toarray()), mask, resident="csc")
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.convex_relu(Zs, mask, resident="csc", n_threads=0)


def test_shape_functions_under_sanitizers(tmp_path):
    """relu_sparse_shape / relu_sparse_sweep_work_elems over a grid of (n, m) (tests/native/relu_sparse_shape_main.cpp); and
    the table it prints is what matrix._relu_sparse_sweep_shape restates."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(ROOT, "tests", "native", "relu_sparse_shape_main.cpp")
    exe = str(tmp_path / "relu_sparse_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True)
    assert out.returncode == 0 and "relu_sparse_shape: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines() if re.fullmatch(r"[\d ]+", ln)]
    assert len(rows) == 18 * 11
    assert {r[0] for r in rows} >= {0, 1, 8229, 65537} and {r[1] for r in rows} >= {1, 32, 33, 64, 65}
    for n, m, *shape in rows:
        assert M._relu_sparse_sweep_shape(n, m) == tuple(shape), (n, m)
    assert any(r[3] >= 3 for r in rows) and max(r[3] for r in rows) == 16
    assert M._relu_sparse_sweep_shape(8229, 19) == (4096, 3, 1)


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "adelie_amd", "csrc", "relu_sparse_shape.hpp")).read()
    for name, val in (("kReluSpWordBits", M._RELU_SP_WORD_BITS), ("kReluSpTileUnit", M._RELU_SP_TILE_UNIT),
                      ("kReluSpMaxTiles", M._RELU_SP_MAX_TILES)):
        assert int(re.search(rf"constexpr (?:int|int64_t) {name} = (\d+);", txt).group(1)) == val


def test_abi_tables_name_the_entry_point():
    assert "design_create_convex_relu_csc" in _abi.HIP_SYMBOLS
    assert _abi.ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "adelie_hip.h")).read()
    assert re.search(r"int adelie_hip_design_create_convex_relu_csc\(adelie_hip_design\* Z, const uint8_t\* mask, int64_t m, int gated,\s*"
                     r"adelie_hip_design\*\* out\);", hdr)
