"""Host-side logic of matrix.convex_relu: the column order j <-> (sgn, j_m, j_d) and the numpy expansion against a literal
restatement of the reference's _cmul indexing (matrix_naive_convex_relu.ipp:17-25), the grid of the structured sweep
(adelie_amd/csrc/relu_shape.hpp) as a stand-alone program under the address and undefined-behaviour sanitizers, its Python
restatement, and the entry point's place in the ABI tables.  None of it needs a device."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from adelie_amd import _abi
from adelie_amd import matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_column(Z, mask, j):
    """Column j as the reference's _cmul reads it: j_sgn = j / (m d); j -= j_sgn m d; j_m = j / d; j -= j_m d; j_d = j;
    (1 - 2 j_sgn) * (mat.col(j_d) o mask.col(j_m))."""
    d, m = Z.shape[1], mask.shape[1]
    j_sgn = j // (m * d)
    j -= j_sgn * m * d
    j_m = j // d
    j -= j_m * d
    j_d = j
    return (1 - 2 * j_sgn) * (Z[:, j_d] * mask[:, j_m].astype(Z.dtype))


@pytest.mark.parametrize("gated", [True, False])
def test_column_order_and_expansion(gated):
    rng = np.random.RandomState(0)
    n, d, m = 5, 3, 4
    Z = rng.normal(size=(n, d))
    mask = rng.uniform(size=(n, m)) < 0.5
    mask[:, 1], mask[:, 2] = False, True
    E = M._relu_expand(Z, mask, gated)
    P = (1 if gated else 2) * m * d
    assert E.shape == (n, P) and E.dtype == Z.dtype and E.flags.f_contiguous
    seen = set()
    for j in range(P):
        sgn, j_m, j_d = M._relu_column(j, d, m)
        assert 0 <= sgn < (1 if gated else 2) and 0 <= j_m < m and 0 <= j_d < d
        assert j == sgn * (m * d) + j_m * d + j_d
        seen.add((sgn, j_m, j_d))
        assert np.array_equal(E[:, j], _reference_column(Z, mask, j))
        assert np.array_equal(E[:, j], (1 - 2 * sgn) * np.where(mask[:, j_m], Z[:, j_d], 0.0))
    assert len(seen) == P
    assert not E[:, d:2 * d].any() and np.array_equal(E[:, 2 * d:3 * d], Z)   # the all-false and the all-true mask column


def test_expansion_is_a_select():
    Z = np.array([[np.inf, 1.0], [2.0, np.nan], [3.0, 4.0]])
    mask = np.array([[False], [False], [True]])
    E = M._relu_expand(Z, mask, False)
    assert np.array_equal(E, np.array([[0, 0, 0, 0], [0, 0, 0, 0], [3, 4, -3, -4.0]]))
    assert M._relu_expand(Z.astype(np.float32), mask, True).dtype == np.float32


def test_shape_functions_under_sanitizers(tmp_path):
    """relu_shape / relu_sweep_work_elems over a grid of (n, d, m) with n = 0, 1 and d, m = 1, 16, 17 among them: the slices
    cover [0, n) exactly once, the partial sums fit the work buffer and are written once each (tests/native/
    relu_shape_main.cpp); and the table it prints is what matrix._relu_sweep_shape restates."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(ROOT, "tests", "native", "relu_shape_main.cpp")
    exe = str(tmp_path / "relu_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe, "--table"], capture_output=True, text=True)
    assert out.returncode == 0 and "relu_shape: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines() if re.fullmatch(r"[\d ]+", ln)]
    assert len(rows) == 18 * 8 * 8
    assert {r[0] for r in rows} >= {0, 1} and {r[1] for r in rows} >= {1, 16, 17} and {r[2] for r in rows} >= {1, 16, 17}
    for n, d, m, *shape in rows:
        assert M._relu_sweep_shape(n, d, m) == tuple(shape), (n, d, m)
    assert any(r[5] >= 3 for r in rows)


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "adelie_amd", "csrc", "relu_shape.hpp")).read()
    for name, val in (("kReluTile", M._RELU_TILE), ("kReluMT", M._RELU_MT), ("kReluRun", M._RELU_RUN)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", txt).group(1)) == val


def test_abi_tables_name_the_entry_point():
    assert "design_create_convex_relu" in _abi.HIP_SYMBOLS
    assert _abi.ABI_VERSION == 14
    hdr = open(os.path.join(ROOT, "include", "adelie_hip.h")).read()
    assert re.search(r"#define ADELIE_HIP_ABI_VERSION 14\b", hdr)
    assert re.search(r"int adelie_hip_design_create_convex_relu\(adelie_hip_design\* Z, const uint8_t\* mask, int64_t m, int gated,\s*"
                     r"adelie_hip_design\*\* out\);", hdr)


def test_front_door_checks_need_no_device():
    import adelie_amd as ad

    assert callable(ad.matrix.convex_relu)
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.convex_relu(np.zeros((3, 2), order="F"), np.ones((3, 1), dtype=bool), n_threads=0)
