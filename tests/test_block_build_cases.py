"""The case table of the block-build tests (tests/block_build_checks.py), checked without a GPU: the exact leg of every case
really is exact in the case's type, the references of the two legs agree, the table names every variant the kernels have, and
the shape functions the launchers share (adelie_amd/csrc/gram_shape.hpp) hold their invariants under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import block_build_checks as bb

_designs = {}


def _values(case, leg):
    key = bb.design_key(case) + (leg,)
    if key not in _designs:
        _designs[key] = bb.make_design_values(case.kind, case.dtype, case.n + case.row_off, leg)[0]
    return _designs[key][case.row_off:]


def test_exact_leg_is_exact_for_every_case():
    """16 max (sum |w x x| + |xm xm|) is a whole number below 2^24 (float32) / 2^53 (float64), the inputs are what the leg
    promises, and every value of the reference is representable in the case's type."""
    worst = {}
    for case in bb.CASES:
        X = _values(case, "exact")
        w, xm = bb.make_vectors(case, "exact", X)
        assert X.shape[0] == case.n and np.abs(X).max() <= 3 and (X * 2 == np.round(X * 2)).all()
        if case.kind != "snp":
            assert (X == np.round(X)).all()
        assert set(np.unique(w)) <= {0.0, 0.5, 1.0, 2.0} and (case.n < 8 or (w == 0).any())
        assert np.abs(xm).max() <= 4 and (xm * 4 == np.round(xm * 4)).all()
        h = bb.exact_headroom(case, X, w, xm)
        assert h < bb.EXACT_LIMIT[case.dtype], (case.name, h)
        worst[case.dtype] = max(worst.get(case.dtype, 0.0), h)
        T = bb.NP_TYPE[case.dtype]
        for ref, _, foot in bb.expected(case, X, w, xm, "exact"):
            assert (ref.astype(T).astype(np.float64) == ref).all()
            assert foot.size == 0 or foot.any() or ref.size == case.out1
    print("largest 16 H: f32 %.0f of 2^24 = %d, f64 %.0f" % (worst["f32"], 2 ** 24, worst["f64"]))
    assert worst["f32"] > 2 ** 18   # the float32 cases are not trivially small: n = 8320 is in the table


def test_rounding_leg_bound_covers_a_float64_product():
    """The derived bound against numpy's own float64 (and float32) product of the same rounded inputs on a few cases: a plain
    product in the case's type stays inside it, one in float32 of float64 inputs does not."""
    for name in ("syrk-dense-f64-n1000-M100", "syrk-dense-f32-n1000-M128", "gram-dense-f64-n1000-M300-N200-sym",
                 "strip-f64-lt-n8320-64.64.128"):
        case = bb.CASE_BY_NAME[name]
        X = _values(case, "rounding")
        w, xm = bb.make_vectors(case, "rounding", X)
        T = bb.NP_TYPE[case.dtype]
        blk = case.blocks[0]
        G, S, Q = bb.block_reference(case, blk, X, w, xm, True)
        bound = (case.n + 4) * bb.UNIT[case.dtype] * S + 2 * bb.UNIT[case.dtype] * Q

        def product(U):
            A, B = X[:, blk.rows].astype(U), (X[:, blk.cols].astype(U) * w.astype(U)[:, None])
            C = A.T @ B
            return (C - np.outer(xm[blk.rows].astype(U), xm[blk.cols].astype(U))) if case.center else C

        err = np.abs(product(T).astype(np.longdouble) - G).astype(np.float64)
        assert (err <= bound).all(), name
        if case.dtype == "f64":
            err32 = np.abs(product(np.float32).astype(np.longdouble) - G).astype(np.float64)
            assert (err32 > bound).mean() > 0.5, name


def test_table_names_every_variant():
    seen = set()
    for c in bb.CASES:
        e = c.expect
        seen.add((e["launcher"], c.kind, c.dtype, e.get("tile"), e.get("vec16"), e.get("strip_lt"), e.get("symmetric"),
                  e.get("n128"), e.get("n64")))
    def has(**kw):
        keys = ("launcher", "kind", "dtype", "tile", "vec16", "strip_lt", "symmetric", "n128", "n64")
        return any(all(kw.get(k) is None or kw[k] == v for k, v in zip(keys, s)) for s in seen)
    for dtype in ("f64", "f32"):
        for vec in (0, 1):
            for sb in (32, 64, 128):
                assert has(launcher=bb.L_SYRK, kind="dense", dtype=dtype, tile=sb, vec16=vec), (dtype, vec, sb)
                assert has(launcher=bb.L_SYRK_BATCH, kind="dense", dtype=dtype, tile=sb, vec16=vec) or (dtype == "f32" and vec == 0), (dtype, vec, sb)
            assert has(launcher=bb.L_GRAM, kind="dense", dtype=dtype, vec16=vec, symmetric=1)
            assert has(launcher=bb.L_GRAM, kind="dense", dtype=dtype, vec16=vec, symmetric=0)
            assert has(launcher=bb.L_GRAM_BATCH, kind="dense", dtype=dtype, vec16=vec)
            for mt in (1, 2, 3, 4):
                assert has(launcher=bb.L_STRIP, dtype=dtype, tile=mt, vec16=vec, strip_lt=0), (dtype, vec, mt)
        for sb in (32, 64, 128):
            assert has(launcher=bb.L_SYRK, kind="snp", dtype=dtype, tile=sb)
            assert has(launcher=bb.L_SYRK_BATCH, kind="snp", dtype=dtype, tile=sb) or dtype == "f32"
        assert has(launcher=bb.L_GRAM, kind="snp", dtype=dtype) and has(launcher=bb.L_GRAM_BATCH, kind="snp", dtype=dtype)
        assert has(launcher=bb.L_BLOCK_CSC, kind="csc", dtype=dtype) and has(launcher=bb.L_GRAM_CSC, kind="csc", dtype=dtype)
    for mt in (1, 2, 3, 4):
        assert has(launcher=bb.L_STRIP, dtype="f64", tile=mt, strip_lt=1)
    for n128, n64 in ((0, 1), (1, 0), (1, 1), (2, 0)):   # N = 1 / 64, 65 / 128, 129 / 192, 200
        assert has(launcher=bb.L_GRAM, kind="dense", dtype="f64", n128=n128, n64=n64), (n128, n64)
    assert any(c.expect.get("nsplit") == bb.MANY and c.mode == bb.MODE_STRIP for c in bb.CASES)
    assert any("csc_row_blocks" in c.expect for c in bb.CASES)
    # the strips reach every count of live column quarters and leave rows / columns below row0 alone
    quarters = {(t[3] + t[5] + 63) // 64 for c in bb.CASES if c.mode == bb.MODE_STRIP for t in c.table}
    assert quarters == {1, 2, 3, 4}
    assert any(t[6] > 0 and t[3] > 0 for c in bb.CASES if c.mode == bb.MODE_STRIP for t in c.table)


def test_shape_functions_under_sanitizers(tmp_path):
    """adelie_amd/csrc/gram_shape.hpp (what the launchers and the kernel-level test entry call) as a stand-alone program under
    the address and undefined-behaviour sanitizers, on the CPU."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "gram_shape_main.cpp")
    exe = str(tmp_path / "gram_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "gram_shape: ok" in out.stdout, out.stdout + out.stderr
