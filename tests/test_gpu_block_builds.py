"""The MFMA block builds (kernels_gram.hip, kernels_strip.hip, the csc builds of kernels_sparse.hip) one launch at a time
against numpy, through adelie_hip_block_build_test.  tests/block_build_checks.py has the case table, the two legs and the
derivation of the bound.  Every case asserts: the exact leg bit for bit, the rounding leg within its bound, the pre-fill (a NaN
payload) untouched outside the blocks' footprint, symmetric blocks exactly symmetric, and `info` naming the variant the case is
there for."""
import numpy as np
import pytest
import scipy.sparse as sp

import adelie_amd as ad
import block_build_checks as bb

pytestmark = pytest.mark.gpu

_designs = {}
_worst = {}


def _design(case, leg):
    """The resident design of a case's (kind, type, rows, leg) and its values; made once per session."""
    key = bb.design_key(case) + (leg,)
    if key not in _designs:
        X, raw = bb.make_design_values(case.kind, case.dtype, case.n + case.row_off, leg)
        T = bb.NP_TYPE[case.dtype]
        if case.kind == "dense":
            d = ad.matrix.dense(np.asfortranarray(raw.astype(T)))
        elif case.kind == "snp":
            d = ad.matrix.snp_calldata(raw[0], raw[1], dtype=T)
        else:
            d = ad.matrix.sparse(sp.csc_matrix(raw.astype(T)), resident="csc")
        _designs[key] = (d, X)
    return _designs[key]


def run_build(hip, d, case, w, xm, out0, out1):
    T = bb.NP_TYPE[case.dtype]
    w = np.ascontiguousarray(w, dtype=T)
    xm = np.ascontiguousarray(xm, dtype=T)
    cols = np.ascontiguousarray(case.cols, dtype=np.int32)
    table = np.zeros((len(case.table), 10), dtype=np.int64)
    for y, row in enumerate(case.table):
        table[y, :len(row)] = row
    info = np.full(10, -1, dtype=np.int64)
    rc = hip.fn("block_build_test")(d._handle, case.mode, case.row_off, w.ctypes.data, cols.ctypes.data, len(cols), table.ctypes.data,
                                    len(case.table), xm.ctypes.data, int(case.center), case.ldc, case.strip_plain,
                                    out0.ctypes.data, out0.size, out1.ctypes.data if out1.size else None, out1.size, info.ctypes.data)
    hip.check(rc)
    return info


@pytest.mark.parametrize("leg", ["exact", "rounding"])
@pytest.mark.parametrize("name", [c.name for c in bb.CASES])
def test_block_build(hip, name, leg):
    case = bb.CASE_BY_NAME[name]
    d, X = _design(case, leg)
    X = X[case.row_off:]
    w, xm = bb.make_vectors(case, leg, X)
    if leg == "exact":
        assert bb.exact_headroom(case, X, w, xm) < bb.EXACT_LIMIT[case.dtype]
    want = bb.expected(case, X, w, xm, leg)
    outs = [bb.prefill(case, 0), bb.prefill(case, 1)]
    info = run_build(hip, d, case, w, xm, outs[0], outs[1])
    got_info = bb.check_info(case, info)
    U = bb.BITS[case.dtype]
    T = bb.NP_TYPE[case.dtype]
    ratio = 0.0
    for which, (ref, bound, foot) in enumerate(want):
        got = outs[which]
        untouched = got.view(U)[~foot] == bb.NAN_BITS[case.dtype]
        assert untouched.all(), "%s: %d entries outside the footprint of buffer %d were written" % (name, (~untouched).sum(), which)
        inside = got[foot]
        assert np.isfinite(inside).all(), "%s: %d entries of the footprint of buffer %d were not written" % (
            name, (~np.isfinite(inside)).sum(), which)
        if leg == "exact":
            bad = inside.view(U) != ref[foot].astype(T).view(U)
            assert not bad.any(), "%s: %d of %d entries of buffer %d differ from the exact reference (first at flat index %d)" % (
                name, bad.sum(), bad.size, which, np.flatnonzero(foot)[np.flatnonzero(bad)[0]])
        else:
            err = np.abs(inside.astype(np.longdouble) - ref[foot]).astype(np.float64)
            bnd = bound[foot]
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
            ratio = max(ratio, float(r.max()) if r.size else 0.0)
    for which, idx, midx in bb.mirror_pairs(case):
        assert (outs[which].view(U)[idx] == outs[which].view(U)[midx]).all(), name + ": not exactly symmetric"
    if leg == "rounding":
        key = (got_info["launcher"], case.kind, case.dtype, got_info["vec16"], got_info["strip_lt"])
        _worst[key] = max(_worst.get(key, 0.0), ratio)
        print("block_build %s worst error / bound = %.3e  [%s]" % (name, ratio, bb.variant_of(case)))
        assert ratio <= 1.0, "%s: error / bound = %.3e" % (name, ratio)


def test_entry_refuses_what_it_cannot_run(hip):
    """Bad tables are refused with an error string before anything is launched."""
    case = bb.CASE_BY_NAME["syrk-dense-f64-n1000-M33"]
    d, X = _design(case, "exact")
    w, xm = bb.make_vectors(case, "exact", X)
    out0 = bb.prefill(case, 0)
    for change in (dict(ldc=8), dict(cols=np.array([bb.P_DENSE] * len(case.cols), dtype=np.int32)), dict(out0=40),
                   dict(mode=bb.MODE_STRIP), dict(table=[(5, 129, 0)]), dict(row_off=case.n)):
        bad = case._replace(**change)
        with pytest.raises(RuntimeError):
            run_build(hip, d, bad, w, xm, out0[:bad.out0], bb.prefill(case, 1))
    assert (out0.view(np.uint64) == bb.NAN_BITS["f64"]).all()
    std = ad.matrix.standardize(d, lazy=True)
    with pytest.raises(RuntimeError):
        run_build(hip, std, case, w, xm, out0, bb.prefill(case, 1))


def test_worst_ratios_reported():
    """Prints the worst error / bound per launcher, design kind, type and load variant seen by this session's rounding legs."""
    names = {1: "syrk", 2: "syrk_batch", 3: "gram", 4: "gram_batch", 5: "strip", 6: "csc_block_gram", 7: "gram_csc"}
    for (launcher, kind, dtype, vec, lt), r in sorted(_worst.items()):
        print("block_build worst %-14s %-5s %s vec16=%d strip_lt=%d  error / bound = %.3e" % (names[launcher], kind, dtype, vec, lt, r))
    assert all(r <= 1.0 for r in _worst.values())
