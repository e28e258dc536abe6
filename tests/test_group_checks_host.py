"""The checkers of tests/group_checks.py against a plain numpy emulation of the group engine's pieces in the target dtype (every
case must pass with every ratio <= 1) and against planted defects (every one must be flagged).  This is the check that
tests/test_gpu_group_pieces.py would fail on a subtly wrong kernel.  No GPU needed."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import group_checks as gc
from adelie_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("f64", "f32")
_eig_done = {}
_margin_cache = {}


def test_ctypes_struct_matches_c_layout():
    fields = [f[0] for f in _abi.GroupPiece._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"adelie_hip.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(adelie_hip_group_piece));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(adelie_hip_group_piece, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_abi.GroupPiece)
    for f, off in zip(fields, out[1:]):
        assert getattr(_abi.GroupPiece, f).offset == off, f
    assert _abi.GDESC == {k: v for k, v in gc.GD.items()}


def _eig_run(case, dtype, defect=None):
    key = (case.name, dtype, defect)
    if key not in _eig_done:
        inp, blocks, desc = gc.eig_inputs(case, dtype)
        gc.emulate_call(gc.MODE_EIG, dtype, inp, defect)
        _eig_done[key] = (inp, blocks, desc)
    return _eig_done[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in gc.EIG_CASES])
def test_eig_emulation_passes(oracle, name, dtype):
    case = next(c for c in gc.EIG_CASES if c.name == name)
    inp, blocks, desc = _eig_run(case, dtype)
    ratios, same = gc.eig_check(case, dtype, inp, blocks, desc, oracle)
    print("eig %s %s: %s  bitwise equal to the CPU Jacobi: %s" % (name, dtype, ratios, same))
    assert ratios and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
def test_eig_flags_perturbed_eigenvector(oracle, dtype):
    case = next(c for c in gc.EIG_CASES if c.name == "gram-q16")
    inp, blocks, desc = _eig_run(case, dtype, "eigvec-1e-9")
    if dtype == "f32":  # a float32 eigenbasis cannot show 1e-9: the output rounding term of the bound is 1.25e-7
        ratios, _ = gc.eig_check(case, dtype, inp, blocks, desc, oracle)
        assert max(ratios.values()) <= 1.0
        return
    ratios, _ = gc.eig_check(case, dtype, inp, blocks, desc, oracle)
    assert ratios[("defect", "q2-16")] > 1.0, ratios


def test_eig_footprint_is_checked(oracle):
    case = next(c for c in gc.EIG_CASES if c.name == "mixed-1-5-96")
    inp, blocks, desc = gc.eig_inputs(case, "f64")
    gc.emulate_call(gc.MODE_EIG, "f64", inp)
    inp["V"][desc[0][2]] = 1.0  # the eigenbasis slot of the group of one value
    with pytest.raises(AssertionError, match="footprint"):
        gc.eig_check(case, "f64", inp, blocks, desc, oracle)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("leg", ["exact", "rounding"])
@pytest.mark.parametrize("name", [c.name for c in gc.ROT_CASES])
def test_rotate_emulation_passes(name, leg, dtype):
    case = next(c for c in gc.ROT_CASES if c.name == name)
    a, Dfull, R, nval = gc.rot_inputs(case, dtype, leg)
    gc.emulate_call(gc.MODE_ROTATE, dtype, a)
    ratios = gc.rot_check(case, dtype, leg, a, Dfull, R, nval)
    if leg == "rounding":
        assert ratios and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["narrow-mixed-inplace", "narrow-mixed-dsrc", "wide-17-dsrc", "wide-64-inplace", "wide-128-dsrc"])
def test_rotate_flags_defects(name, dtype):
    case = next(c for c in gc.ROT_CASES if c.name == name)
    # V transposed: the exact leg sees it bit for bit, the rounding leg leaves its bound
    a, Dfull, R, nval = gc.rot_inputs(case, dtype, "exact")
    gc.emulate_call(gc.MODE_ROTATE, dtype, a, "v-transposed")
    with pytest.raises(AssertionError, match="exact"):
        gc.rot_check(case, dtype, "exact", a, Dfull, R, nval)
    a, Dfull, R, nval = gc.rot_inputs(case, dtype, "rounding")
    gc.emulate_call(gc.MODE_ROTATE, dtype, a, "v-transposed")
    assert max(gc.rot_check(case, dtype, "rounding", a, Dfull, R, nval).values()) > 1.0
    # an entry written outside the footprint
    if nval < gc.G:
        a, Dfull, R, nval = gc.rot_inputs(case, dtype, "rounding")
        gc.emulate_call(gc.MODE_ROTATE, dtype, a, "outside-footprint")
        with pytest.raises(AssertionError, match="outside"):
            gc.rot_check(case, dtype, "rounding", a, Dfull, R, nval)


@pytest.mark.parametrize("name", [c.name for c in gc.LAY_CASES])
def test_layout_reference_is_consistent(name):
    case = next(c for c in gc.LAY_CASES if c.name == name)
    a, _ = gc.layout_tables(case.blocks, case.perm, gc._rng("lay " + name))
    a["desc"] = np.full(a["nblk"] * gc.GD["STRIDE"], -1, np.int32)
    gc.emulate_call(gc.MODE_LAYOUT, "f64", a)
    gc.layout_check(name, a, a["desc"])
    d = a["desc"].reshape(a["nblk"], -1)
    for j, blk in enumerate(case.blocks):
        assert d[j, gc.GD["NG"]] == len(blk) and d[j, gc.GD["NVAL"]] == sum(blk)
        vmap = d[j, :sum(blk)]
        assert len(set(vmap)) == len(vmap) and vmap.max() < a["nv"]
    a["desc"][gc.GD["VPOS"] + 1] += 1
    with pytest.raises(AssertionError, match="descriptor"):
        gc.layout_check(name, a, a["desc"])


def _solve_run(case, dtype, defect=None):
    a, aux = gc.solve_inputs(case, dtype)
    if case.kind == "chained":
        gc.chain_eig_rotate(gc.emulate_call, dtype, a, aux)
    a_in = gc.copy_inputs(a)
    gc.emulate_call(case.mode, dtype, a, defect)
    return a_in, aux, a


SOLVE_RUNS = [(c.name, dt) for c in gc.SOLVE_CASES for dt in DTYPES if not (c.kind == "chained" and dt == "f32")]


@pytest.mark.parametrize("name,dtype", SOLVE_RUNS)
def test_solve_emulation_passes(name, dtype):
    case = gc.SOLVE_BY_NAME[name]
    a_in, aux, a = _solve_run(case, dtype)
    ratios = gc.solve_check(case, dtype, a_in, aux, a)
    print("solve %s %s: %s" % (name, dtype, {k: "%.2e" % v for k, v in ratios.items()}))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    if case.kind is None:
        assert ("rsq", "state") in ratios and ("cm", "state") in ratios


CLEAR_RUNS = [r for r in SOLVE_RUNS if gc.SOLVE_BY_NAME[r[0]].kind in (None, "chained")]


def _margins(name, dtype):
    """(screen group, q, | ||u|| - l1p | / l1p, min(Lambda) + l2p, 'zero' / 'root') per visited group of the emulated call."""
    if (name, dtype) not in _margin_cache:
        case = gc.SOLVE_BY_NAME[name]
        a_in, aux, a = _solve_run(case, dtype)
        _margin_cache[name, dtype] = [
            m + ("zero" if not a["beta"][a["sbegin"][m[0]]:a["sbegin"][m[0]] + m[1]].any() else "root",)
            for m in gc.threshold_margins(case, dtype, a_in, aux, a)]
    return _margin_cache[name, dtype]


@pytest.mark.parametrize("name,dtype", CLEAR_RUNS)
def test_solve_inputs_keep_clear_of_the_threshold(name, dtype):
    """No group within 1e-6 relative of ||u|| = l1 pen, and min(Lambda) + l2 pen > 0 for every group."""
    margins = _margins(name, dtype)
    assert len(margins) == sum(len(b) for b in gc.SOLVE_BY_NAME[name].blocks)
    assert min(m[2] for m in margins) > 1e-6, sorted(margins, key=lambda m: m[2])[:3]
    assert min(m[3] for m in margins) > 0


def test_solve_table_covers_both_sides_of_the_threshold():
    """Every width class has groups that end at zero and groups that end at a root, in both dtypes (PANEL_SOLVE: all four
    classes; GRAM_PASS: widths up to 16)."""
    sides = set()
    for name, dtype in CLEAR_RUNS:
        for m in _margins(name, dtype):
            sides.add((gc.SOLVE_BY_NAME[name].mode, dtype, gc.width_class(m[1]), m[4]))
    for dtype in DTYPES:
        for side in ("zero", "root"):
            for cls in ("q1", "q2-16", "q17-64", "q65-128"):
                assert (gc.MODE_PANEL, dtype, cls, side) in sides, (dtype, cls, side)
            for cls in ("q1", "q2-16"):
                assert (gc.MODE_GRAM, dtype, cls, side) in sides, (dtype, cls, side)


# defect -> the ratio key or the assertion message that must flag it, and the cases it is planted in
SOLVE_DEFECTS = {
    "no-l2": ("visit", ["panel-all-widths", "panel-128", "gram-narrow"]),
    "grad-skip": ("visit", ["panel-all-widths", "gram-narrow"]),
    "loose-root": ("visit", ["panel-all-widths", "panel-128", "gram-narrow"]),
    "rsq-skip": ("rsq", ["panel-all-widths", "gram-narrow"]),
    "dlt-ulp": ("dlt is not", ["panel-all-widths", "panel-64-64"]),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", sorted(SOLVE_DEFECTS))
def test_solve_flags_defects(defect, dtype):
    what, names = SOLVE_DEFECTS[defect]
    for name in names:
        case = gc.SOLVE_BY_NAME[name]
        a_in, aux, a = _solve_run(case, dtype, defect)
        if what.startswith("dlt"):
            with pytest.raises(AssertionError, match=what):
                gc.solve_check(case, dtype, a_in, aux, a)
            continue
        ratios = gc.solve_check(case, dtype, a_in, aux, a)
        worst = max(r for k, r in ratios.items() if k[0] == what)
        print("defect %s in %s %s: worst %s ratio %.3e" % (defect, name, dtype, what, worst))
        assert worst > 1.0, (defect, name, ratios)
