"""The checkers of tests/multi_checks.py against a plain numpy emulation of the multi-response kernels in the target dtype (every
case must pass with every ratio <= 1) and against planted defects (every one must be flagged by at least one case).  This is the
check that tests/test_gpu_multi_pieces.py would fail on a subtly wrong kernel.  No GPU needed."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import multi_checks as mc
from adelie_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("f64", "f32")
LEGS = ("exact", "rounding")


def test_ctypes_struct_matches_c_layout():
    fields = [f[0] for f in _abi.MultiPiece._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"adelie_hip.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(adelie_hip_multi_piece));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(adelie_hip_multi_piece, {f}));\n'
    prog += 'printf("%d\\n", (int)ADELIE_HIP_MULTI_BATCH_PICK);\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_abi.MultiPiece) == 8 * len(fields)
    for f, off in zip(fields, out[1:]):
        assert getattr(_abi.MultiPiece, f).offset == off, f
    assert out[-1] == _abi.MULTI_BATCH_PICK == mc.MODE_PICK
    assert (_abi.MULTI_SWEEP, _abi.MULTI_STEP, _abi.MULTI_FUSED_STEP, _abi.MULTI_BLOCK_LISTS, _abi.MULTI_EXPAND, _abi.MULTI_EXPAND_CROSS,
            _abi.MULTI_AXPY, _abi.MULTI_TO_MAJOR, _abi.MULTI_FROM_MAJOR) == (
        mc.MODE_SWEEP, mc.MODE_STEP, mc.MODE_FUSED, mc.MODE_LISTS, mc.MODE_EXPAND, mc.MODE_CROSS, mc.MODE_AXPY, mc.MODE_TO_MAJOR,
        mc.MODE_FROM_MAJOR)


# ---- every case passes on the emulation -------------------------------------------------------------------------------------------
def run_sweep(case, leg, defect=None):
    a = mc.sweep_inputs(case, leg)
    info = mc.emulate_call(mc.MODE_SWEEP, case.dtype, a, defect)
    return mc.sweep_check(case, leg, a, info)


def run_step(case, dtype, leg, defect=None, fused_too=True):
    """STEP, then FUSED_STEP on the same inputs where it applies; returns the worst ratios."""
    a0 = mc.step_inputs(case, dtype, leg)
    worst, outs = {}, {}
    for fused in (False, True):
        if fused and (case.nb_cols > 128 or not fused_too):
            continue
        a = mc.with_part(a0, dtype, fused)
        a_in = mc.copy_inputs(a)
        info = mc.emulate_call(mc.MODE_FUSED if fused else mc.MODE_STEP, dtype, a, defect)
        for k, v in mc.step_check(case, dtype, leg, a_in, a, info, fused).items():
            worst[k] = max(worst.get(k, 0.0), v)
        outs[fused] = a
    if True in outs:
        mc.fused_equals_step(outs[False], outs[True], dtype)
    return worst


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("dtype,nb", [(dt, nb) for dt in DTYPES for nb in sorted({c.nb for c in mc.SWEEP_CASES if c.dtype == dt})])
def test_sweep_emulation_passes(dtype, nb, leg):
    worst = 0.0
    for case in mc.SWEEP_CASES:
        if (case.dtype, case.nb) == (dtype, nb):
            worst = max(worst, run_sweep(case, leg).get("sweep", 0.0))
    print("sweep %s nb %d %s: worst error / bound of the emulation = %.3e" % (dtype, nb, leg, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in mc.STEP_CASES])
def test_step_emulation_passes(name, dtype, leg):
    worst = run_step(mc.STEP_BY_NAME[name], dtype, leg)
    if leg == "rounding":
        print("step %s %s: worst error / bound of the emulation = %s" % (name, dtype, worst))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES)
def test_other_modes_emulation_passes(dtype):
    for case in mc.AXPY_CASES:
        for leg in LEGS:
            a = mc.axpy_inputs(case, dtype, leg)
            a_in = mc.copy_inputs(a)
            mc.emulate_call(mc.MODE_AXPY, dtype, a)
            assert mc.axpy_check(case, dtype, leg, a_in, a).get("axpy", 0.0) <= 1.0
    for case in mc.LIST_CASES:
        a = mc.lists_inputs(case)
        mc.emulate_call(mc.MODE_LISTS, dtype, a)
        mc.lists_check(a)
    for case in mc.EXPAND_CASES:
        a = mc.expand_inputs(case, dtype)
        a_in = mc.copy_inputs(a)
        mc.emulate_call(mc.MODE_CROSS if case.nc else mc.MODE_EXPAND, dtype, a)
        mc.expand_check(a_in, a)
    for case in mc.MAJOR_CASES:
        for mode in (mc.MODE_TO_MAJOR, mc.MODE_FROM_MAJOR):
            a = mc.major_inputs(case, dtype)
            mc.emulate_call(mode, dtype, a)
            assert np.array_equal(mc.bits(a["out"]), mc.bits(np.ascontiguousarray(mc.major_reference(a, mode == mc.MODE_TO_MAJOR))))
    for case in mc.PICK_CASES:
        for leg in LEGS:
            a = mc.pick_inputs(case, dtype, leg)
            mc.emulate_call(mc.MODE_PICK, dtype, a)
            assert mc.pick_check(dtype, leg, a).get("pick", 0.0) <= 1.0


def test_lists_reference_by_hand():
    u, s, r = mc.lists_reference(np.array([6, 7, 3, 8, 4, 30], np.int32), 3)
    assert u.tolist() == [2, 1, 10] and s.tolist() == [0, 0, 1, 0, 1, 2] and r.tolist() == [0, 1, 0, 2, 1, 0]
    feat, slot = mc.build_slots(np.array([6, 7, 3, 8, 4, 30], np.int32), 3)
    assert feat == [2, 1, 2, 1, 10] and slot == [0, 0, 1, 2, 3, 4]    # non-consecutive entries of a feature get slots of their own


# ---- every planted defect is flagged ----------------------------------------------------------------------------------------------
def flagged(run):
    try:
        ratios = run()
    except AssertionError:
        return True
    return any(not (v <= 1.0) for v in ratios.values())


SWEEP_DEFECTS = {
    # defect -> the cases that can see it
    "tile_parity": lambda c: c.variant == mc.STAGED and c.nb >= 64 * mc.VEC[c.dtype],
    # (the staged kernel's tail starts behind its last whole tile, the others' behind their last whole vector)
    "drop_tail": lambda c: (c.nb % (64 * mc.VEC[c.dtype]) != 0 if c.variant == mc.STAGED
                            else c.base in ("dense", "snp") and c.nb % mc.VEC[c.dtype] != 0),
    "store_dup": lambda c: c.K % mc.kt_of(c.K) != 0 and c.pb + c.icpt > 1,
    "l0_ignored": lambda c: c.K > 8,
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", sorted(SWEEP_DEFECTS))
def test_sweep_defect_is_flagged(defect, dtype):
    cases = [c for c in mc.SWEEP_CASES if c.dtype == dtype and SWEEP_DEFECTS[defect](c)]
    assert cases
    hits = {leg: [c.name for c in cases if flagged(lambda: run_sweep(c, leg, defect))] for leg in LEGS}
    print("%s %s: flagged by %d (exact) / %d (rounding) of %d cases" % (defect, dtype, len(hits["exact"]), len(hits["rounding"]), len(cases)))
    assert hits["exact"] and hits["rounding"]
    if defect != "store_dup":                      # (a duplicate that lands past the last slot read is not seen: not every case can)
        assert len(hits["exact"]) == len(cases)
    # the same cases pass without the defect
    assert not any(flagged(lambda: run_sweep(c, "exact")) for c in cases[:8])


def test_staged_variants_catch_parity_only_with_the_staged_kernel():
    """A four-wave case does not stage and must not be touched by the staged kernel's defect: the checks are specific."""
    case = next(c for c in mc.SWEEP_CASES if c.variant == mc.FOURWAVE and c.nb >= 256)
    assert not flagged(lambda: run_sweep(case, "exact", "tile_parity"))


STEP_DEFECTS = {
    "head_prev": (lambda c: max(c.nz, c.nb_cols) > 64 and c.dkind != "straddle", LEGS),
    "pad_unmasked": (lambda c: True, ("rounding",)),
    "part_unlisted": (lambda c: c.ckind in ("resp02", "twice") or c.nb_cols % c.K != 0, LEGS),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", sorted(STEP_DEFECTS))
def test_step_defect_is_flagged(defect, dtype):
    pick, legs = STEP_DEFECTS[defect]
    cases = [c for c in mc.STEP_CASES if pick(c)]
    assert cases
    for leg in legs:
        hits = [c.name for c in cases if flagged(lambda: run_step(c, dtype, leg, defect, fused_too=False))]
        print("%s %s %s: flagged by %d of %d cases" % (defect, dtype, leg, len(hits), len(cases)))
        assert hits


def test_head_defect_needs_a_boundary_at_64():
    """A list whose 64th and 65th entries share a feature is where a head test that reads list[m - 1] across the boundary differs
    from one that does not: with the entry joined to the previous slot the straddling lists come out right, the others wrong."""
    straddle = next(c for c in mc.STEP_CASES if c.dkind == "straddle" and c.K == 3 and c.nb_cols == 128)
    assert not flagged(lambda: run_step(straddle, "f64", "exact", "head_prev", fused_too=False))
    aligned = next(c for c in mc.STEP_CASES if c.dkind == "groups" and c.nz == 128 and 64 % c.K == 0)
    assert flagged(lambda: run_step(aligned, "f64", "exact", "head_prev", fused_too=False))


@pytest.mark.parametrize("dtype", DTYPES)
def test_expand_defect_is_flagged(dtype):
    hits = []
    for case in mc.EXPAND_CASES:
        if case.nc:
            continue
        a = mc.expand_inputs(case, dtype)
        a_in = mc.copy_inputs(a)
        mc.emulate_call(mc.MODE_EXPAND, dtype, a, "expand_zero")
        if flagged(lambda: mc.expand_check(a_in, a) or {}):
            hits.append(case.name)
    assert set(hits) == {c.name for c in mc.EXPAND_CASES if not c.nc and max(c.lsels) > 0}, hits


def test_every_defect_has_a_test():
    assert set(mc.DEFECTS) == set(SWEEP_DEFECTS) | set(STEP_DEFECTS) | {"expand_zero"}


# ---- the case tables reach what they are meant to reach ------------------------------------------------------------------------------
def test_case_tables_cover_the_dispatch():
    seen = {(c.dtype, c.variant, mc.kt_of(c.K)) for c in mc.SWEEP_CASES}
    for dtype in DTYPES:
        for kt in (2, 4):
            assert (dtype, mc.PLAIN, kt) in seen
        assert (dtype, mc.FOURWAVE, 8) in seen and (dtype, mc.STAGED, 8) in seen
    for dtype in DTYPES:
        cs = [c for c in mc.SWEEP_CASES if c.dtype == dtype]
        plans = {c.name: mc.sweep_plan(c.nb, c.pb + c.icpt, c.K, mc.VEC[dtype], c.base not in ("oddld", "xoff"),
                                       c.nb % mc.VEC[dtype] == 0 and c.v_off == 0) for c in cs}
        for variant in (mc.PLAIN, mc.FOURWAVE, mc.STAGED):                 # both split counts, in every variant
            assert {plans[c.name].nsplit for c in cs if c.variant == variant} == {1, 2}, (dtype, variant)
        for variant in (mc.PLAIN, mc.FOURWAVE):                          # vector and scalar loads, both reasons for the latter
            assert {plans[c.name].vec for c in cs if c.variant == variant} == {1, mc.VEC[dtype]}
            assert {c.base for c in cs if c.variant == variant} >= {"dense", "oddld", "xoff", "snp"}
        staged = [c for c in cs if c.variant == mc.STAGED]
        TR = 64 * mc.VEC[dtype]
        assert any(c.nb < TR for c in staged) and any(c.nb % TR == 0 for c in staged) and any(c.nb % TR and c.nb > TR for c in staged)
        assert {(c.K + 7) // 8 for c in staged} == {1, 2} and any(c.base == "snp" for c in staged)
        assert {c.v_off for c in cs if c.variant == mc.FOURWAVE} == {0, 1}
        assert {c.K for c in cs} == set(mc.SWEEP_K) and {c.pb + c.icpt for c in cs} >= set(mc.SWEEP_NFEAT)
        assert {c.icpt for c in cs} == {0, 1} and {c.nb for c in cs} >= set(mc.SWEEP_NB[dtype])
        assert any(c.base == "snp" and c.nb % 4 for c in cs)
    assert {c.base for c in mc.STEP_CASES} == {"dense", "oddld", "xoff", "snp"}
    for base in ("dense", "oddld", "snp"):
        assert {c.nb for c in mc.STEP_CASES if c.base == base} >= {40, "T", "T+1", 1031}
    assert {c.nz for c in mc.STEP_CASES} >= {0, 1, 8, 9, 17, 128} and any(c.nz_dev > 128 for c in mc.STEP_CASES)
    assert {c.nb_cols for c in mc.STEP_CASES} >= {1, 64, 65, 128, 256}
    assert {mc.kt_of(c.K) for c in mc.STEP_CASES} == {2, 4, 8} and any(c.K > 8 for c in mc.STEP_CASES)
    assert {c.dkind for c in mc.STEP_CASES} >= {"groups", "straddle", "resp02", "twice"} and {c.icpt for c in mc.STEP_CASES} == {0, 1}
    # the fused step: an nb whose last 16-wave workgroup is partly empty, and one that fills whole workgroups' worth of slices
    assert any(c.nb == 1031 and c.nb_cols <= 128 for c in mc.STEP_CASES)
