"""The checks of tests/glm_checks.py against a plain numpy model of the GLM family kernels in the value type (every case must pass
with every ratio <= 1: this is also where the conditions that only concern the references are verified) and against planted
defects (every one must be flagged by a named case).  This is the check that tests/test_gpu_glm_pieces.py would fail on a subtly
wrong kernel.  No GPU needed."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import glm_checks as gc
from adelie_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("f64", "f32")
MEMBERS = (gc.GAUSSIAN, gc.LOGIT, gc.PROBIT, gc.POISSON, gc.MULTINOMIAL)
KIND_MODES = (gc.M_PREPARE, gc.M_FINISH, gc.M_NULL, gc.M_GRAD, gc.M_LOSS, gc.M_LOSS2)
EXACT_MODES = (gc.M_PREPARE, gc.M_WEIGHTS, gc.M_FINISH, gc.M_NULL, gc.M_GRAD, gc.M_LOSS, gc.M_LOSS2, gc.M_SET_ETA, gc.M_DOT)


def model(defect=None):
    return lambda mode, dtype, a: gc.emulate_call(mode, dtype, a, defect)


def test_ctypes_struct_matches_c_layout():
    fields = [f[0] for f in _abi.GlmPiece._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"adelie_hip.h\"\nint main(){\n"
    prog += 'printf("%zu\\n", sizeof(adelie_hip_glm_piece));\n'
    for f in fields:
        prog += f'printf("%zu\\n", offsetof(adelie_hip_glm_piece, {f}));\n'
    prog += 'printf("%d\\n", (int)ADELIE_HIP_GLM_PIECE_SCATTER);\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = [int(x) for x in subprocess.check_output([exe]).split()]
    assert out[0] == ctypes.sizeof(_abi.GlmPiece) == 8 * len(fields)
    for f, off in zip(fields, out[1:]):
        assert getattr(_abi.GlmPiece, f).offset == off, f
    assert out[-1] == _abi.GLM_PIECE_SCATTER == gc.M_SCATTER
    assert (_abi.GLM_PIECE_PREPARE, _abi.GLM_PIECE_WEIGHTS, _abi.GLM_PIECE_FINISH, _abi.GLM_PIECE_NULL_STEP, _abi.GLM_PIECE_GRADIENT,
            _abi.GLM_PIECE_LOSS, _abi.GLM_PIECE_LOSS2, _abi.GLM_PIECE_MULTI_LOSS2, _abi.GLM_PIECE_SET_ETA, _abi.GLM_PIECE_DOT_DIFF,
            _abi.GLM_PIECE_REL_CHANGE, _abi.GLM_PIECE_GATHER) == tuple(range(12))
    assert (_abi.GLM_GAUSSIAN, _abi.GLM_BINOMIAL_LOGIT, _abi.GLM_GAUSSIAN_IRLS, _abi.GLM_MULTINOMIAL, _abi.GLM_POISSON,
            _abi.GLM_BINOMIAL_PROBIT, _abi.GLM_CALLBACK, _abi.GLM_COX) == (
        gc.GAUSSIAN, gc.LOGIT, gc.GAUSSIAN_IRLS, gc.MULTINOMIAL, gc.POISSON, gc.PROBIT, gc.CALLBACK, gc.COX)


def test_the_reduction_grid_and_the_build_flags_are_the_ones_assumed():
    src = open(os.path.join(ROOT, "adelie_amd", "csrc", "kernels_glm.hip")).read()
    assert re.search(r"constexpr int RB = 256;", src) and re.search(r"constexpr int RT = 256;", src)
    flags = open(os.path.join(ROOT, "adelie_amd", "csrc", "build.sh")).read() + open(os.path.join(ROOT, "adelie_amd", "csrc", "build.mk")).read()
    assert "fast-math" not in flags and "-Ofast" not in flags and "unsafe-fp" not in flags
    assert gc.reduction_depth(65536) == 21 and gc.reduction_depth(65537) == 22 and gc.reduction_depth(131149) == 23


def test_probit_saturation_thresholds():
    """At the decision leg's |eta| the distance of erf to 1 is below 2^-20 ulp; at the rounding leg's it is far above an ulp."""
    for dtype in DTYPES:
        u = gc.UNIT[dtype]
        assert gc.ctx.erfc(gc.M(gc.PROBIT_SAT[dtype]) / gc.ctx.sqrt(2)) < 2.0 ** -20 * u
        assert gc.ctx.erfc(gc.M(gc.RANGES[(gc.PROBIT, dtype)]) / gc.ctx.sqrt(2)) > 2.0 ** 10 * u
        T = gc.NP_TYPE[dtype]
        assert gc.np_cdf(T, np.array([gc.PROBIT_SAT[dtype], -gc.PROBIT_SAT[dtype]], dtype=T)).tolist() == [1.0, 0.0]


# ---- every case passes on the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_leg_passes_on_the_model(dtype):
    for mode in EXACT_MODES:
        for n in gc.N_LIST:
            gc.run_exact(model(), mode, dtype, n)
    for nb, K in gc.MULTI_SHAPES:
        gc.run_exact(model(), gc.M_MLOSS2, dtype, nb, K)
    gc.run_moves(model(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", MEMBERS)
def test_rounding_leg_passes_on_the_model(kind, dtype):
    print("eta within +-%g" % gc.RANGES[(kind, dtype)])
    for mode in KIND_MODES + ((gc.M_MLOSS2,) if kind in (gc.GAUSSIAN, gc.MULTINOMIAL) else ()):
        if mode == gc.M_LOSS2 and kind == gc.MULTINOMIAL:
            continue
        ratios = gc.run_rounding(model(), mode, kind, dtype)
        print("model %-11s %-11s %s worst error / bound = %s" % (gc.MODE_NAME[mode], gc.KIND_NAME[kind], dtype,
                                                                {k: "%.3e" % v for k, v in sorted(ratios.items())}))
        assert all(v <= 1.0 for v in ratios.values()), (gc.MODE_NAME[mode], ratios)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kindless_launchers_pass_on_the_model(dtype):
    for mode in (gc.M_WEIGHTS, gc.M_SET_ETA, gc.M_DOT):
        ratios = gc.run_rounding(model(), mode, gc.GAUSSIAN, dtype)
        print("model %-11s %s worst error / bound = %s" % (gc.MODE_NAME[mode], dtype, {k: "%.3e" % v for k, v in sorted(ratios.items())}))
        assert all(v <= 1.0 for v in ratios.values()), (gc.MODE_NAME[mode], ratios)
    gc.run_rel_change(model(), dtype)


DECISIONS = [(mode, kind, K) for kind in (gc.GAUSSIAN, gc.LOGIT, gc.PROBIT, gc.POISSON) for mode in (gc.M_GRAD, gc.M_PREPARE, gc.M_NULL, gc.M_LOSS, gc.M_LOSS2)
             for K in (1,)] + [(mode, gc.MULTINOMIAL, K) for K in (1, 2, 3, 7) for mode in (gc.M_GRAD, gc.M_PREPARE, gc.M_NULL, gc.M_LOSS, gc.M_MLOSS2)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_decision_leg_passes_on_the_model(dtype):
    fired = 0
    for mode, kind, K in DECISIONS:
        ratios = gc.run_decision(model(), mode, kind, dtype, K)
        fired += ratios.pop("raised", 0)
        assert all(v <= 1.0 for v in ratios.values()), (gc.MODE_NAME[mode], gc.KIND_NAME[kind], K, ratios)
    assert fired > 40                                             # the raise decided in every family
    ratios = gc.run_prefilled_kinds(model(), dtype)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    gc.run_overflow_decisions(model(), dtype)


# ---- every planted defect is flagged by a named case -------------------------------------------------------------------------------------
def flagged(run):
    try:
        ratios = run()
    except AssertionError:
        return True
    return any(not (v <= 1.0) for k, v in (ratios or {}).items() if k != "raised")


CATCHERS = {
    "drop_tail": [lambda c, dt: gc.run_exact(c, gc.M_LOSS, dt, 257), lambda c, dt: gc.run_exact(c, gc.M_GRAD, dt, 65),
                  lambda c, dt: gc.run_exact(c, gc.M_NULL, dt, 65537), lambda c, dt: gc.run_exact(c, gc.M_MLOSS2, dt, 63, 2),
                  lambda c, dt: gc.run_rounding(c, gc.M_LOSS, gc.LOGIT, dt, ((63, 1),)), lambda c, dt: gc.run_rel_change(c, dt)],
    "skip_trip2": [lambda c, dt: gc.run_exact(c, gc.M_LOSS, dt, 65537), lambda c, dt: gc.run_exact(c, gc.M_FINISH, dt, 131149),
                   lambda c, dt: gc.run_exact(c, gc.M_MLOSS2, dt, 65537, 3),
                   lambda c, dt: gc.run_rounding(c, gc.M_LOSS2, gc.PROBIT, dt, ((131149, 1),)), lambda c, dt: gc.run_rel_change(c, dt)],
    "swap_acc": [lambda c, dt: gc.run_exact(c, gc.M_WEIGHTS, dt, 257), lambda c, dt: gc.run_rounding(c, gc.M_WEIGHTS, gc.GAUSSIAN, dt, ((1, 1),))],
    "h0_lt": [lambda c, dt: gc.run_decision(c, gc.M_PREPARE, gc.LOGIT, dt), lambda c, dt: gc.run_decision(c, gc.M_NULL, gc.POISSON, dt),
              lambda c, dt: gc.run_prefilled_kinds(c, dt), lambda c, dt: gc.run_overflow_decisions(c, dt)],
    "raise_after_div": [lambda c, dt: gc.run_decision(c, gc.M_PREPARE, gc.POISSON, dt), lambda c, dt: gc.run_decision(c, gc.M_NULL, gc.LOGIT, dt),
                        lambda c, dt: gc.run_prefilled_kinds(c, dt)],
    "no_w_guard": [lambda c, dt: gc.run_decision(c, gc.M_PREPARE, gc.LOGIT, dt), lambda c, dt: gc.run_decision(c, gc.M_PREPARE, gc.MULTINOMIAL, dt, 3),
                   lambda c, dt: gc.run_decision(c, gc.M_NULL, gc.MULTINOMIAL, dt, 2)],
    "no_probit_clamp": [lambda c, dt: gc.run_decision(c, gc.M_GRAD, gc.PROBIT, dt), lambda c, dt: gc.run_decision(c, gc.M_LOSS, gc.PROBIT, dt),
                        lambda c, dt: gc.run_decision(c, gc.M_PREPARE, gc.PROBIT, dt), lambda c, dt: gc.run_decision(c, gc.M_LOSS2, gc.PROBIT, dt)],
    "no_shift": [lambda c, dt: gc.run_decision(c, gc.M_GRAD, gc.MULTINOMIAL, dt, 3), lambda c, dt: gc.run_decision(c, gc.M_LOSS, gc.MULTINOMIAL, dt, 2),
                 lambda c, dt: gc.run_decision(c, gc.M_MLOSS2, gc.MULTINOMIAL, dt, 7)],
    "rel_no_reset": [lambda c, dt: gc.run_rel_change(c, dt)],
    "rel_nan_zero": [lambda c, dt: gc.run_rel_change(c, dt)],
    "row_major": [lambda c, dt: gc.run_exact(c, gc.M_MLOSS2, dt, 257, 2), lambda c, dt: gc.run_exact(c, gc.M_MLOSS2, dt, 65, 7),
                  lambda c, dt: gc.run_rounding(c, gc.M_GRAD, gc.MULTINOMIAL, dt, ((63, 2),)),
                  lambda c, dt: gc.run_rounding(c, gc.M_LOSS, gc.MULTINOMIAL, dt, ((64, 3),))],
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", gc.DEFECTS)
def test_defect_is_flagged(defect, dtype):
    for q, run in enumerate(CATCHERS[defect]):
        assert not flagged(lambda: run(model(), dtype)), "catcher %d of %s fails without the defect" % (q, defect)
        assert flagged(lambda: run(model(defect), dtype)), "catcher %d does not see %s" % (q, defect)


def test_every_defect_has_a_catcher():
    assert set(CATCHERS) == set(gc.DEFECTS)


def test_checks_are_specific():
    """A defect of one kernel does not touch the cases of another: a one-trip case passes with the second trip skipped, a case with
    no NaN with NaN read as zero."""
    assert not flagged(lambda: gc.run_exact(model("skip_trip2"), gc.M_LOSS, "f64", 65536))
    assert not flagged(lambda: gc.run_exact(model("swap_acc"), gc.M_NULL, "f32", 257))
    assert not flagged(lambda: gc.run_decision(model("no_probit_clamp"), gc.M_GRAD, gc.LOGIT, "f64"))
