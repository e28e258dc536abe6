"""The GLM family kernels one launch at a time, through adelie_hip_glm_piece_test: every launcher of kernels_glm.hip on an exact leg
(integers, bit for bit against an int64 reference), a rounding leg (the kernel's stated formula in mpmath, forward-error bounds
derived per operation) and a decision leg (inputs where a branch decides).  tests/glm_checks.py has the inputs, the references and
the derivation of every bound; tests/test_glm_checks_host.py shows that these checks fail on subtly wrong kernels."""
import numpy as np
import pytest

import glm_checks as gc

pytestmark = pytest.mark.gpu

DTYPES = ("f64", "f32")
SCALAR_MEMBERS = (gc.GAUSSIAN, gc.LOGIT, gc.PROBIT, gc.POISSON)
MEMBERS = SCALAR_MEMBERS + (gc.MULTINOMIAL,)
_worst = {}


def dev(hip):
    return lambda mode, dtype, a: gc.device_call(hip, mode, dtype, a)


def _note(mode, kind, dtype, ratios):
    ratios = {k: v for k, v in ratios.items() if k != "raised"}
    print("glm_piece %-11s %-11s %s worst error / bound = %s" % (
        gc.MODE_NAME[mode], gc.KIND_NAME[kind] if kind is not None else "-", dtype, {k: "%.3e" % v for k, v in sorted(ratios.items())}))
    for key, r in ratios.items():
        k = (gc.MODE_NAME[mode], gc.KIND_NAME[kind] if kind is not None else "-", dtype, key)
        _worst[k] = max(_worst.get(k, 0.0), r)
    assert all(v <= 1.0 for v in ratios.values()), (gc.MODE_NAME[mode], kind, dtype, ratios)


def _legs(hip, mode, dtype, leg, kinds, multi_K=()):
    call = dev(hip)
    if leg == "exact":
        for n in gc.N_LIST:
            gc.run_exact(call, mode, dtype, n)
    elif leg == "rounding":
        for kind in kinds:
            if kind != gc.GAUSSIAN:
                print("eta within +-%g" % gc.RANGES[(kind, dtype)])
            _note(mode, kind, dtype, gc.run_rounding(call, mode, kind, dtype))
    else:
        for kind in kinds:
            for K in (multi_K if kind == gc.MULTINOMIAL else (1,)):
                _note(mode, kind, dtype, gc.run_decision(call, mode, kind, dtype, K))


LEGS3 = ("exact", "rounding", "decision")


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_irls_prepare(hip, dtype, leg):
    _legs(hip, gc.M_PREPARE, dtype, leg, MEMBERS, (1, 2, 3, 7))
    if leg == "decision":     # CALLBACK and COX: hess is read, not recomputed; z comes from irls_resid only for CALLBACK
        _note(gc.M_PREPARE, None, dtype, gc.run_prefilled_kinds(dev(hip), dtype, (gc.M_PREPARE,)))


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_step(hip, dtype, leg):
    _legs(hip, gc.M_NULL, dtype, leg, MEMBERS, (1, 2, 3, 7))
    if leg == "decision":
        _note(gc.M_NULL, None, dtype, gc.run_prefilled_kinds(dev(hip), dtype, (gc.M_NULL,)))


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_irls_finish(hip, dtype, leg):
    if leg == "decision":     # resid stays as it was under CALLBACK and COX; under MULTINOMIAL it is the row-coupled gradient (rounding leg)
        _note(gc.M_FINISH, None, dtype, gc.run_prefilled_kinds(dev(hip), dtype, (gc.M_FINISH,)))
    else:
        _legs(hip, gc.M_FINISH, dtype, leg, MEMBERS)


@pytest.mark.parametrize("leg", ("exact", "rounding"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_irls_weights(hip, dtype, leg):
    _legs(hip, gc.M_WEIGHTS, dtype, leg, (gc.GAUSSIAN,))


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_glm_gradient(hip, dtype, leg):
    _legs(hip, gc.M_GRAD, dtype, leg, MEMBERS, (1, 2, 3, 7))


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_glm_loss(hip, dtype, leg):
    _legs(hip, gc.M_LOSS, dtype, leg, MEMBERS, (1, 2, 3, 7))


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_glm_loss2(hip, dtype, leg):
    _legs(hip, gc.M_LOSS2, dtype, leg, SCALAR_MEMBERS)


@pytest.mark.parametrize("leg", LEGS3)
@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_loss2(hip, dtype, leg):
    if leg == "exact":        # multigaussian, response-major [k nb + i]
        for nb, K in gc.MULTI_SHAPES:
            gc.run_exact(dev(hip), gc.M_MLOSS2, dtype, nb, K)
    else:
        _legs(hip, gc.M_MLOSS2, dtype, leg, (gc.GAUSSIAN, gc.MULTINOMIAL) if leg == "rounding" else (gc.MULTINOMIAL,), (1, 2, 3, 7))


@pytest.mark.parametrize("leg", ("exact", "rounding"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_set_eta_and_dot_diff(hip, dtype, leg):
    for mode in (gc.M_SET_ETA, gc.M_DOT):
        _legs(hip, mode, dtype, leg, (gc.GAUSSIAN,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_overflow_decisions(hip, dtype):
    """Logit at eta = +-800 / +-100, Poisson loss at eta = -inf and hugely negative eta, Poisson with exp(eta) underflowed to zero:
    the expected values written out in the value type, bit for bit."""
    gc.run_overflow_decisions(dev(hip), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rel_change(hip, dtype):
    gc.run_rel_change(dev(hip), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_and_scatter(hip, dtype):
    gc.run_moves(dev(hip), dtype)


def test_entry_refuses_what_it_cannot_run(hip):
    """Bad tables are refused with an error string before anything is launched; the pre-filled outputs stay as they were."""
    dtype = "f64"
    T = np.float64

    def refused(mode, a):
        a = gc.copy_inputs(a)
        a.setdefault("sums", gc.prefill(dtype, 16))
        before = {k: v.copy() for k, v in a.items() if isinstance(v, np.ndarray)}
        with pytest.raises(RuntimeError):
            gc.device_call(hip, mode, dtype, a)
        for k, v in before.items():
            assert np.array_equal(a[k].view(np.uint8), v.view(np.uint8)), k

    def inputs(mode, kind, K=1):
        base = gc.base_arrays(kind, dtype, K)
        NB = base["y"].shape[1]
        Kb = K if (kind == gc.MULTINOMIAL or mode == gc.M_MLOSS2) else 1
        a = gc.call_inputs(mode, kind, dtype, NB * Kb, Kb, base)
        a["K"] = K
        return a

    g = inputs(gc.M_GRAD, gc.LOGIT)
    gc.device_call(hip, gc.M_GRAD, dtype, gc.copy_inputs(g))      # (the table itself is fine)
    refused(gc.M_GRAD, dict(g, n=0))
    refused(gc.M_GRAD, dict(g, n=-5))
    refused(gc.M_GRAD, dict(g, n=(1 << 24) + 1))
    refused(gc.M_GRAD, dict(g, kind=8))
    refused(gc.M_GRAD, dict(g, kind=-1))
    refused(gc.M_GRAD, dict(g, kind=gc.CALLBACK))
    refused(gc.M_GRAD, dict(g, y=None))
    refused(gc.M_GRAD, dict(g, resid=None))
    refused(13, g)
    refused(-1, g)
    m = inputs(gc.M_GRAD, gc.MULTINOMIAL, 3)
    gc.device_call(hip, gc.M_GRAD, dtype, gc.copy_inputs(m))
    refused(gc.M_GRAD, dict(m, K=0))
    refused(gc.M_GRAD, dict(m, K=2))                                # n != nb K
    refused(gc.M_GRAD, dict(m, nb=m["nb"] + 1))
    refused(gc.M_GRAD, dict(m, K=65, nb=1, n=65))
    lo = inputs(gc.M_LOSS, gc.PROBIT)
    refused(gc.M_LOSS, dict(lo, kind=gc.COX))
    refused(gc.M_LOSS, dict(lo, sums=None))
    l2 = inputs(gc.M_LOSS2, gc.POISSON)
    refused(gc.M_LOSS2, dict(l2, kind=gc.MULTINOMIAL))
    refused(gc.M_LOSS2, dict(l2, wb=None))
    ml = inputs(gc.M_MLOSS2, gc.MULTINOMIAL, 2)
    refused(gc.M_MLOSS2, dict(ml, kind=gc.LOGIT))
    refused(gc.M_MLOSS2, dict(ml, b0v=None))
    refused(gc.M_MLOSS2, dict(ml, nb=ml["nb"] - 1))
    for kind in (gc.CALLBACK, gc.COX):
        p = inputs(gc.M_PREPARE, kind)
        gc.device_call(hip, gc.M_PREPARE, dtype, gc.copy_inputs(dict(p, y=None, w=None)))
        refused(gc.M_PREPARE, dict(p, hess=None))
        refused(gc.M_PREPARE, dict(p, irls_resid=None))
        q = inputs(gc.M_NULL, kind)
        refused(gc.M_NULL, dict(q, hess=None))
        if kind == gc.CALLBACK:
            refused(gc.M_NULL, dict(q, cb_z=None))
        else:
            refused(gc.M_NULL, dict(q, resid=None))
    p = inputs(gc.M_PREPARE, gc.LOGIT)
    refused(gc.M_PREPARE, dict(p, w=None))                          # only the pre-filled kinds do without y and w
    wt = inputs(gc.M_WEIGHTS, gc.GAUSSIAN)
    refused(gc.M_WEIGHTS, dict(wt, hess_sum=0.0))
    # GATHER / SCATTER: an index outside the table, a negative one, a repeated one
    table = np.arange(10, dtype=T)
    idx = np.array([0, 9, 3, 4], dtype=np.int32)
    ok = dict(cnt=4, src=table, src_elems=10, idx=idx, dst=gc.prefill(dtype, 4), dst_elems=4)
    gc.device_call(hip, gc.M_GATHER, dtype, gc.copy_inputs(ok))
    for bad in (10, -1):
        refused(gc.M_GATHER, dict(ok, idx=np.array([0, bad, 3, 4], dtype=np.int32)))
    refused(gc.M_GATHER, dict(ok, cnt=-1))
    refused(gc.M_GATHER, dict(ok, src_elems=0))
    sc = dict(cnt=4, src=table[:4].copy(), src_elems=4, idx=idx, dst=gc.prefill(dtype, 10), dst_elems=10)
    gc.device_call(hip, gc.M_SCATTER, dtype, gc.copy_inputs(sc))
    for bad in (10, -1, 3):
        refused(gc.M_SCATTER, dict(sc, idx=np.array([0, bad, 3, 4], dtype=np.int32)))
    refused(gc.M_SCATTER, dict(sc, dst=None))


def test_worst_ratios_reported():
    """Prints the worst error / bound per launcher, kind, dtype and figure seen by this session's cases (A = gc.A_ULP)."""
    print("A = %d ulp per exp / log / erf call (the issue's fallback: no accuracy table found under the ROCm installation)" % gc.A_ULP)
    for key, r in sorted(_worst.items()):
        print("glm_piece worst %-11s %-11s %s %-10s error / bound = %.3e" % (key + (r,)))
    assert all(r <= 1.0 for r in _worst.values())
