"""The multi-response kernels one launch at a time, through adelie_hip_multi_piece_test: the K-wide sweep in each of its variants,
the panel step and its fused form, and the list / expansion / layout launchers, each against an integer reference (bit for bit)
and a longdouble reference (derived bounds).  tests/multi_checks.py has the case tables, the references and the derivation of
every bound; tests/test_multi_checks_host.py shows that these checks fail on subtly wrong kernels."""
import numpy as np
import pytest

import adelie_amd as ad
import multi_checks as mc

pytestmark = pytest.mark.gpu

DTYPES = ("f64", "f32")
LEGS = ("exact", "rounding")
_worst = {}


def _note(mode, dtype, ratios):
    for key, r in ratios.items():
        k = (mode, dtype, key)
        _worst[k] = max(_worst.get(k, 0.0), r)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", [c.name for c in mc.SWEEP_CASES])
def test_sweep(hip, name, leg):
    case = mc.SWEEP_BY_NAME[name]
    a = mc.sweep_inputs(case, leg)
    info = mc.device_call(hip, mc.MODE_SWEEP, case.dtype, a)
    ratios = mc.sweep_check(case, leg, a, info)
    if leg == "rounding":
        print("multi_piece sweep %s %s kernel, %d split(s): worst error / bound = %.3e" % (
            name, mc.VARIANT_NAME[int(info[0])], info[5], ratios["sweep"]))
        _note("sweep-" + mc.VARIANT_NAME[int(info[0])], case.dtype, ratios)
        assert ratios["sweep"] <= 1.0, ratios


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in mc.STEP_CASES])
def test_step_and_fused_step(hip, name, dtype, leg):
    """STEP against the references, then FUSED_STEP on the same inputs (nb_cols <= 128): the same references, and STEP's bits."""
    case = mc.STEP_BY_NAME[name]
    a0 = mc.step_inputs(case, dtype, leg)
    outs = {}
    for fused in (False, True):
        if fused and case.nb_cols > 128:
            continue
        a = mc.with_part(a0, dtype, fused)
        a_in = mc.copy_inputs(a)
        info = mc.device_call(hip, mc.MODE_FUSED if fused else mc.MODE_STEP, dtype, a)
        ratios = mc.step_check(case, dtype, leg, a_in, a, info, fused)
        if leg == "rounding":
            print("multi_piece %s %s %s worst error / bound = %s" % (
                "fused_step" if fused else "step", name, dtype, {k: "%.3e" % v for k, v in sorted(ratios.items())}))
            _note("fused_step" if fused else "step", dtype, ratios)
            assert all(v <= 1.0 for v in ratios.values()), ratios
        outs[fused] = a
    if True in outs:
        mc.fused_equals_step(outs[False], outs[True], dtype)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_axpy_and_batch_pick(hip, dtype, leg):
    for case in mc.AXPY_CASES:
        a = mc.axpy_inputs(case, dtype, leg)
        a_in = mc.copy_inputs(a)
        mc.device_call(hip, mc.MODE_AXPY, dtype, a)
        ratios = mc.axpy_check(case, dtype, leg, a_in, a)
        _note("axpy", dtype, ratios)
        assert all(v <= 1.0 for v in ratios.values()), (case.name, ratios)
    for case in mc.PICK_CASES:
        a = mc.pick_inputs(case, dtype, leg)
        mc.device_call(hip, mc.MODE_PICK, dtype, a)
        ratios = mc.pick_check(dtype, leg, a)
        _note("batch_pick", dtype, ratios)
        assert all(v <= 1.0 for v in ratios.values()), (case.name, ratios)
    if leg == "rounding":
        print("multi_piece axpy / batch_pick %s worst error / bound = %.3e / %.3e" % (
            dtype, _worst.get(("axpy", dtype, "axpy"), 0.0), _worst.get(("batch_pick", dtype, "pick"), 0.0)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lists_expand_and_layout_bit_for_bit(hip, dtype):
    for case in mc.LIST_CASES:
        a = mc.lists_inputs(case)
        mc.device_call(hip, mc.MODE_LISTS, dtype, a)
        mc.lists_check(a)
    for case in mc.EXPAND_CASES:
        a = mc.expand_inputs(case, dtype)
        a_in = mc.copy_inputs(a)
        mc.device_call(hip, mc.MODE_CROSS if case.nc else mc.MODE_EXPAND, dtype, a)
        mc.expand_check(a_in, a)
    for case in mc.MAJOR_CASES:
        for mode in (mc.MODE_TO_MAJOR, mc.MODE_FROM_MAJOR):
            a = mc.major_inputs(case, dtype)
            mc.device_call(hip, mode, dtype, a)
            assert np.array_equal(mc.bits(a["out"]), mc.bits(np.ascontiguousarray(mc.major_reference(a, mode == mc.MODE_TO_MAJOR)))), case.name


def test_entry_refuses_what_it_cannot_run(hip):
    """Bad tables are refused with an error string before anything is launched; the pre-filled outputs stay as they were."""
    dtype = "f64"

    def refused(mode, a, outputs):
        before = {k: a[k].copy() for k in outputs}
        with pytest.raises(RuntimeError):
            mc.device_call(hip, mode, dtype, a)
        for k in outputs:
            assert np.array_equal(a[k].view(np.uint8), before[k].view(np.uint8)), k

    case = mc.STEP_BY_NAME["n1031-K3-dense-nz17-c64-groups-groups-i1"]
    base = mc.with_part(mc.step_inputs(case, dtype, "exact"), dtype, False)
    ncol = (base["pb"] + base["icpt"]) * base["K"]

    def step(**change):
        a = mc.copy_inputs(base)
        for k, v in change.items():
            if isinstance(v, tuple):
                a[k][v[0]] = v[1]
            else:
                a[k] = v
        return a

    outs = ("r", "part")
    for mode in (mc.MODE_STEP, mc.MODE_FUSED):
        refused(mode, step(dcol=(3, ncol)), outs)               # a column index one past the view
        refused(mode, step(dcol=(0, -1)), outs)
        refused(mode, step(cols=(63, ncol)), outs)
        refused(mode, step(nz=18), outs)                        # more changes than dcol / dlt hold
        refused(mode, step(nz=-1), outs)
        refused(mode, step(ld=base["nb"] - 1), outs)            # a leading dimension below nb; X too short for pb columns
        refused(mode, step(pb=base["pb"] + 1), outs)
        refused(mode, step(x_off=65), outs)
        refused(mode, step(K=0), outs)
        refused(mode, step(icpt=2), outs)
        refused(mode, step(part_elems=64 * mc.part_ld(base, dtype, mode == mc.MODE_FUSED) - 1), outs)   # part too small
    big = mc.step_inputs(mc.STEP_BY_NAME["n130-K3-oddld-nz128-c256-straddle-straddle-i1"], dtype, "exact")
    a = mc.with_part(big, dtype, False)
    a["dcol"], a["dlt"], a["n_dcol"], a["nz"] = np.resize(a["dcol"], 129), np.resize(a["dlt"], 129), 129, 129
    refused(mc.MODE_STEP, a, outs)                              # 129 changes
    a = mc.with_part(big, dtype, False)
    a["cols"], a["nb_cols"] = np.resize(a["cols"], 257), 257
    a["part"] = mc.prefill(dtype, 257 * mc.part_ld(a, dtype, False))
    refused(mc.MODE_STEP, a, outs)                              # 257 gradient columns
    a = mc.with_part(big, dtype, True)
    a["part"] = mc.prefill(dtype, 256 * mc.part_ld(a, dtype, True))
    refused(mc.MODE_FUSED, a, outs)                             # 256 gradient columns in the fused step (one block there)
    # the 2-bit base: bytes per column below (nb + 3) / 4, bits too short
    snp = mc.sweep_inputs(mc.SWEEP_BY_NAME["f64-n131-f9-K5-i1-snp"], "exact")
    for change in (dict(ldb=32), dict(pb=snp["pb"] + 1), dict(v_off=65), dict(v_off=-1)):
        a = mc.copy_inputs(snp)
        a.update(change)
        refused(mc.MODE_SWEEP, a, ("out",))
    # the lists and the expansion
    la = mc.lists_inputs(mc.LIST_CASES[1])
    for change in (dict(nv=129), dict(nv=0), dict(K=0)):
        a = mc.copy_inputs(la)
        a.update(change)
        refused(mc.MODE_LISTS, a, ("ulist", "slot", "resp"))
    a = mc.copy_inputs(la)
    a["cols"][2] = -3
    refused(mc.MODE_LISTS, a, ("ulist", "slot", "resp"))
    for case in (mc.EXPAND_CASES[1], mc.EXPAND_CASES[7]):
        ea = mc.expand_inputs(case, dtype)
        mode = mc.MODE_CROSS if case.nc else mc.MODE_EXPAND
        for change in ("slot", "slot_neg", "ldd", "D", "nv"):
            a = mc.copy_inputs(ea)
            if change == "slot":
                a["slot"][0] = a["ldc"]                         # a slot outside C
            elif change == "slot_neg":
                a["slot_c" if case.nc else "slot"][1] = -1
            elif change == "ldd":
                a["ldd"] = a["nv"] - 1
            elif change == "D":
                a["D_elems"] = a["D"].size - a["ldd"]
            else:
                a["nv"] = 129
            refused(mode, a, ("D",))
    pa = mc.pick_inputs(mc.PICK_CASES[1], dtype, "exact")
    a = mc.copy_inputs(pa)
    a["lsel"] = a["K"]
    refused(mc.MODE_PICK, a, ("out",))
    refused(10, mc.copy_inputs(pa), ("out",))                   # an unknown mode


@pytest.mark.parametrize("dtype,n", [("f64", 400), ("f32", 260)])
def test_mul_batch_reaches_the_staged_sweep(hip, dtype, n):
    """mul_batch with more than four vectors and a row count that keeps each of them 16-byte aligned is the public route into the
    staged sweep.  It takes its vectors eight at a time: 8 vectors are one sweep with K = 8, 13 one with K = 8 and one with K = 5
    (three clamped duplicates), 16 two with K = 8.  Exact on integers."""
    T = mc.NP_TYPE[dtype]
    rng = mc._rng("mul_batch %s" % dtype)
    p = 41
    E = rng.randint(-3, 4, size=(n, p)).astype(T)
    X = ad.matrix.dense(np.asfortranarray(E))
    for B in (8, 13, 16):
        for K in {min(B, 8), B % 8 or 8}:
            assert mc.sweep_plan(n, p, K, mc.VEC[dtype], True, True).variant == mc.STAGED
        V = rng.randint(-3, 4, size=(B, n)).astype(T)
        got = X.mul_batch(V)
        ref = V.astype(np.int64) @ E.astype(np.int64)
        assert got.dtype == T and np.array_equal(got, ref.astype(T)), B


def test_worst_ratios_reported():
    """Prints the worst error / bound per mode, dtype and figure seen by this session's cases."""
    for key, r in sorted(_worst.items()):
        print("multi_piece worst %-16s %s %-5s error / bound = %.3e" % (key + (r,)))
    assert all(r <= 1.0 for r in _worst.values())
