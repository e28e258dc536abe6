"""The device pieces of the group engine one launch at a time, through adelie_hip_group_piece_test: the eigenbasis kernel, the
block rotation, the layout descriptors and the two forms of the group visits, each against a longdouble reference.
tests/group_checks.py has the case tables, the references and the derivation of every bound;
tests/test_group_checks_host.py shows that these checks fail on subtly wrong kernels."""
import numpy as np
import pytest

import group_checks as gc

pytestmark = pytest.mark.gpu

DTYPES = ("f64", "f32")
_worst = {}


def _note(mode, dtype, ratios):
    for key, r in ratios.items():
        k = (mode, dtype) + (key if isinstance(key, tuple) else ("entry", key))
        _worst[k] = max(_worst.get(k, 0.0), r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in gc.EIG_CASES])
def test_eig(hip, oracle, name, dtype):
    case = next(c for c in gc.EIG_CASES if c.name == name)
    inp, blocks, desc = gc.eig_inputs(case, dtype)
    gc.device_call(hip, gc.MODE_EIG, dtype, inp)
    ratios, same = gc.eig_check(case, dtype, inp, blocks, desc, oracle)
    print("group_piece eig %s %s worst figure / bound = %.3e%s" % (
        name, dtype, max(ratios.values()), "" if dtype == "f32" else "  bit for bit the CPU Jacobi: %s" % same))
    _note("eig", dtype, ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("leg", ["exact", "rounding"])
@pytest.mark.parametrize("name", [c.name for c in gc.ROT_CASES])
def test_rotate(hip, name, leg, dtype):
    case = next(c for c in gc.ROT_CASES if c.name == name)
    a, Dfull, R, nval = gc.rot_inputs(case, dtype, leg)
    info = gc.device_call(hip, gc.MODE_ROTATE, dtype, a)
    assert info[1] == (1 if max(case.sizes) > gc.ROT_QM else 0)
    ratios = gc.rot_check(case, dtype, leg, a, Dfull, R, nval)
    if leg == "rounding":
        print("group_piece rotate %s %s worst error / bound = %.3e" % (name, dtype, max(ratios.values())))
        _note("rotate", dtype, ratios)
        assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c.name for c in gc.LAY_CASES])
def test_layout(hip, name, dtype):
    case = next(c for c in gc.LAY_CASES if c.name == name)
    a, _ = gc.layout_tables(case.blocks, case.perm, gc._rng("lay " + name))
    a["desc"] = np.full(a["nblk"] * gc.GD["STRIDE"], -1, np.int32)
    gc.device_call(hip, gc.MODE_LAYOUT, dtype, a)
    gc.layout_check(name, a, a["desc"])


@pytest.mark.parametrize("name,dtype", [(c.name, dt) for c in gc.SOLVE_CASES for dt in DTYPES if not (c.kind == "chained" and dt == "f32")])
def test_solve(hip, name, dtype):
    case = gc.SOLVE_BY_NAME[name]
    a, aux = gc.solve_inputs(case, dtype)
    if case.kind == "chained":
        gc.chain_eig_rotate(lambda mode, dt, arrays: gc.device_call(hip, mode, dt, arrays), dtype, a, aux)
    a_in = gc.copy_inputs(a)
    info = gc.device_call(hip, case.mode, dtype, a)
    assert info[0] == (1 + a["nblk"] if case.mode == gc.MODE_PANEL else 2 + 2 * a["nblk"])
    ratios = gc.solve_check(case, dtype, a_in, aux, a)
    mode = "panel_solve" if case.mode == gc.MODE_PANEL else "gram_pass"
    print("group_piece %s %s %s worst error / bound = %.3e  %s" % (
        mode, name, dtype, max(ratios.values(), default=0.0), {"%s %s" % k: "%.2e" % v for k, v in sorted(ratios.items())}))
    _note(mode, dtype, ratios)
    assert all(r <= 1.0 for r in ratios.values()), ratios


def test_entry_refuses_what_it_cannot_run(hip):
    """Bad tables are refused with an error string before anything is launched; the pre-filled outputs stay as they were."""
    case = next(c for c in gc.EIG_CASES if c.name == "gram-q16")
    inp, _, _ = gc.eig_inputs(case, "f64")

    def refused(mode, a, outputs):
        with pytest.raises(RuntimeError):
            gc.device_call(hip, mode, "f64", a)
        for k in outputs:
            assert gc.is_prefill(a[k]).all() if a[k].dtype == np.float64 else (a[k] == -1).all(), k

    # a group of 97 values for the eigenbasis kernel
    big = gc.EigCase("q97", [(97, "gram", 1.0)], "tight", 97)
    a, _, _ = gc.eig_inputs(big, "f64")
    refused(gc.MODE_EIG, a, ("vars", "V"))
    a["max_q"] = 96
    refused(gc.MODE_EIG, a, ("vars", "V"))
    # an eigenbasis past the end of V, a block past the end of the source
    a = gc.copy_inputs(inp)
    a["eig"][2] = a["V"].size - 16 * 16 + 1
    refused(gc.MODE_EIG, a, ("vars", "V"))
    a = gc.copy_inputs(inp)
    a["eig"][0] += 1 + 5
    refused(gc.MODE_EIG, a, ("vars", "V"))
    # an unknown mode
    refused(5, gc.copy_inputs(inp), ("vars", "V"))
    # a block of 129 values: in the rotation's offsets and in a pass
    rc = next(c for c in gc.ROT_CASES if c.name == "narrow-mixed-dsrc")
    a, _, _, _ = gc.rot_inputs(rc, "f64", "exact")
    a["goff"][-1] = 129
    refused(gc.MODE_ROTATE, a, ("D",))
    a, _, _, _ = gc.rot_inputs(rc, "f64", "exact")
    a["rvoff"][0] = a["V"].size - 24
    refused(gc.MODE_ROTATE, a, ("D",))
    a, _ = gc.layout_tables([[64, 64, 1]], True, gc._rng("refuse"))
    a["desc"] = np.full(gc.GD["STRIDE"], -1, np.int32)
    refused(gc.MODE_LAYOUT, a, ("desc",))
    # a list index out of range, a list naming a group twice, blk_g0 not increasing
    for change in ("range", "twice", "g0"):
        a, _ = gc.layout_tables([[3, 4], [5, 1]], True, gc._rng("refuse"))
        a["desc"] = np.full(2 * gc.GD["STRIDE"], -1, np.int32)
        if change == "range":
            a["list"][1] = a["ns"]
        elif change == "twice":
            a["list"][1] = a["list"][0]
        else:
            a["blk_g0"][1] = 0
        refused(gc.MODE_LAYOUT, a, ("desc",))
    # the solves: max_active_size < 0, a voff past V
    sc = gc.SOLVE_BY_NAME["panel-newton"]
    for change in ("max_active", "voff"):
        a, _ = gc.solve_inputs(sc, "f64")
        if change == "max_active":
            a["max_active_size"] = -1
        else:
            wide = int(np.argmax(a["ssize"]))
            a["voff"][wide] = a["V"].size - 4
        refused(gc.MODE_PANEL, a, ("dlt", "dd", "dcol", "desc"))


def test_worst_ratios_reported():
    """Prints the worst error / bound per mode, dtype, figure and width class seen by this session's cases."""
    for key, r in sorted(_worst.items()):
        print("group_piece worst %-11s %s %-10s %-8s error / bound = %.3e" % (key + (r,)))
    assert all(r <= 1.0 for r in _worst.values())
