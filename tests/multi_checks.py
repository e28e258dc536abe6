"""The multi-response kernels (adelie_amd/csrc/kernels_multi.hip), one launch at a time, against plain references (no GPU needed
to import).

A *call* is one ``adelie_hip_multi_piece_test``: SWEEP (launch_multi_sweep), STEP (launch_multi_panel_step), FUSED_STEP
(launch_multi_panel_fused beside a solve that changes nothing), BLOCK_LISTS, EXPAND, EXPAND_CROSS, AXPY, TO_MAJOR, FROM_MAJOR and
BATCH_PICK.  This module holds the case tables, the inputs (built from named seeds), the references, ``device_call``,
``emulate_call`` -- a plain numpy emulation in the target dtype that follows the kernels' partition into lanes, tiles, slices and
splits and takes an optional planted defect -- and the derivation of every bound.  tests/test_gpu_multi_pieces.py runs the cases
on the device, tests/test_multi_checks_host.py runs the same checkers on the emulation and on the planted defects.

The view is [1 (x) I_K, X (x) I_K] over a base of nb rows and pb columns: view column c = u K + l is (extended feature u,
response l), u < icpt is the column of ones.  Vectors of nb K values are response-major.  References are computed from the arrays
actually handed to the call (the columns are decoded from the X or bits array of the call, pad rows excluded), in integer numpy on
the exact leg and in ``np.longdouble`` on the rounding leg.  u = 2^-53 / 2^-24 is the unit roundoff, gamma_k = k u / (1 - k u).

Exact leg.  X, v, w, r, dlt, coef are small integers (|x| <= 3, |v| <= 3, |r| <= 8, 0 <= w <= 3, |dlt| <= 3).  Sweep: a sum has
at most 4200 terms of size <= 9: below 2^16.  Step: |r_out| <= 8 + 128 * 9 = 1160, |w r| <= 3480, a slice partial has at most
256 terms of size <= 3 * 3480: below 2^22.  Every product and every partial sum is therefore an integer below 2^24, exact in both
dtypes in any order and with or without fused multiply-adds, and the outputs are asserted bit for bit.  On a dense base the pad
rows (rows nb .. ld of every column) hold integers above 2^22; on a 2-bit base the pad calls of the last byte hold code 3
(missing) with impute values >= 1: one pad row that reaches a sum changes it.

Rounding leg.  Standard normal inputs, a NaN payload in the pad rows; every output must be finite, and per output
|error| <= gamma_d * (sum of the absolute terms), d the longest chain of roundings any summation order of the kernel can have:

* SWEEP.  From the plan in info: a lane accumulates at most ceil(min(rows per split, nb) / 64) terms (the four-wave kernels: 64
  lanes share the rows of a split; the plain kernel's 256 lanes have fewer) with one rounding each (fma), the wave sum adds 6
  levels, the plain kernel's sum over its four waves 4, the sum over the splits nsplit: d = ceil(rows / 64) + 6 + 4 + nsplit.
* STEP, r.  r_out = r_in - sum_m dlt_m x_m over the entries of that response: one fma per entry and the subtraction:
  d = entries of the response + 1, against |r_in| + sum |dlt_m x_m|.
* STEP, part[c][slice] against sum over the slice of x (w r) with r the kernel's OWN output: w r is rounded once, a lane sums
  VEC products, the butterfly over 64 lanes adds 6 levels; the issue's figure d = 64 + VEC + 2 covers any order of the 64 lanes.
* AXPY.  out = r + sign * sum coef_m x_m, per entry one rounded product sign * coef, one product and one sum (or one fma):
  d = 3 * entries, against |r| + sum |coef_m x_m|.
* BATCH_PICK with a subtrahend: one product and one difference, d = 2.
The emulation sums in the same partition but forms a * b + c with two roundings where the kernel uses one (numpy has no fused
multiply-add in float64): it stays within gamma_2d, and its ratios against gamma_d are printed by the host test.
Nothing in these bounds is measured on the code under test.

Bit for bit in both legs: STEP with nz = 0 leaves r unchanged; the pre-fill of part is untouched outside
[0, nb_cols) x [0, slices) and wherever a (feature, response) is not listed; FUSED_STEP gives STEP's r and STEP's partials for
every slice (both run multi_step_phases over the same slices, only the leading dimension of part differs) and exact zeros for the
slices of its last workgroup that lie past nb; BLOCK_LISTS, EXPAND, EXPAND_CROSS, TO_MAJOR, FROM_MAJOR and BATCH_PICK on integer
inputs against numpy, with the pre-fill kept wherever the kernel does not write (ulist past the number of distinct features, D
outside nv x nv, entries of other responses at lsel > 0).

Planted defects (``emulate_call(..., defect=)``): 'tile_parity' (the staged sweep reads LDS tile b ^ 1: the previous tile's
vectors, zeros for the first), 'drop_tail' (the sweep drops its rows past the last whole tile / vector), 'store_dup' (the sweep
stores the clamped duplicates: features past nfeat and responses past K land on their neighbours' slots), 'l0_ignored' (the
second response chunk reads the first chunk's vectors), 'head_prev' (build_slots never starts a slot at an entry whose index is a
multiple of 64: the entry joins the previous feature's slot; the other way to ignore list[m - 1] there -- always starting a slot
-- gives the same bits, since a feature split over two slots adds the same products to different responses), 'pad_unmasked' (the
step multiplies the pad rows of its last slice with zeros: NaN on the rounding leg), 'part_unlisted' (the step stores the partial
of an unlisted response, at column 0), 'expand_zero' (EXPAND zeroes the other responses at lsel > 0).
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from group_checks import DT_CODE, NP_TYPE, UNIT, _rng, bits, gamma, is_prefill, prefill

LD = np.longdouble
VEC = {"f64": 2, "f32": 4}
(MODE_SWEEP, MODE_STEP, MODE_FUSED, MODE_LISTS, MODE_EXPAND, MODE_CROSS, MODE_AXPY, MODE_TO_MAJOR, MODE_FROM_MAJOR,
 MODE_PICK) = range(10)
PLAIN, FOURWAVE, STAGED = 0, 1, 2
VARIANT_NAME = {PLAIN: "plain", FOURWAVE: "four-wave", STAGED: "staged"}
MAXB, MFS, MT = 128, 16, 256
PAD_INT = 1 << 22
DEFECTS = ("tile_parity", "drop_tail", "store_dup", "l0_ignored", "head_prev", "pad_unmasked", "part_unlisted", "expand_zero")

POINTERS = ("X", "bits", "impute", "v", "out", "w", "r", "dcol", "dlt", "cols", "part", "ulist", "slot", "resp", "slot_c", "resp_c",
            "C", "D", "lsel_list")
ARRAY_TYPE = dict(bits=np.uint8, dcol=np.int32, cols=np.int32, ulist=np.int32, slot=np.int32, resp=np.int32, slot_c=np.int32,
                  resp_c=np.int32, lsel_list=np.int64)
SIZED = dict(X="X_elems", bits="bits_elems", part="part_elems", C="C_elems", D="D_elems", dcol="n_dcol", lsel_list="n_lsel")


def device_call(hip, mode, dtype, a):
    """Runs one call on the device.  `a`: field name -> contiguous numpy array (written in place where the mode writes) or
    scalar.  Returns info (8 values)."""
    from adelie_amd import _abi

    s = _abi.MultiPiece()
    s.dtype, s.mode = DT_CODE[dtype], mode
    for k, v in a.items():
        if k in POINTERS:
            if v is None:
                continue
            want = ARRAY_TYPE.get(k, NP_TYPE[dtype])
            assert v.dtype == want and v.flags.c_contiguous, k
            setattr(s, k, v.ctypes.data)
            if k in SIZED and SIZED[k] not in a:
                setattr(s, SIZED[k], v.size)
        else:
            setattr(s, k, v)
    info = np.full(8, -1, dtype=np.int64)
    hip.check(hip.fn("multi_piece_test")(C.byref(s), info.ctypes.data))
    return info


def copy_inputs(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


# ---- the host-side decisions, restated (adelie_amd/csrc/multi_shape.hpp; the host test compares them with the header's) -----------
def kt_of(K):
    return 8 if K > 4 else 4 if K > 2 else 2


def msweep_shape(nb, nfeat, vec, feats):
    blocks_c = (nfeat + feats - 1) // feats
    unit = MT * vec
    max_split = max(1, (nb + unit * 4 - 1) // (unit * 4))
    ns = max(1, (1024 + blocks_c - 1) // blocks_c)
    ns = min(ns, max_split, 65535)
    rps = (nb + ns - 1) // ns
    rps = (rps + unit - 1) // unit * unit
    ns = max(1, (nb + rps - 1) // rps)
    return blocks_c, ns, rps


Plan = namedtuple("Plan", "variant vec kt feats blocks_c nsplit rps kchunks")


def sweep_plan(nb, nfeat, K, vec, base_vec, v_vec):
    kt = kt_of(K)
    wide = kt == 8
    feats = 32 if wide else 8
    blocks_c, ns, rps = msweep_shape(nb, nfeat, vec, feats)
    variant = STAGED if (wide and base_vec and v_vec) else FOURWAVE if wide else PLAIN
    return Plan(variant, vec if base_vec else 1, kt, feats, blocks_c, ns, rps, (K + kt - 1) // kt)


def sweep_work_elems(nb, nfeat, K, vec):
    return max(msweep_shape(nb, nfeat, vec, f)[1] for f in (8, 32, 16)) * nfeat * K + 16


def base_vec_of(a, dtype):
    """Whether the base takes 16-byte loads (multi_vecok): always on a 2-bit base; the allocation is 256-byte aligned."""
    if a.get("bits") is not None:
        return True
    es = 8 if dtype == "f64" else 4
    return a["ld"] % VEC[dtype] == 0 and (a.get("x_off", 0) * es) % 16 == 0


def step_vec(a, dtype):
    return VEC[dtype] if base_vec_of(a, dtype) else 1


def plan_of(a, dtype):
    es = 8 if dtype == "f64" else 4
    v_vec = a["nb"] % VEC[dtype] == 0 and (a.get("v_off", 0) * es) % 16 == 0
    return sweep_plan(a["nb"], a["pb"] + a["icpt"], a["K"], VEC[dtype], base_vec_of(a, dtype), v_vec)


# ---- the view -----------------------------------------------------------------------------------------------------------------------
def dense_base(rng, dtype, leg, nb, pb, ld):
    """X as the caller lays it out: pb columns of ld values, the rows past nb holding the pad."""
    T = NP_TYPE[dtype]
    X = np.empty((pb, ld), dtype=T)
    if leg == "exact":
        X[:, :nb] = rng.randint(-3, 4, size=(pb, nb))
        X[:, nb:] = PAD_INT + np.arange(ld - nb)[None, :] + np.arange(pb)[:, None]
    else:
        X[:, :nb] = rng.normal(size=(pb, nb))
        X[:, nb:] = prefill(dtype, 1)[0]
    return X.reshape(-1)


def snp_base(rng, dtype, leg, nb, pb, ldb):
    """2-bit calls, four per byte: missing calls (code 3) in every column, code 3 in the pad calls and 0xFF in the pad bytes."""
    T = NP_TYPE[dtype]
    codes = rng.randint(0, 3, size=(pb, ldb * 4)).astype(np.uint8)
    miss = rng.uniform(size=(pb, ldb * 4)) < 0.15
    miss[:, rng.randint(0, nb)] = True
    miss[np.arange(pb), rng.randint(0, nb, size=pb)] = True
    codes[miss] = 3
    codes[:, nb:] = 3
    c4 = codes.reshape(pb, ldb, 4)
    by = (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)
    impute = (rng.randint(1, 4, size=pb) if leg == "exact" else rng.uniform(0.5, 1.5, size=pb)).astype(T)
    return by.reshape(-1), impute


def ext_cols(a, dtype, rows=None):
    """The extended features of the call's view, (pb + icpt, rows) in the dtype, decoded from the arrays of the call; rows
    defaults to nb (no pad row).  With rows > nb the pad is included as the kernel would read it unmasked (NaN past the column)."""
    T = NP_TYPE[dtype]
    nb, pb, icpt = a["nb"], a["pb"], a["icpt"]
    rows = nb if rows is None else rows
    E = np.full((pb + icpt, rows), np.nan, dtype=T)
    if icpt:
        E[0, :nb] = 1
        E[0, nb:min(rows, (nb + 31) // 32 * 32)] = 0
    if a.get("bits") is not None:
        ldb = a["ldb"]
        by = a["bits"][:pb * ldb].reshape(pb, ldb)
        codes = np.stack([(by >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(pb, ldb * 4)
        vals = np.where(codes == 3, a["impute"][:, None], codes.astype(T)).astype(T)
        m = min(rows, ldb * 4)
        E[icpt:, :m] = vals[:, :m]
    else:
        ld = a["ld"]
        Xc = a["X"][:pb * ld].reshape(pb, ld)
        m = min(rows, ld)
        E[icpt:, :m] = Xc[:, :m]
    return E


def make_view(rng, dtype, leg, nb, pb, K, icpt, base):
    """base: 'dense' (16-byte loads), 'oddld' / 'xoff' (scalar loads), 'snp'."""
    a = dict(nb=nb, pb=pb, K=K, icpt=icpt)
    if base == "snp":
        ldb = (nb + 3) // 4 + 1
        a["bits"], a["impute"] = snp_base(rng, dtype, leg, nb, pb, ldb)
        a["ldb"] = ldb
    else:
        ld = (nb // 32 + 1) * 32 + (1 if base == "oddld" else 0)
        a["X"] = dense_base(rng, dtype, leg, nb, pb, ld)
        a["ld"] = ld
        a["x_off"] = 1 if base == "xoff" else 0
    return a


def values(rng, dtype, leg, shape, lo=-3, hi=3):
    T = NP_TYPE[dtype]
    return (rng.randint(lo, hi + 1, size=shape) if leg == "exact" else rng.normal(size=shape)).astype(T)


# ---- arithmetic in the target dtype ---------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """a * b + c: one rounding in float32 (through float64), two in float64."""
    if c.dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def worst_ratio(err, bound):
    """max err / bound; where the bound is zero (every term of the sum is zero) the error must be zero."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.isfinite(err).all(), "a non-finite output"
    zero = bound == 0
    assert (err[zero] == 0).all(), "a sum of zeros came out non-zero"
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def tree64(x):
    """Sum over axis 0 (64 lanes) as a binary tree of 6 levels (the shuffle / butterfly order of the kernels)."""
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = x[:h] + x[h:]
    return x[0]


# ---- SWEEP ------------------------------------------------------------------------------------------------------------------------
SweepCase = namedtuple("SweepCase", "name dtype nb pb K icpt base v_off variant")
SWEEP_NB = {"f64": (100, 128, 130, 256, 400, 2600), "f32": (100, 256, 260, 512, 4200)}
SWEEP_K = (1, 2, 3, 4, 5, 8, 9, 11, 16)
SWEEP_NFEAT = (1, 7, 8, 9, 33, 41)


def _sweep_cases():
    out = []

    def add(dtype, nb, nfeat, K, icpt, base="dense", v_off=0):
        if nfeat - icpt < 1:
            icpt = 0
        a = dict(nb=nb, pb=nfeat - icpt, icpt=icpt, K=K, v_off=v_off)
        if base == "snp":
            a["bits"] = True
        else:
            a["ld"] = (nb // 32 + 1) * 32 + (1 if base == "oddld" else 0)
            a["x_off"] = 1 if base == "xoff" else 0
        variant = plan_of(a, dtype).variant
        name = "%s-n%d-f%d-K%d-i%d-%s%s" % (dtype, nb, nfeat, K, icpt, base, "-voff" if v_off else "")
        if all(c.name != name for c in out):
            out.append(SweepCase(name, dtype, nb, nfeat - icpt, K, icpt, base, v_off, variant))

    for dtype in ("f64", "f32"):
        q = 0
        for nb in SWEEP_NB[dtype]:                       # every K at every nb, the feature counts and icpt taking turns
            for K in SWEEP_K:
                add(dtype, nb, SWEEP_NFEAT[q % 6], K, (q // 6) % 2)
                q += 1
        mid, big = SWEEP_NB[dtype][2], SWEEP_NB[dtype][-1]
        for nfeat in SWEEP_NFEAT:                        # every feature count with both icpt at the 1-tile-and-tail shape
            for K in (4, 5, 9):
                for icpt in (0, 1):
                    add(dtype, mid, nfeat, K, icpt)
        for K in (5, 8, 11, 16):                         # the two-split shape in the staged kernel, both chunk counts
            add(dtype, big, 41, K, 1)
            add(dtype, big, 33, K, 0)
        add(dtype, big, 41, 3, 1)                        # ... and in the plain kernel
        odd = {"f64": 131, "f32": 262}[dtype]            # four waves without staging: nb % VEC != 0; v off 16-byte alignment
        for K in (5, 8, 11):
            add(dtype, odd, 33, K, 1)
            add(dtype, SWEEP_NB[dtype][-2], 33, K, 1, v_off=1)
            add(dtype, big, 9, K, 0, v_off=1)
        for base in ("oddld", "xoff"):                   # scalar loads: odd leading dimension; X off 16-byte alignment
            for K in (2, 4, 8, 11):
                add(dtype, mid, 9, K, 1, base)
            add(dtype, big, 41, 8, 0, base)
            add(dtype, odd, 7, 3, 0, base)
        for nb in (131, 262, 2601):                      # 2-bit base, nb % 4 != 0, missing calls in every column
            for K in (2, 5, 11):
                add(dtype, nb, 9, K, 1, "snp")
                add(dtype, nb, 33, K, 0, "snp")
        for K in (5, 11):                                # ... and the staged kernel on a 2-bit base (nb % VEC == 0)
            add(dtype, 260, 9, K, 1, "snp")
    return out


SWEEP_CASES = _sweep_cases()
SWEEP_BY_NAME = {c.name: c for c in SWEEP_CASES}


def sweep_inputs(case, leg):
    rng = _rng("sweep %s %s" % (case.name, leg))
    a = make_view(rng, case.dtype, leg, case.nb, case.pb, case.K, case.icpt, case.base)
    a["v"] = values(rng, case.dtype, leg, case.K * case.nb)
    a["v_off"] = case.v_off
    a["out"] = prefill(case.dtype, (case.pb + case.icpt) * case.K)
    return a


def _lane_steps(variant, vec, r0, r1, drop_tail):
    """The rows a lane adds, in order: a list of (rows [RT], tile index or -1); rows < 0 where the lane idles."""
    RT = MT if variant == PLAIN else 64
    lane = np.arange(RT)
    steps = []
    if variant == STAGED:
        TR = 64 * vec
        nt = (r1 - r0) // TR
        for it in range(nt):
            for e in range(vec):
                steps.append((r0 + it * TR + lane * vec + e, it))
        t0 = r0 + nt * TR
    else:
        t0 = r0 + (r1 - r0) // vec * vec
        i = r0 + lane * vec
        while i[0] < t0:
            for e in range(vec):
                steps.append((np.where(i < t0, i + e, -1), -1))
            i = i + RT * vec
    if not drop_tail:
        i = t0 + lane
        while i[0] < r1:
            steps.append((np.where(i < r1, i, -1), -1))
            i = i + RT
    return steps


def emulate_sweep(dtype, a, defect=None):
    T = NP_TYPE[dtype]
    nb, K, nfeat = a["nb"], a["K"], a["pb"] + a["icpt"]
    pl = plan_of(a, dtype)
    E = ext_cols(a, dtype)                       # (nfeat, nb)
    v = a["v"].reshape(K, nb)
    if defect == "l0_ignored":
        v = v[[l if l < pl.kt else min(l - l // pl.kt * pl.kt, K - 1) for l in range(K)]]
    work = np.zeros(max(sweep_work_elems(nb, nfeat, K, VEC[dtype]), 1), dtype=T)
    TR = 64 * pl.vec
    with np.errstate(invalid="ignore", over="ignore"):
        for sp in range(pl.nsplit):
            r0 = sp * pl.rps
            r1 = min(nb, r0 + pl.rps)
            RT = MT if pl.variant == PLAIN else 64
            acc = np.zeros((RT, nfeat, K), dtype=T)
            for rows, it in _lane_steps(pl.variant, pl.vec, r0, r1, defect == "drop_tail"):
                ok = rows >= 0
                rc = np.where(ok, rows, 0)
                x = E[:, rc].T
                if defect == "tile_parity" and it >= 0:
                    vv = v[:, rc - TR].T if it > 0 else np.zeros((RT, K), dtype=T)
                else:
                    vv = v[:, rc].T
                new = fma(x[:, :, None], vv[:, None, :], acc)
                acc = np.where(ok[:, None, None], new, acc)
            if pl.variant == PLAIN:
                red = [tree64(acc[64 * w:64 * w + 64]) for w in range(4)]
                s = np.zeros((nfeat, K), dtype=T)
                for w in range(4):
                    s = s + red[w]
            else:
                s = tree64(acc)
            work[sp * nfeat * K:(sp + 1) * nfeat * K] = s.reshape(-1)
            if defect == "store_dup":
                for u in range(pl.blocks_c * pl.feats):
                    for l in range(pl.kchunks * pl.kt):
                        if u < nfeat and l < K:
                            continue
                        q = (sp * nfeat + u) * K + l
                        if q < work.size:
                            work[q] = s[min(u, nfeat - 1), min(l, K - 1)]
        out = np.zeros(nfeat * K, dtype=T)
        for sp in range(pl.nsplit):
            out = out + work[sp * nfeat * K:(sp + 1) * nfeat * K]
    a["out"][:] = out
    return np.array(list(pl), dtype=np.int64)


def sweep_depth(info, nb):
    rows = min(int(info[6]), nb)
    return (rows + 63) // 64 + 6 + 4 + int(info[5])


def sweep_check(case, leg, a, info):
    """Asserts the plan and, on the exact leg, the bits; returns {'sweep': worst error / bound} on the rounding leg."""
    dtype = case.dtype
    pl = plan_of(a, dtype)
    assert tuple(int(x) for x in info) == tuple(pl), (tuple(info), pl)
    assert info[0] == case.variant, "%s ran, %s intended" % (VARIANT_NAME[int(info[0])], VARIANT_NAME[case.variant])
    nb, K, nfeat = a["nb"], a["K"], a["pb"] + a["icpt"]
    E = ext_cols(a, dtype)
    v = a["v"].reshape(K, nb)
    out = a["out"].reshape(nfeat, K)
    if leg == "exact":
        ref = E.astype(np.int64) @ v.astype(np.int64).T
        assert np.abs(ref).max() < 2 ** 24
        assert np.array_equal(out, ref.astype(out.dtype)), "sweep differs from the integer reference at %s" % (
            np.argwhere(out != ref.astype(out.dtype))[:4].tolist())
        return {}
    assert np.isfinite(out).all(), "a pad row reached the sweep"
    ref = E.astype(LD) @ v.astype(LD).T
    mag = np.abs(E).astype(LD) @ np.abs(v).astype(LD).T
    bound = gamma(sweep_depth(info, nb), UNIT[dtype]) * mag
    return {"sweep": worst_ratio(np.abs(out.astype(LD) - ref), bound)}


# ---- STEP / FUSED_STEP ----------------------------------------------------------------------------------------------------------------
# nb: a row count, or 'T' (64 * VEC: exactly one full slice) / 'T+1'; dkind / ckind: how the change list / the gradient list is laid out
StepCase = namedtuple("StepCase", "name nb K pb icpt base nz nz_dev nb_cols dkind ckind")


def _step_cases():
    out = []

    def add(nb, K, base, nz, nb_cols, dkind="groups", ckind="groups", icpt=1, nz_dev=None):
        pb = (max(nz, nb_cols, 8) + K - 1) // K + 3
        name = "n%s-K%d-%s-nz%d%s-c%d-%s-%s-i%d" % (nb, K, base, nz, "" if nz_dev is None else "dev%d" % nz_dev, nb_cols, dkind, ckind, icpt)
        out.append(StepCase(name, nb, K, pb, icpt, base, nz, nz if nz_dev is None else nz_dev, nb_cols, dkind, ckind))

    nzs, ncs, Ks = (0, 1, 8, 9, 17, 128), (1, 64, 65, 128, 256), (1, 2, 3, 4, 5, 8, 11)
    q = 0
    for nb in (40, "T", "T+1", 1031):                    # every row count on every base
        for base in ("dense", "oddld", "xoff", "snp"):
            add(nb, Ks[q % 7], base, nzs[(q + 2) % 6], ncs[q % 5], icpt=q % 2)
            q += 1
    for nz in nzs:                                       # every nz and every nb_cols on the vector-loaded base
        add(1031, 3, "dense", nz, 64)
    add(1031, 3, "dense", 128, 64, nz_dev=200)           # nz_dev above 128: the kernel stops at 128
    for nc in ncs:
        add("T+1", 4, "dense", 9, nc)
        add(40, 5, "snp", 17, nc, icpt=0)
    for K in (2, 3, 4, 8):                               # entries 63 and 64 (the 64th and 65th) belong to one feature
        add(130, K, "dense", 128, 128, "straddle", "straddle")
    add(130, 3, "oddld", 128, 256, "straddle", "straddle")  # ... and entries 127 / 128 of the two-block gradient list
    add(130, 3, "dense", 17, 65, "resp02", "resp02")     # a feature present for responses 0 and 2 only
    add(130, 4, "snp", 17, 65, "resp02", "resp02")
    add(130, 3, "dense", 17, 65, "twice", "twice")       # a feature listed twice, non-consecutively
    add(130, 2, "xoff", 9, 17, "twice", "twice", icpt=0)
    add(130, 11, "dense", 128, 128)                      # entries with l >= 8 at K = 11; the ones feature leads both lists
    add("T+1", 11, "snp", 17, 65, "resp02", "twice")
    return out


STEP_CASES = _step_cases()
STEP_BY_NAME = {c.name: c for c in STEP_CASES}


def step_nb(case, dtype):
    return {"T": 64 * VEC[dtype], "T+1": 64 * VEC[dtype] + 1}.get(case.nb, case.nb)


def make_list(rng, n, nfeat, K, kind, lead_ones):
    """n distinct view columns, the responses of a feature next to each other as the solver's groups are."""
    feats = list(rng.permutation(nfeat))
    if lead_ones:                                         # the ones feature (u = 0) first
        feats.remove(0)
        feats.insert(0, 0)
    groups = [[u * K + l for l in range(K)] for u in feats]
    if kind == "straddle" and K > 1:
        if 64 % K == 0:
            groups[0] = groups[0][1:]                     # shift the group boundaries off the multiples of 64
    elif kind == "resp02" and K >= 3:
        groups[1] = [groups[1][0], groups[1][2]]
    elif kind == "twice" and K >= 2:
        g = groups[1]
        groups[1], tail = g[:1], g[1:]
        groups.insert(3, tail)                            # the rest of feature groups[1] behind another feature
    flat = [c for g in groups for c in g]
    assert len(flat) >= n, (len(flat), n)
    lst = np.array(flat[:n], dtype=np.int32)
    if kind == "straddle" and n > 64 and K > 1:
        assert lst[63] // K == lst[64] // K
    return lst


def step_inputs(case, dtype, leg):
    rng = _rng("step %s %s %s" % (case.name, dtype, leg))
    nb, K = step_nb(case, dtype), case.K
    a = make_view(rng, dtype, leg, nb, case.pb, K, case.icpt, case.base)
    nfeat = case.pb + case.icpt
    a["w"] = (rng.randint(0, 4, size=K * nb) if leg == "exact" else rng.uniform(0.5, 1.5, size=K * nb)).astype(NP_TYPE[dtype])
    a["r"] = values(rng, dtype, leg, K * nb, -8, 8)
    a["dcol"] = make_list(rng, case.nz, nfeat, K, case.dkind, case.icpt == 1)
    a["dlt"] = values(rng, dtype, leg, case.nz)
    if leg == "exact":
        a["dlt"][a["dlt"] == 0] = 2
    a["n_dcol"] = case.nz
    a["nz"] = case.nz_dev
    a["cols"] = make_list(rng, case.nb_cols, nfeat, K, case.ckind, case.icpt == 1)
    a["nb_cols"] = case.nb_cols
    return a


def part_ld(a, dtype, fused):
    sl = -(-a["nb"] // (64 * step_vec(a, dtype)))
    return -(-sl // MFS) * MFS if fused else sl


def with_part(a, dtype, fused, extra=5):
    """The call's arrays with a pre-filled part: nb_cols * ld and `extra` elements behind it that nothing may touch."""
    b = copy_inputs(a)
    b["part"] = prefill(dtype, a["nb_cols"] * part_ld(a, dtype, fused) + extra)
    return b


def build_slots(lst, K, defect=None):
    """feat per slot and the slot of every entry (kernels_multi.hip::build_slots)."""
    feat, slot = [], []
    for m, col in enumerate(lst):
        u = int(col) // K
        head = m == 0 or u != int(lst[m - 1]) // K
        if defect == "head_prev" and m > 0 and m % 64 == 0:
            head = False
        if head:
            feat.append(u)
        slot.append(len(feat) - 1)
    return feat, slot


def emulate_step(dtype, a, fused=False, defect=None):
    T = NP_TYPE[dtype]
    nb, K = a["nb"], a["K"]
    vec = step_vec(a, dtype)
    RS = 64 * vec
    nsl = -(-nb // RS)
    ld = part_ld(a, dtype, fused)
    nrow = ld * RS if fused else nsl * RS
    E = ext_cols(a, dtype, nrow)
    if defect != "pad_unmasked":
        E[:, nb:] = 0
    nz = min(int(a["nz"]), MAXB)
    nbc = a["nb_cols"] if fused else min(a["nb_cols"], 2 * MAXB)
    featA, slotA = build_slots(a["dcol"][:nz], K, defect)
    featB, slotB = build_slots(a["cols"][:nbc], K, defect)
    r = a["r"].reshape(K, nb)
    w = a["w"].reshape(K, nb)
    part = a["part"]
    kt = kt_of(K)
    with np.errstate(invalid="ignore", over="ignore"):
        # (A) per response: one fma per slot of the list, the slots in order (a slot that does not list the response adds 0)
        dA = np.zeros((len(featA), K), dtype=T)
        for m in range(nz):
            dA[slotA[m], int(a["dcol"][m]) % K] = a["dlt"][m]
        acc = np.zeros((K, nb), dtype=T)
        for s_, u in enumerate(featA):
            acc = fma(dA[s_][:, None], E[u, :nb][None, :], acc)
        if featA:
            r[:] = r - acc
        wr = np.zeros((K, nrow), dtype=T)
        wr[:, :nb] = w * r
        # (B) per slot and listed response: VEC fmas per lane, the butterfly over the 64 lanes, one partial per slice
        valB = {}
        for m in range(nbc):
            valB[(slotB[m], int(a["cols"][m]) % K)] = m
        nslice = nrow // RS
        for s_, u in enumerate(featB):
            x = E[u].reshape(nslice, 64, vec)
            for l in range((K + kt - 1) // kt * kt):
                c = valB.get((s_, l), -1)
                if c < 0 and not (defect == "part_unlisted" and l < K):
                    continue
                d = np.zeros((nslice, 64), dtype=T)
                wl = wr[min(l, K - 1)].reshape(nslice, 64, vec)
                for e in range(vec):
                    d = fma(x[:, :, e], wl[:, :, e], d)
                tot = tree64(d.T)
                part[max(c, 0) * ld:max(c, 0) * ld + nslice] = tot
    return np.array([ld, vec, 0, 0, 0, 0, 0, 0], dtype=np.int64)


def step_check(case, dtype, leg, a_in, a, info, fused=False):
    """The r and part of a STEP / FUSED_STEP call against the references; returns the worst ratios of the rounding leg."""
    nb, K = a["nb"], a["K"]
    vec = step_vec(a, dtype)
    RS = 64 * vec
    nsl = -(-nb // RS)
    ld = part_ld(a, dtype, fused)
    assert (int(info[0]), int(info[1])) == (ld, vec), (info[:2], ld, vec)
    assert vec == (1 if case.base in ("oddld", "xoff") else VEC[dtype])
    E = ext_cols(a_in, dtype)
    nz = min(int(a["nz"]), MAXB)
    dcol, dlt, cols = a_in["dcol"][:nz], a_in["dlt"][:nz], a_in["cols"]
    r_in, r = a_in["r"].reshape(K, nb), a["r"].reshape(K, nb)
    w = a_in["w"].reshape(K, nb)
    nbc = a["nb_cols"]
    part = a["part"]
    P = part[:nbc * ld].reshape(nbc, ld)
    assert is_prefill(part[nbc * ld:]).all(), "part written past nb_cols * ld"
    if not fused:
        assert nsl == ld
    else:
        assert np.array_equal(bits(np.ascontiguousarray(P[:, nsl:])), np.zeros((nbc, ld - nsl), dtype=bits(P).dtype)), \
            "a slice past nb holds something other than +0"
    for k in ("w", "dlt"):
        assert np.array_equal(bits(a[k]), bits(a_in[k]))
    if nz == 0:
        assert np.array_equal(bits(a["r"]), bits(a_in["r"])), "nz = 0 changed r"
    pad = nsl * RS - nb
    ratios = {}
    if leg == "exact":
        I = np.int64
        ref_r = r_in.astype(I).copy()
        for m in range(nz):
            ref_r[int(dcol[m]) % K] -= int(dlt[m]) * E[int(dcol[m]) // K].astype(I)
        assert np.abs(ref_r).max() < 2 ** 24
        assert np.array_equal(r, ref_r.astype(r.dtype)), "r differs from the integer reference"
        wr = np.pad(w.astype(I) * ref_r, ((0, 0), (0, pad)))
        for c in range(nbc):
            u, l = int(cols[c]) // K, int(cols[c]) % K
            ref = (np.pad(E[u].astype(I), (0, pad)) * wr[l]).reshape(nsl, RS).sum(axis=1)
            assert np.abs(ref).max() < 2 ** 24
            assert np.array_equal(P[c, :nsl], ref.astype(P.dtype)), "part[%d] differs from the integer reference" % c
        return ratios
    assert np.isfinite(r).all() and np.isfinite(P).all(), "a pad row reached the step"
    u_ = UNIT[dtype]
    ref_r, mag, cnt = r_in.astype(LD).copy(), np.abs(r_in).astype(LD), np.zeros(K, dtype=int)
    for m in range(nz):
        l, x = int(dcol[m]) % K, E[int(dcol[m]) // K].astype(LD)
        ref_r[l] -= LD(dlt[m]) * x
        mag[l] += abs(LD(dlt[m])) * np.abs(x)
        cnt[l] += 1
    worst = 0.0
    for l in range(K):
        if cnt[l] == 0:
            assert np.array_equal(bits(np.ascontiguousarray(r[l])), bits(np.ascontiguousarray(r_in[l]))), "an unlisted response's r changed"
        else:
            worst = max(worst, worst_ratio(np.abs(r[l].astype(LD) - ref_r[l]), gamma(cnt[l] + 1, u_) * mag[l]))
    ratios["r"] = worst
    wr = np.pad(w.astype(LD) * r.astype(LD), ((0, 0), (0, pad)))        # from the kernel's own r
    g = gamma(64 + vec + 2, u_)
    worst = 0.0
    for c in range(nbc):
        x = np.pad(E[int(cols[c]) // K].astype(LD), (0, pad))
        t = (x * wr[int(cols[c]) % K]).reshape(nsl, RS)
        ref, m_ = t.sum(axis=1), np.abs(t).sum(axis=1)
        worst = max(worst, worst_ratio(np.abs(P[c, :nsl].astype(LD) - ref), g * m_))
    ratios["part"] = worst
    return ratios


def fused_equals_step(a_step, a_fused, dtype):
    """FUSED_STEP's r and per-slice partials are STEP's, bit for bit."""
    nbc = a_step["nb_cols"]
    ls, lf = part_ld(a_step, dtype, False), part_ld(a_step, dtype, True)
    assert np.array_equal(bits(a_step["r"]), bits(a_fused["r"])), "r of the fused step differs from the step's"
    Ps = a_step["part"][:nbc * ls].reshape(nbc, ls)
    Pf = a_fused["part"][:nbc * lf].reshape(nbc, lf)[:, :ls]
    assert np.array_equal(bits(np.ascontiguousarray(Ps)), bits(np.ascontiguousarray(Pf))), "partials of the fused step differ from the step's"


# ---- AXPY ---------------------------------------------------------------------------------------------------------------------------
AxpyCase = namedtuple("AxpyCase", "name nb K pb icpt base cnt n_dcol sign")
AXPY_CASES = [AxpyCase("n257-K3-dense", 257, 3, 9, 1, "dense", 17, 20, -1.0), AxpyCase("n130-K11-oddld", 130, 11, 5, 1, "oddld", 40, 40, 1.0),
              AxpyCase("n131-K2-snp", 131, 2, 9, 0, "snp", 9, 9, -1.0), AxpyCase("n40-K1-zero", 40, 1, 9, 1, "dense", 0, 4, 1.0)]


def axpy_inputs(case, dtype, leg):
    rng = _rng("axpy %s %s %s" % (case.name, dtype, leg))
    a = make_view(rng, dtype, leg, case.nb, case.pb, case.K, case.icpt, case.base)
    a["r"] = values(rng, dtype, leg, case.K * case.nb, -8, 8)
    a["dcol"] = make_list(rng, case.n_dcol, case.pb + case.icpt, case.K, "groups", case.icpt == 1)
    a["dlt"] = values(rng, dtype, leg, case.n_dcol)
    a["nz"], a["sign"] = case.cnt, case.sign
    return a


def emulate_axpy(dtype, a):
    T = NP_TYPE[dtype]
    nb, K = a["nb"], a["K"]
    E = ext_cols(a, dtype)
    out = a["r"].reshape(K, nb)
    for m in range(int(a["nz"])):
        c = int(a["dcol"][m])
        out[c % K] = out[c % K] + (T(a["sign"]) * a["dlt"][m]) * E[c // K]
    return np.zeros(8, dtype=np.int64)


def axpy_check(case, dtype, leg, a_in, a):
    nb, K = a["nb"], a["K"]
    E = ext_cols(a_in, dtype)
    Tref = np.int64 if leg == "exact" else LD
    ref, mag, cnt = a_in["r"].reshape(K, nb).astype(Tref), np.abs(a_in["r"].reshape(K, nb)).astype(LD), np.zeros(K, dtype=int)
    for m in range(case.cnt):
        c = int(a_in["dcol"][m])
        t = Tref(a_in["dlt"][m]) * E[c // K].astype(Tref)
        ref[c % K] += Tref(case.sign) * t
        mag[c % K] += np.abs(t).astype(LD)
        cnt[c % K] += 1
    out = a["r"].reshape(K, nb)
    if leg == "exact":
        assert np.array_equal(out, ref.astype(out.dtype))
        return {}
    assert np.isfinite(out).all()
    worst = 0.0
    for l in range(K):
        if cnt[l] == 0:
            assert np.array_equal(bits(np.ascontiguousarray(out[l])), bits(np.ascontiguousarray(a_in["r"].reshape(K, nb)[l])))
        else:
            worst = max(worst, worst_ratio(np.abs(out[l].astype(LD) - ref[l]), gamma(3 * cnt[l], UNIT[dtype]) * mag[l]))
    return {"axpy": worst}


# ---- BLOCK_LISTS, EXPAND, EXPAND_CROSS, TO_MAJOR, FROM_MAJOR, BATCH_PICK (integer inputs, bit for bit) ---------------------------------
ListCase = namedtuple("ListCase", "name nv K kind")
LIST_CASES = [ListCase("nv%d-K%d-%s" % (nv, K, kind), nv, K, kind)
              for nv, K, kind in ((1, 1, "groups"), (7, 3, "twice"), (64, 4, "groups"), (65, 3, "straddle"), (128, 11, "groups"),
                                  (128, 1, "groups"), (128, 3, "twice"), (100, 5, "resp02"))]


def lists_inputs(case):
    rng = _rng("lists " + case.name)
    nfeat = case.nv // case.K + 6
    cols = make_list(rng, case.nv, nfeat, case.K, case.kind, False) + np.int32(case.K * 1000)   # features need not start at 0
    return dict(K=case.K, nv=case.nv, cols=cols, ulist=np.full(case.nv, -7, np.int32), slot=np.full(case.nv, -7, np.int32),
                resp=np.full(case.nv, -7, np.int32))


def lists_reference(cols, K):
    ulist, slot = [], []
    for c in cols:
        u = int(c) // K
        if u not in ulist:
            ulist.append(u)
        slot.append(ulist.index(u))
    return np.array(ulist, np.int32), np.array(slot, np.int32), (cols % K).astype(np.int32)


def emulate_lists(a):
    u, s, r = lists_reference(a["cols"], a["K"])
    a["ulist"][:u.size], a["slot"][:], a["resp"][:] = u, s, r


def lists_check(a):
    u, s, r = lists_reference(a["cols"], a["K"])
    assert np.array_equal(a["ulist"][:u.size], u) and (a["ulist"][u.size:] == -7).all(), "ulist"
    assert np.array_equal(a["slot"], s) and np.array_equal(a["resp"], r)


ExpandCase = namedtuple("ExpandCase", "name nv nc K lsels")       # nc = 0: EXPAND on nv x nv, otherwise EXPAND_CROSS on nv x nc
EXPAND_CASES = [ExpandCase("nv1-K1-all", 1, 0, 1, (-1,)), ExpandCase("nv65-K3-all", 65, 0, 3, (-1,)), ExpandCase("nv128-K5-all", 128, 0, 5, (-1,)),
                ExpandCase("nv65-K3-seq", 65, 0, 3, (0, 1, 2)), ExpandCase("nv128-K11-seq", 128, 0, 11, tuple(range(11))),
                ExpandCase("nv100-K4-only2", 100, 0, 4, (2,)), ExpandCase("nv100-K4-only0", 100, 0, 4, (0,)),
                ExpandCase("cross-65x128-K3", 65, 128, 3, ()), ExpandCase("cross-128x1-K11", 128, 1, 11, ()), ExpandCase("cross-1x64-K2", 1, 64, 2, ())]


def expand_inputs(case, dtype):
    rng = _rng("expand " + case.name)
    T = NP_TYPE[dtype]
    K = case.K

    def lists(n):
        cols = make_list(rng, n, n // K + 6, K, "twice" if K > 1 else "groups", False)
        _, slot, resp = lists_reference(cols, K)
        return slot, resp

    a = dict(nv=case.nv)
    a["slot"], a["resp"] = lists(case.nv)
    ncols = case.nc or case.nv
    if case.nc:
        a["nc"] = case.nc
        a["slot_c"], a["resp_c"] = lists(case.nc)
    ldc = max(int(a["slot"].max()), int(a.get("slot_c", a["slot"]).max())) + 2
    a["ldc"] = ldc
    a["C"] = rng.randint(-99, 100, size=ldc * ldc).astype(T)
    a["ldd"] = case.nv + 3
    a["D"] = prefill(dtype, ncols * a["ldd"])
    if not case.nc:
        a["lsel_list"] = np.array(case.lsels, dtype=np.int64)
    return a


def emulate_expand(a, defect=None):
    nv, ldc, ldd = a["nv"], a["ldc"], a["ldd"]
    C = a["C"].reshape(-1, ldc)                      # C[col, row]: column-major
    if "slot_c" in a:
        D = a["D"].reshape(a["nc"], ldd)
        same = a["resp"][None, :] == a["resp_c"][:, None]
        D[:, :nv] = np.where(same, C[a["slot_c"][:, None], a["slot"][None, :]], 0)
        return
    D = a["D"].reshape(nv, ldd)
    vals = C[a["slot"][:, None], a["slot"][None, :]]
    for lsel in a["lsel_list"]:
        same = a["resp"][None, :] == a["resp"][:, None]
        hit = same & ((lsel < 0) | (a["resp"][None, :] == lsel))
        zero = ~hit & ((lsel <= 0) or defect == "expand_zero")
        D[:, :nv] = np.where(hit, vals, np.where(zero, 0, D[:, :nv]))


def expand_check(a_in, a):
    nv, ldd = a["nv"], a["ldd"]
    ref = copy_inputs(a_in)
    emulate_expand(ref)
    assert np.array_equal(bits(a["D"]), bits(ref["D"])), "D differs from numpy's expansion (or a pre-filled entry changed)"
    ncols = a.get("nc") or nv
    assert is_prefill(a["D"].reshape(ncols, ldd)[:, nv:]).all()
    if "lsel_list" in a and a["lsel_list"][0] > 0:
        other = a["resp"][None, :] != a["resp"][:, None]
        assert is_prefill(a["D"].reshape(nv, ldd)[:, :nv][other]).all(), "entries between different responses must survive lsel > 0"


MajorCase = namedtuple("MajorCase", "name nb K")
MAJOR_CASES = [MajorCase("n%d-K%d" % (nb, K), nb, K) for nb, K in ((1, 1), (255, 3), (256, 5), (257, 11), (1031, 2))]
PickCase = namedtuple("PickCase", "name nfeat K slot sub")
PICK_CASES = [PickCase("f%d-K%d-s%d-%s" % (f, K, s, "sub" if sub else "plain"), f, K, s, sub)
              for f, K, s, sub in ((1, 1, 0, False), (255, 3, 2, True), (257, 16, 15, False), (1000, 5, 0, True))]


def major_inputs(case, dtype, leg="exact"):
    rng = _rng("major " + case.name)
    return dict(nb=case.nb, K=case.K, v=values(rng, dtype, leg, case.nb * case.K, -99, 99), out=prefill(dtype, case.nb * case.K))


def major_reference(a, to_major):
    nb, K = a["nb"], a["K"]
    return a["v"].reshape(nb, K).T.reshape(-1) if to_major else a["v"].reshape(K, nb).T.reshape(-1)


def pick_inputs(case, dtype, leg):
    rng = _rng("pick %s %s" % (case.name, leg))
    a = dict(pb=case.nfeat, K=case.K, lsel=case.slot, v=values(rng, dtype, leg, case.nfeat * case.K, -99, 99), out=prefill(dtype, case.nfeat),
             sign=3.0 if leg == "exact" else 0.7)
    if case.sub:
        a["w"] = values(rng, dtype, leg, case.nfeat, -9, 9)
    return a


def emulate_pick(dtype, a):
    T = NP_TYPE[dtype]
    s = a["v"].reshape(a["pb"], a["K"])[:, a["lsel"]].copy()
    if a.get("w") is not None:
        s = s - T(a["sign"]) * a["w"]
    a["out"][:] = s


def pick_check(dtype, leg, a):
    src = a["v"].reshape(a["pb"], a["K"])[:, a["lsel"]]
    if a.get("w") is None:
        assert np.array_equal(bits(a["out"]), bits(np.ascontiguousarray(src)))
        return {}
    scale = NP_TYPE[dtype](a["sign"])
    if leg == "exact":
        assert np.array_equal(a["out"], src - scale * a["w"])
        return {}
    ref = src.astype(LD) - LD(scale) * a["w"].astype(LD)
    mag = np.abs(src).astype(LD) + abs(LD(scale)) * np.abs(a["w"]).astype(LD)
    return {"pick": worst_ratio(np.abs(a["out"].astype(LD) - ref), gamma(2, UNIT[dtype]) * mag)}


# ---- one emulated call ------------------------------------------------------------------------------------------------------------
def emulate_call(mode, dtype, a, defect=None):
    """The call in plain numpy in the target dtype, outputs written into `a` as the device call writes them; returns info."""
    if mode == MODE_SWEEP:
        return emulate_sweep(dtype, a, defect)
    if mode in (MODE_STEP, MODE_FUSED):
        return emulate_step(dtype, a, mode == MODE_FUSED, defect)
    if mode == MODE_AXPY:
        return emulate_axpy(dtype, a)
    if mode == MODE_LISTS:
        emulate_lists(a)
    elif mode in (MODE_EXPAND, MODE_CROSS):
        emulate_expand(a, defect)
    elif mode in (MODE_TO_MAJOR, MODE_FROM_MAJOR):
        a["out"][:] = major_reference(a, mode == MODE_TO_MAJOR)
    elif mode == MODE_PICK:
        emulate_pick(dtype, a)
    return np.zeros(8, dtype=np.int64)
