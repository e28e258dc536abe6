"""The MFMA block builds of the panel engine against a plain numpy reference (no GPU needed to import this).

A *case* is one call of ``adelie_hip_block_build_test``: one build launch and its reduce, through the launcher the solver
calls, on a design of one kind and type.  This module holds the case table, the inputs of the two legs, the reference and the
bounds; tests/test_gpu_block_builds.py runs the cases on the device, tests/test_block_build_cases.py checks the table itself.

Exact leg.  X holds integers in [-3, 3] (2-bit designs: the calls 0 / 1 / 2 and missing calls imputed with a dyadic value),
w_i in {0, 1/2, 1, 2}, xm multiples of 1/4 with |xm| <= 4.  Every product w x x and xm xm is then a multiple of 1/16 and every
partial sum, in any order, with or without FMA, is an integer number of sixteenths below H = max_ab sum_i |w_i x_ia x_ib| +
|xm_a xm_b|.  While 16 H < 2^24 (float32; 2^53 for float64) all of them are exactly representable, so the device result must be
the reference bit for bit.  ``exact_headroom`` computes 16 H and the tests assert the condition before they compare.

Rounding leg.  Gaussian X, uniform weights summing to one (some of them zero), the true weighted means as xm, all rounded to the
design's type first; the reference is computed from the rounded inputs in extended precision.  A sum of n terms w x x evaluated
in any order in arithmetic of unit roundoff u (one rounding for w x, one per accumulation, fused or not) is within
(n + 1) u sum |w x x| of the exact sum to first order; the product xm xm and the final subtraction add u |xm xm| and
u |C| <= u (sum |w x x| + |xm xm|).  Hence

    |C - C_ref|_ab <= (n + 4) u sum_i |w_i x_ia x_ib| + 2 u |xm_a xm_b|,        u = 2^-53 or 2^-24,

the two spare units of sum |w x x| covering the second-order terms.  An f64 build that went through f32 anywhere misses it by
a factor of 2^29 / n.
"""
import zlib
from collections import namedtuple

import numpy as np

MODE_SYRK, MODE_SYRK_BATCH, MODE_GRAM, MODE_GRAM_BATCH, MODE_STRIP = range(5)
# info[0] of adelie_hip_block_build_test
L_SYRK, L_SYRK_BATCH, L_GRAM, L_GRAM_BATCH, L_STRIP, L_BLOCK_CSC, L_GRAM_CSC = range(1, 8)
INFO = ("launcher", "nsplit", "kchunk", "tile", "n128", "n64", "vec16", "strip_lt", "symmetric", "csc_row_blocks")

P_DENSE = 448   # columns of the dense and 2-bit designs of the tests
P_CSC = 24
CSC_EMPTY, CSC_FULL = 3, 5   # columns of a compressed-column design without entries / with every entry stored
SNP_ALL_MISSING, SNP_ALL_ZERO = 7, 11
N_CSC_TWO_BLOCKS = (1 << 17) + 1   # csc_block_layout: float64 row blocks of 2^20 / 8 rows; the smallest n with two of them
SLOT = 128 * 128

NP_TYPE = {"f64": np.float64, "f32": np.float32}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
EXACT_LIMIT = {"f64": 2 ** 53, "f32": 2 ** 24}
NAN_BITS = {"f64": np.uint64(0x7FF8DEAD0000BEEF), "f32": np.uint32(0x7FC0BEEF)}
BITS = {"f64": np.uint64, "f32": np.uint32}

# name; design kind ('dense', 'snp', 'csc'); 'f64' / 'f32'; mode; rows the build sees; rows of the design skipped in front of
# them; column list; table rows; centring; leading dimension; plain f64 strip kernel; elements of the two outputs; what info
# must report (key -> value, or key -> (lo, hi) bounds); the blocks (see Block)
Case = namedtuple("Case", "name kind dtype mode n row_off cols table center ldc strip_plain out0 out1 expect blocks")
# one block of the result: values x_rows^T W x_cols - xm xm^T at buf[dst + (rpos0 + a) + (cpos0 + b) ldc] and, with `mirror`,
# at buf[dst + (cpos0 + b) + (rpos0 + a) ldc] as well
Block = namedtuple("Block", "buf dst rows cols rpos0 cpos0 mirror")


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def design_key(case):
    return (case.kind, case.dtype, case.n + case.row_off)


def make_design_values(kind, dtype, n_rows, leg):
    """The design's values as float64 (already representable in `dtype`) and what is needed to create it:
    dense: (X, X); snp: (X, (calls int8, impute float64)); csc: (X, X) with exact zeros where nothing is stored."""
    rng = np.random.RandomState(zlib.crc32(("%s %s %d %s" % (kind, dtype, n_rows, leg)).encode()) & 0x7FFFFFFF)
    T = NP_TYPE[dtype]
    if kind == "dense":
        if leg == "exact":
            X = rng.randint(-3, 4, size=(n_rows, P_DENSE)).astype(np.float64)
        else:
            X = rng.normal(size=(n_rows, P_DENSE)).astype(T).astype(np.float64)
        return X, X
    if kind == "snp":
        calls = rng.randint(0, 3, size=(n_rows, P_DENSE)).astype(np.int8)
        miss = rng.uniform(size=calls.shape) < 0.1
        calls[miss] = -9
        calls[:, SNP_ALL_MISSING] = -9
        calls[:, SNP_ALL_ZERO] = 0
        if leg == "exact":   # dyadic imputed values: multiples of 1/2 in [0, 2], so that w x x stays a multiple of 1/8
            impute = rng.randint(0, 5, size=P_DENSE) * 0.5
            calls[:, ::2] = np.where(calls[:, ::2] < 0, 1, calls[:, ::2])   # every other column without missing calls
            calls[:, SNP_ALL_MISSING] = -9
        else:                # the means of the calls that are there (0 for the column without any)
            valid = calls >= 0
            impute = np.where(valid, calls, 0).sum(axis=0) / np.maximum(valid.sum(axis=0), 1)
        impute = impute.astype(T).astype(np.float64)
        X = np.where(calls >= 0, calls, 0).astype(np.float64) + (calls < 0) * impute[None, :]
        return X, (np.asfortranarray(calls), impute)
    assert kind == "csc"
    dens = 0.3 if n_rows <= 2000 else 0.01
    mask = rng.uniform(size=(n_rows, P_CSC)) < dens
    mask[:, CSC_EMPTY] = False
    mask[:, CSC_FULL] = True
    if leg == "exact":
        V = rng.randint(1, 4, size=mask.shape) * rng.choice([-1.0, 1.0], size=mask.shape)
    else:
        V = rng.normal(size=mask.shape).astype(T).astype(np.float64)
        V[V == 0] = 1.0
    X = np.where(mask, V, 0.0)
    return X, X


def make_vectors(case, leg, X_used):
    """w (n,) and xm (p,), float64 values representable in the case's type.  X_used: the rows the build sees."""
    rng = _rng(case.name + leg)
    T = NP_TYPE[case.dtype]
    n, p = X_used.shape
    if leg == "exact":
        w = rng.choice([0.0, 0.5, 1.0, 2.0], size=n)
        xm = rng.randint(-16, 17, size=p) * 0.25
    else:
        w = rng.uniform(size=n)
        w[rng.uniform(size=n) < 0.2] = 0.0
        if w.sum() == 0:
            w[0] = 1.0
        w = (w / w.sum()).astype(T).astype(np.float64)
        xm = ((X_used * w[:, None]).sum(axis=0) / w.sum()).astype(T).astype(np.float64)
    return w, xm


def prefill(case, which):
    size = case.out0 if which == 0 else case.out1
    return np.full(size, NAN_BITS[case.dtype], dtype=BITS[case.dtype]).view(NP_TYPE[case.dtype])


# ---- reference -------------------------------------------------------------------------------------------------------------
def block_reference(case, blk, X_used, w, xm, extended):
    """(values, abs-sum, |xm xm|) of one block, rows x cols.  extended: accumulate in long double (the rounding leg)."""
    A = X_used[:, blk.rows]
    B = X_used[:, blk.cols] * w[:, None]           # exact in the exact leg; the rounding leg's reference redoes it below
    S = np.abs(A).T @ np.abs(B)
    Q = np.abs(np.outer(xm[blk.rows], xm[blk.cols]))
    if extended:
        assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the reference needs an extended-precision long double"
        Al = np.ascontiguousarray(A.T.astype(np.longdouble))
        Bl = X_used[:, blk.cols].astype(np.longdouble) * w.astype(np.longdouble)[:, None]
        G = Al @ Bl
        if case.center:
            G = G - np.outer(xm[blk.rows].astype(np.longdouble), xm[blk.cols].astype(np.longdouble))
    else:
        G = A.T @ B
        if case.center:
            G = G - np.outer(xm[blk.rows], xm[blk.cols])
        G = G + 0.0
    if not case.center:
        Q = np.zeros_like(Q)
    return G, S, Q


def block_index(case, blk):
    """Flat indices of the block's entries (rows x cols) and of their mirror images."""
    a = np.arange(len(blk.rows))[:, None] + blk.rpos0
    b = np.arange(len(blk.cols))[None, :] + blk.cpos0
    return blk.dst + a + b * case.ldc, blk.dst + b + a * case.ldc


def exact_headroom(case, X_used, w, xm):
    """16 max_ab (sum_i |w_i x_ia x_ib| + |xm_a xm_b|) over the case's blocks, checked to be a whole number of sixteenths."""
    worst = 0.0
    for blk in case.blocks:
        _, S, Q = block_reference(case, blk, X_used, w, xm, False)
        H = (S + Q) * 16.0
        assert (H == np.round(H)).all(), case.name
        worst = max(worst, float(H.max()))
    return worst


def expected(case, X_used, w, xm, leg):
    """Per output buffer: (reference values as float64 / long double, bound, footprint mask), flat."""
    out = []
    for which, size in ((0, case.out0), (1, case.out1)):
        ref = np.zeros(size, dtype=np.longdouble if leg == "rounding" else np.float64)
        bound = np.zeros(size)
        foot = np.zeros(size, dtype=bool)
        out.append((ref, bound, foot))
    u = UNIT[case.dtype]
    for blk in case.blocks:
        G, S, Q = block_reference(case, blk, X_used, w, xm, leg == "rounding")
        bnd = (case.n + 4) * u * S + 2 * u * Q
        ref, bound, foot = out[blk.buf]
        idx, midx = block_index(case, blk)
        if blk.mirror:
            ref[midx] = G
            bound[midx] = bnd
            foot[midx] = True
        ref[idx] = G
        bound[idx] = bnd
        foot[idx] = True
    return out


def mirror_pairs(case):
    """(buffer, flat index, flat index of the mirror image) of every block written symmetrically."""
    out = []
    for blk in case.blocks:
        if blk.mirror:
            idx, midx = block_index(case, blk)
            out.append((blk.buf, idx.ravel(), midx.ravel()))
    return out


def check_info(case, info):
    got = dict(zip(INFO, (int(v) for v in info)))
    for key, want in case.expect.items():
        if isinstance(want, tuple):
            assert want[0] <= got[key] <= want[1], (case.name, key, got)
        else:
            assert got[key] == want, (case.name, key, got)
    if got["launcher"] in (L_SYRK, L_SYRK_BATCH, L_GRAM, L_GRAM_BATCH, L_STRIP):
        ns, kc = got["nsplit"], got["kchunk"]
        assert ns >= 1 and (ns - 1) * kc < case.n <= ns * kc, (case.name, got)
    return got


# ---- the case table --------------------------------------------------------------------------------------------------------
def _pick(rng, count, p, avoid=()):
    """`count` distinct columns in random (unsorted) order."""
    pool = np.setdiff1d(np.arange(p), np.asarray(avoid, dtype=np.int64))
    return rng.permutation(pool)[:count].astype(np.int32)


def _variant(kind, dtype, row_off):
    return 1 if (kind != "dense" or row_off == 0) else 0


def _p(kind):
    return P_CSC if kind == "csc" else P_DENSE


def _special_first(kind, cols):
    """Puts the design's special columns in front of a list (an empty and a full csc column; the all-missing / all-zero 2-bit ones)."""
    sp = {"csc": (CSC_EMPTY, CSC_FULL), "snp": (SNP_ALL_MISSING, SNP_ALL_ZERO), "dense": ()}[kind]
    sp = [c for c in sp][: len(cols)]
    rest = [c for c in cols if c not in sp]
    return np.array(sp + rest, dtype=np.int32)[: len(cols)]


def syrk_case(kind, dtype, n, M, row_off=0, center=True, nsplit=None):
    name = "syrk-%s-%s-n%d-M%d%s" % (kind, dtype, n, M, "-scalar" if row_off else "")
    rng = _rng(name)
    p = _p(kind)
    lead = _pick(rng, 5, p)
    if kind == "csc" and M >= 6:   # the same column twice in the list
        cols = _special_first(kind, _pick(rng, M - 1, p))
        cols = np.concatenate([cols, cols[1:2]]).astype(np.int32)
    else:
        cols = _special_first(kind, _pick(rng, M, p)) if M >= 2 else _pick(rng, M, p)
    allc = np.concatenate([lead, cols]).astype(np.int32)
    ldc, dst = 128, 5 + 3 * 128
    out0 = dst + (M - 1) * (ldc + 1) + 1 + 7
    cidx = np.arange(5, 5 + M)
    blocks = [Block(0, dst, allc[cidx], allc[cidx], 0, 0, True)]
    if kind == "csc":
        expect = {"launcher": L_BLOCK_CSC, "tile": M}
        if n >= N_CSC_TWO_BLOCKS:
            expect["csc_row_blocks"] = (2, 64)
    else:
        expect = {"launcher": L_SYRK, "tile": 32 if M <= 32 else (64 if M <= 64 else 128), "vec16": _variant(kind, dtype, row_off)}
        if nsplit is not None:
            expect["nsplit"] = nsplit
    return Case(name, kind, dtype, MODE_SYRK, n, row_off, allc, [(5, M, dst)], center, ldc, 0, out0, 0, expect, blocks)


def syrk_batch_case(kind, dtype, n, nbs, row_off=0, center=True, nsplit=None, tag=""):
    name = "syrkb-%s-%s-n%d-c%d-mx%d%s%s" % (kind, dtype, n, len(nbs), max(nbs), tag, "-scalar" if row_off else "")
    rng = _rng(name)
    p = _p(kind)
    lists, table, blocks, off = [], [], [], 0
    for y, nb in enumerate(nbs):
        cols = _pick(rng, nb, p)
        if y == 0:
            cols = _special_first(kind, cols) if nb >= 2 else cols
        if y == 1:                         # a column that appears in two blocks
            cols[0] = lists[0][-1]
        if kind == "csc" and y == 2 and nb >= 2:   # the same column twice in one list
            cols[-1] = cols[0]
        lists.append(cols)
        dst = y * SLOT + (y % 3)           # (into a pool of 128 x 128 slots, leading dimension 128)
        if (nb - 1) * 129 + (y % 3) >= SLOT:
            dst = y * SLOT
        table.append((off, nb, dst))
        blocks.append(Block(0, dst, cols, cols, 0, 0, True))
        off += nb
    allc = np.concatenate(lists).astype(np.int32)
    mx = max(nbs)
    if kind == "csc":
        expect = {"launcher": L_BLOCK_CSC, "tile": mx}
    else:
        expect = {"launcher": L_SYRK_BATCH, "tile": 32 if mx <= 32 else (64 if mx <= 64 else 128),
                  "vec16": _variant(kind, dtype, row_off)}
        if nsplit is not None:
            expect["nsplit"] = nsplit
    return Case(name, kind, dtype, MODE_SYRK_BATCH, n, row_off, allc, table, center, 128, 0, len(nbs) * SLOT, 0, expect, blocks)


def gram_case(kind, dtype, n, M, N, route, row_off=0, center=True, nsplit=None):
    """route 'sym': ncols is the tail of mcols at the same positions (m_pos0 = 3); 'gen': two distinct lists, m_pos0 = 2,
    n_pos0 = 1; 'panel' (csc): ncols a middle slice of mcols at the same positions; 'apart' (csc): two distinct lists whose
    position ranges do not meet."""
    name = "gram-%s-%s-n%d-M%d-N%d-%s%s%s" % (kind, dtype, n, M, N, route, "" if center else "-raw", "-scalar" if row_off else "")
    rng = _rng(name)
    p = _p(kind)
    if route == "sym":
        assert N <= M
        mcols = _pick(rng, M, p) if M <= p else rng.randint(0, p, size=M).astype(np.int32)
        if M >= 2:
            mcols = _special_first(kind, mcols) if M <= p else mcols
        allc, moff, noff, m_pos0 = mcols, 0, M - N, 3
        n_pos0 = m_pos0 + M - N
        symmetric = 1
    elif route == "panel":
        assert N < M
        mcols = rng.randint(0, p, size=M).astype(np.int32)
        allc, moff, m_pos0 = mcols, 0, 0
        noff = n_pos0 = (M - N) // 2
        symmetric = 0
    else:
        mcols = _pick(rng, M, p) if M <= p else rng.randint(0, p, size=M).astype(np.int32)
        ncols = _pick(rng, N, p) if N <= p else rng.randint(0, p, size=N).astype(np.int32)
        if kind == "csc" and N >= 2:
            ncols[-1] = ncols[0]
        allc, moff, noff = np.concatenate([mcols, ncols]).astype(np.int32), 0, M
        m_pos0, n_pos0 = (2, 1) if route == "gen" else (0, M + 1)
        symmetric = 0
    side = max(m_pos0 + M, n_pos0 + N)
    ldc = side + 3
    out0 = side * ldc
    mirror = bool(symmetric) or kind == "csc"
    blocks = [Block(0, 0, allc[moff:moff + M], allc[noff:noff + N], m_pos0, n_pos0, mirror)]
    if kind == "csc":
        expect = {"launcher": L_GRAM_CSC}
        if n >= N_CSC_TWO_BLOCKS:
            expect["csc_row_blocks"] = (2, 64)
    else:
        rem = N % 128
        n128 = N // 128 + (1 if rem > 64 else 0)
        n64 = 1 if 0 < rem <= 64 else 0
        expect = {"launcher": L_GRAM, "symmetric": symmetric, "n128": n128, "n64": n64, "tile": (M + 127) // 128,
                  "vec16": _variant(kind, dtype, row_off)}
        if nsplit is not None:
            expect["nsplit"] = nsplit
    return Case(name, kind, dtype, MODE_GRAM, n, row_off, allc, [(moff, M, m_pos0, noff, N, n_pos0)], center, ldc, 0, out0, 0,
                expect, blocks)


def gram_batch_case(kind, dtype, n, shapes, row_off=0, center=True, nsplit=None):
    name = "gramb-%s-%s-n%d-c%d%s" % (kind, dtype, n, len(shapes), "-scalar" if row_off else "")
    rng = _rng(name)
    lists, table, blocks, off = [], [], [], 0
    for y, (m, nn) in enumerate(shapes):
        rows = _pick(rng, m, P_DENSE)
        cols = _pick(rng, nn, P_DENSE)
        if y == 0 and kind == "snp" and m >= 2:
            rows = _special_first(kind, rows)
        dst = y * SLOT
        table.append((off, m, off + m, nn, dst))
        blocks.append(Block(0, dst, rows, cols, 0, 0, False))
        lists += [rows, cols]
        off += m + nn
    allc = np.concatenate(lists).astype(np.int32)
    expect = {"launcher": L_GRAM_BATCH, "tile": 128, "vec16": _variant(kind, dtype, row_off)}
    if nsplit is not None:
        expect["nsplit"] = nsplit
    return Case(name, kind, dtype, MODE_GRAM_BATCH, n, row_off, allc, table, center, 128, 0, len(shapes) * SLOT, 0, expect, blocks)


def strip_case(dtype, n, strips, form="lt", center=True, nsplit=None, tag=""):
    """strips: (m, row0, c0n) each; c1n = row0 + m.  form: 'lt' (f64: strip_lt_kernel; f32: the one kernel there is), 'plain'
    (f64 strip_kernel by the flag), 'scalar' (a row offset of one element: the scalar-load variant)."""
    name = "strip-%s-%s-n%d-%s%s" % (dtype, form, n, "+".join("%d.%d.%d" % s for s in strips), tag)
    rng = _rng(name)
    row_off = 1 if form == "scalar" else 0
    lists, table, blocks, off = [], [], [], 0
    mx = 0
    for y, (m, row0, c0n) in enumerate(strips):
        c1n = row0 + m
        assert 1 <= m <= 64 and c1n <= 128 and c0n <= 128
        both = _pick(rng, c0n + c1n, P_DENSE)
        c0, c1 = both[:c0n], both[c0n:]
        v = c1[row0:]
        c0off, c1off = off, off + c0n
        dstD = y * SLOT
        dstX = y * SLOT
        table.append((c1off + row0, m, c0off, c0n, c1off, c1n, row0, dstX, dstD))
        blocks.append(Block(0, dstD, v, c1, row0, 0, True))
        if c0n:
            blocks.append(Block(1, dstX, v, c0, row0, 0, False))
        lists.append(both)
        off += c0n + c1n
        mx = max(mx, m)
    allc = np.concatenate(lists).astype(np.int32)
    lt = 1 if (dtype == "f64" and form == "lt") else 0
    expect = {"launcher": L_STRIP, "tile": (mx + 15) // 16, "strip_lt": lt, "vec16": 0 if form == "scalar" else 1}
    if nsplit is not None:
        expect["nsplit"] = nsplit
    return Case(name, "dense", dtype, MODE_STRIP, n, row_off, allc, table, center, 128, 1 if form == "plain" else 0,
                len(strips) * SLOT, len(strips) * SLOT, expect, blocks)


ONE = (1, 1)        # nsplit of a launch whose rows fit one K-split
SOME = (2, 64)
MANY = (65, 1 << 20)


def build_cases():
    c = []
    # ---- single diagonal blocks ---------------------------------------------------------------------------------------------
    for i, M in enumerate((1, 16, 17, 32, 33, 48, 64, 65, 100, 127, 128)):
        c.append(syrk_case("dense", "f64", 1000, M, center=bool(i % 2 == 0), nsplit=SOME))
    for n, ns in ((1, ONE), (31, ONE), (256, ONE), (257, (2, 2))):
        c.append(syrk_case("dense", "f64", n, 33, nsplit=ns))
        c.append(syrk_case("dense", "f64", n, 100, nsplit=ns))
    c.append(syrk_case("dense", "f64", 8320, 65, nsplit=(13, 64)))       # the reduce's loop unrolled over 16 splits
    for n, M in ((1000, 17), (1000, 64), (1000, 128), (257, 33), (8320, 100)):
        c.append(syrk_case("dense", "f32", n, M))
    for dtype, M in (("f64", 32), ("f64", 48), ("f64", 65), ("f32", 17), ("f32", 48), ("f32", 128)):
        c.append(syrk_case("dense", dtype, 1000, M, row_off=1))
    c.append(syrk_case("dense", "f64", 257, 127, row_off=1, nsplit=(2, 2)))
    for n in (255, 257, 1000):                                           # n = 3, 1, 0 (mod 4): the 2-bit packing
        for M in (17, 64, 100):
            c.append(syrk_case("snp", "f64", n, M))
    for n in (1, 31, 256, 8320):
        c.append(syrk_case("snp", "f64", n, 64))
    c.append(syrk_case("snp", "f64", 254, 33))                           # n = 2 (mod 4)
    for n, M in ((1000, 64), (257, 33), (255, 128), (257, 17)):
        c.append(syrk_case("snp", "f32", n, M))
    for dtype in ("f64", "f32"):
        c.append(syrk_case("csc", dtype, 1000, 12))
    c.append(syrk_case("csc", "f64", N_CSC_TWO_BLOCKS, 10))              # a design of two row blocks
    # ---- batches of diagonal blocks -----------------------------------------------------------------------------------------
    mix128 = (128, 1, 17, 64, 33, 100, 16, 65)
    mix64 = (64, 1, 16, 17, 32, 33, 48, 5, 64, 2, 31, 49, 63, 20, 40, 8)
    mix32 = (32, 1, 16, 17, 5, 31, 2, 9)
    for n, ns in ((1, ONE), (31, ONE), (256, ONE), (257, (2, 2)), (1000, SOME)):
        c.append(syrk_batch_case("dense", "f64", n, mix128, nsplit=ns))
    c.append(syrk_batch_case("dense", "f64", 1000, mix64, center=False))
    c.append(syrk_batch_case("dense", "f64", 1000, mix32))
    c.append(syrk_batch_case("dense", "f64", 1000, (32,)))
    c.append(syrk_batch_case("dense", "f64", 8320, (127,), nsplit=(13, 64)))
    c.append(syrk_batch_case("dense", "f32", 1000, mix128))
    c.append(syrk_batch_case("dense", "f32", 257, mix64))
    c.append(syrk_batch_case("dense", "f32", 31, (17,)))
    c.append(syrk_batch_case("dense", "f64", 1000, mix128, row_off=1))
    c.append(syrk_batch_case("dense", "f64", 257, mix32, row_off=1))
    c.append(syrk_batch_case("dense", "f64", 1000, mix64, row_off=1))
    c.append(syrk_batch_case("dense", "f32", 1000, mix64, row_off=1))
    c.append(syrk_batch_case("dense", "f32", 257, mix128, row_off=1))
    c.append(syrk_batch_case("dense", "f32", 257, mix32, row_off=1))
    for n in (255, 257, 1000):
        c.append(syrk_batch_case("snp", "f64", n, mix128))
    for n in (1, 254, 1000):
        c.append(syrk_batch_case("snp", "f64", n, mix64))
    c.append(syrk_batch_case("snp", "f64", 257, mix32))
    c.append(syrk_batch_case("snp", "f32", 1000, mix64))
    c.append(syrk_batch_case("snp", "f32", 255, mix128))
    for dtype in ("f64", "f32"):
        c.append(syrk_batch_case("csc", dtype, 1000, (12, 1, 7, 20, 5, 3, 9, 24)))
    c.append(syrk_batch_case("csc", "f64", 1000, (9,)))
    c.append(syrk_batch_case("csc", "f64", N_CSC_TWO_BLOCKS, (8, 3)))
    # ---- the general Gram -------------------------------------------------------------------------------------------------
    sym = ((1, 1), (127, 64), (128, 128), (129, 65), (300, 200), (300, 129), (300, 192), (128, 1), (129, 128))
    gen = ((1, 200), (127, 65), (129, 128), (300, 64), (128, 192), (300, 129), (1, 1), (127, 1))
    for i, (M, N) in enumerate(sym):
        c.append(gram_case("dense", "f64", 1000, M, N, "sym", center=bool(i % 2 == 0), nsplit=SOME))
    for i, (M, N) in enumerate(gen):
        c.append(gram_case("dense", "f64", 1000, M, N, "gen", center=bool(i % 2 == 1), nsplit=SOME))
    c.append(gram_case("dense", "f64", 1000, 300, 64, "panel"))   # a middle slice of the row list: positions shared, not symmetric
    for n, ns in ((1, ONE), (31, ONE), (256, ONE), (257, (2, 2))):
        c.append(gram_case("dense", "f64", n, 129, 65, "sym", nsplit=ns))
        c.append(gram_case("dense", "f64", n, 127, 65, "gen", nsplit=ns))
    c.append(gram_case("dense", "f64", 8320, 129, 65, "sym", nsplit=(13, 1 << 20)))
    for M, N, route in ((300, 200, "sym"), (129, 65, "sym"), (127, 64, "gen"), (300, 129, "gen")):
        c.append(gram_case("dense", "f32", 1000, M, N, route))
    c.append(gram_case("dense", "f32", 257, 128, 128, "sym"))
    for dtype in ("f64", "f32"):
        c.append(gram_case("dense", dtype, 1000, 300, 200, "sym", row_off=1))
        c.append(gram_case("dense", dtype, 257, 127, 65, "gen", row_off=1))
    for n in (255, 257, 1000):
        c.append(gram_case("snp", "f64", n, 129, 65, "sym"))
        c.append(gram_case("snp", "f64", n, 127, 192, "gen"))
    c.append(gram_case("snp", "f64", 1000, 300, 200, "sym", center=False))
    c.append(gram_case("snp", "f64", 31, 128, 1, "sym"))
    c.append(gram_case("snp", "f32", 1000, 300, 129, "gen"))
    c.append(gram_case("snp", "f32", 254, 129, 128, "sym"))
    for dtype in ("f64", "f32"):
        c.append(gram_case("csc", dtype, 1000, 20, 9, "sym"))
        c.append(gram_case("csc", dtype, 1000, 30, 11, "panel", center=False))
        c.append(gram_case("csc", dtype, 1000, 7, 17, "apart"))
    c.append(gram_case("csc", "f64", 257, 24, 24, "sym"))
    c.append(gram_case("csc", "f64", N_CSC_TWO_BLOCKS, 10, 4, "sym"))
    # ---- batches of cross blocks --------------------------------------------------------------------------------------------
    three = ((128, 128), (1, 33), (17, 1))
    sixteen = tuple((m, nn) for m in (1, 16, 17, 128) for nn in (1, 33, 128)) + ((16, 128), (128, 1), (17, 33), (1, 1))
    for n, ns in ((1, ONE), (31, ONE), (256, ONE), (257, (2, 2)), (1000, SOME)):
        c.append(gram_batch_case("dense", "f64", n, three, nsplit=ns))
    c.append(gram_batch_case("dense", "f64", 1000, sixteen, center=False))
    c.append(gram_batch_case("dense", "f64", 1000, ((16, 33),)))
    c.append(gram_batch_case("dense", "f64", 8320, ((17, 128),), nsplit=(13, 64)))
    c.append(gram_batch_case("dense", "f32", 1000, sixteen))
    c.append(gram_batch_case("dense", "f32", 257, three))
    c.append(gram_batch_case("dense", "f64", 1000, sixteen, row_off=1))
    c.append(gram_batch_case("dense", "f32", 257, three, row_off=1))
    for n in (255, 257, 1000):
        c.append(gram_batch_case("snp", "f64", n, three))
    c.append(gram_batch_case("snp", "f64", 1000, sixteen))
    c.append(gram_batch_case("snp", "f32", 254, sixteen))
    # ---- strips: (m, row0, c0n) -----------------------------------------------------------------------------------------------
    singles = ((1, 0, 0), (1, 127, 128), (16, 0, 1), (17, 1, 128), (32, 64, 0), (33, 64, 128), (48, 64, 1), (49, 1, 0),
               (64, 64, 128), (64, 0, 1), (16, 64, 128), (48, 1, 128))
    few = ((16, 0, 1), (17, 1, 128), (48, 64, 1), (64, 64, 128), (1, 127, 128), (49, 1, 0))
    mixed8 = ((1, 0, 0), (16, 64, 128), (17, 1, 1), (32, 0, 128), (33, 64, 0), (48, 1, 128), (49, 64, 1), (64, 64, 128))
    small8 = ((1, 127, 128), (16, 0, 0), (5, 64, 1), (16, 1, 128), (9, 0, 1), (2, 64, 128), (16, 64, 0), (3, 1, 1))
    for i, st in enumerate(singles):
        c.append(strip_case("f64", 1000, (st,), "lt", center=bool(i % 3 != 1), nsplit=SOME))
    for form, dtype in (("plain", "f64"), ("scalar", "f64"), ("lt", "f32"), ("scalar", "f32")):
        for st in few:
            c.append(strip_case(dtype, 1000, (st,), form))
    for form, dtype in (("lt", "f64"), ("plain", "f64"), ("scalar", "f64"), ("lt", "f32"), ("scalar", "f32")):
        c.append(strip_case(dtype, 1000, mixed8, form, tag="-mixed"))
        c.append(strip_case(dtype, 257, small8, form, tag="-small"))
        for n, ns in ((1, ONE), (31, ONE), (256, (1, 2)), (257, (2, 3)), (8320, MANY)):
            c.append(strip_case(dtype, n, ((17, 1, 128),), form, nsplit=ns))
    c.append(strip_case("f64", 8320, ((64, 64, 128),), "lt", nsplit=MANY))
    c.append(strip_case("f32", 8320, ((64, 64, 128),), "lt", nsplit=MANY))
    names = [k.name for k in c]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return c


CASES = build_cases()
CASE_BY_NAME = {k.name: k for k in CASES}


def variant_of(case):
    """What the case's info assertion names, as text (profiles/block_builds.txt lists case -> variant)."""
    return " ".join("%s=%s" % (k, ("%d..%d" % v) if isinstance(v, tuple) else v) for k, v in case.expect.items())
