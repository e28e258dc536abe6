"""The device pieces of the group engine, one launch at a time, against plain longdouble references (no GPU needed to import).

A *call* is one ``adelie_hip_group_piece_test``: mode EIG (launch_grp_eig), ROTATE (launch_grp_block_rotate), LAYOUT
(launch_grp_layout), PANEL_SOLVE (launch_cd_group_panel_solve with rot = 1, block by block) or GRAM_PASS
(launch_cd_group_block_pass).  This module holds the case tables, the inputs, the references and the derivation of every bound;
``device_call`` runs a call on the device, ``emulate_call`` in plain numpy in the target dtype (optionally with a planted
defect).  tests/test_gpu_group_pieces.py runs the cases on the device, tests/test_group_checks_host.py runs the same checkers on
the emulation and on planted defects.  Every reference is computed in ``np.longdouble`` from the arrays actually handed to the
call; float32 inputs are promoted exactly.  u = 2^-53 / 2^-24 is the unit roundoff, gamma_k = k u / (1 - k u).

EIG.  Per group: the pre-fill of vars and V (a NaN payload) is untouched outside the group's footprint, vars ascending, and three
scale-free figures: the orthogonality defect max |V^T V - I|, the residual max |A V - V diag(lambda)| / ||A||_F over the columns
whose reference eigenvalue is positive, and the eigenvalue error max |lambda - max(eigvalsh(A), 0)| / ||A||_F.  Each is bounded by
8 x the largest of: the same figure of the CPU checker's cyclic Jacobi (same rotation order and formulas as the kernel), the
same figure of numpy.linalg.eigh, and q 2^-52.  The margin of 8 covers the lane-parallel application of each rotation.  float32
outputs are the double results rounded once: + 2.1 2^-24 on the defect (unit columns, Cauchy-Schwarz: 2 u + u^2 per inner
product), + 2^-24 max|lambda| / ||A||_F on the eigenvalues, + 2^-24 ||A||_2 sqrt(q) / ||A||_F on the residual.

ROTATE.  Exact leg: D and V hold small integers (V block-diagonal, not orthogonal, D not symmetric), every product and partial
sum is an integer below 2^24: the result is asserted bit for bit.  Rounding leg: D a random positive semi-definite block, V
from numpy.linalg.eigh; entry (r, c) is two successive fma dot products of lengths q_c and q_r, q = max(q_r, q_c), so
|err| <= (2 gamma_q + gamma_q^2) (|R|^T |D| |R|)_rc; entries whose row and column groups both have q = 1 are copied bit for bit.
Footprint: in place nothing outside the leading nval x nval changes; with Dsrc != Dptr every such entry keeps the pre-fill,
except that the narrow route's paired store may leave Dsrc's entry in row nval of the first nval columns when nval is odd.
Symmetry of the result is NOT asserted: the two passes round differently and the solves read only below the diagonal.

LAYOUT.  All GDESC_STRIDE words against a numpy construction, except the unnamed gaps between the tables (GAPS below).

PANEL_SOLVE / GRAM_PASS.  Per visit, with no error carried along the block: for group k of a block (values o .. o + q, penalty
p, l1p = l1 p, l2p = l2 p, eigenpairs Lambda, V_k) form, in longdouble and from the kernel's OWN outputs for the values visited
before it (delta_m = beta_new - beta0),

    u = V_k^T (g_k - sum_{m<k} D[k, m] delta_m) + Lambda o (V_k^T beta0_k)

(GRAM_PASS: C in place of D, every value visited earlier in the pass).  If ||u|| + slack < l1p the new coefficients must be
exact zeros, whatever beta0 was.  Otherwise, with bt = V_k^T beta_new_k, b = Lambda + l2p,

    || u - b o bt - l1p bt / ||bt|| ||_2  <=  l1p newton_tol + ||e_u||_2 + gamma_{q+4} (||b o bt|| + l1p) + max(b) gamma_q ||bt|| + e_V

Derivation.  The kernel stops at |f(h)| <= newton_tol, f(h) = sum_i v_i^2 / (b_i h + l1p)^2 - 1, and returns x_i = h v_i /
(b_i h + l1p): then ||x|| / h = sqrt(1 + f) and v - b o x - l1p x / ||x|| = l1p x (1 / h - 1 / ||x||), of norm l1p |sqrt(1 + f)
- 1| <= l1p newton_tol: the first term.  e_u = gamma_{nval+q} (|V_k|^T (|g_k| + sum |D[k, m]| |delta_m|) + Lambda o |V_k|^T
|beta0_k|) (+ u |V_k|^T |D[k, m]| |V_m| |V_m^T delta_m| in PANEL_SOLVE, whose block was rounded to the dtype after the rotation; the
chained case, whose block is the device's own rotation, has ROTATE's 2 gamma_q + gamma_q^2 on top of that u) is the
rounding of the gradient the kernel carried: dot products of length q for the rotations and at most nval fused accumulations.
gamma_{q+4} covers the evaluation of x and of the two reductions, max(b) gamma_q ||bt|| the back rotation beta_new = V_k x.
e_V accounts for eigenbases that are orthogonal only up to E_m = V_m^T V_m - I (numpy's, rounded to the dtype): the kernel's
rotated change of an earlier group is x_m - V_m^T beta0_m while the check sees V_k^T D delta_m with delta_m = V_m x_m - beta0_m, a
difference of ||V_k^T D[k, m]|| ||E_m|| ||beta0_m||, and bt = (I + E_k) x:
e_V = sum_{m<k} ||D[k, m]||_F ||E_m||_F ||beta0_m|| + ||E_k||_F (max(b) ||bt|| + 2 l1p + max(Lambda) ||beta0_k||).
The state: rsq, resid_sum and cm against their longdouble sums over the changed groups, within gamma_{N+8} of the sum of the
absolute terms (N the values of the blocks so far) plus the first-order effect of e_u and of the difference e_d between the
kernel's rotated change and V_k^T delta_k, ||e_d|| <= (||E_k||_F + q gamma_q) (||bt|| + ||V_k^T beta0_k||).
GRAM_PASS: final g = g_in - C delta within gamma_{nz+2} |C| |delta| + nblk u (|g_in| + |C| |delta|) (one rounded subtraction per block).
The above-threshold leg is asserted in float64 for all widths and in float32 for widths up to 16 (newton_tol is 1e-5 there by
design and the wider paths sum without fma); the zero leg and the bit-for-bit bookkeeping in both dtypes for all widths.
"""
import ctypes as C
import zlib
from collections import namedtuple

import numpy as np

LD = np.longdouble
G = 128
SLOT = G * G
MODE_EIG, MODE_ROTATE, MODE_LAYOUT, MODE_PANEL, MODE_GRAM = range(5)
CD_OK, CD_MAX_ACTIVE, CD_NEWTON = 0, 2, 3
GD = dict(VMAP=0, VGRP=128, VSS=256, GOFF=384, GQ=520, GSS=648, NG=776, NVAL=777, VOFF=784, VPOS=912, VQ=1040, STRIDE=1168)
# words of a descriptor no table names: behind goff's 129 entries, and behind NG / NVAL
GAPS = list(range(GD["GOFF"] + 129, GD["GQ"])) + list(range(GD["NVAL"] + 1, GD["VOFF"]))
NP_TYPE = {"f64": np.float64, "f32": np.float32}
DT_CODE = {"f64": 1, "f32": 0}
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NAN_BITS = {"f64": np.uint64(0x7FF8DEAD0000BEEF), "f32": np.uint32(0x7FC0BEEF)}
BITS = {"f64": np.uint64, "f32": np.uint32}
NEWTON_TOL = {"f64": 1e-12, "f32": 1e-5}
EIG_MAX_Q = 96
ROT_QM = 16


def gamma(k, u):
    return k * u / (1 - k * u)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def prefill(dtype, n):
    return np.full(n, NAN_BITS[dtype], dtype=BITS[dtype]).view(NP_TYPE[dtype])


def bits(a):
    return a.view(BITS["f64" if a.dtype == np.float64 else "f32"])


def is_prefill(a):
    return bits(a) == NAN_BITS["f64" if a.dtype == np.float64 else "f32"]


def width_class(q):
    return "q1" if q == 1 else "q2-16" if q <= 16 else "q17-64" if q <= 64 else "q65-128"


# ---- the call ---------------------------------------------------------------------------------------------------------------
POINTERS = ("eig", "src", "vars", "V", "goff", "rvoff", "D", "Dsrc", "sbegin", "ssize", "voff", "blk_g0", "list", "desc", "Dblk",
            "gblk", "C", "xmean", "spen", "vcol", "beta", "g", "is_active", "active_set", "dcol", "dlt", "dd", "st_f", "st_i")
ARRAY_TYPE = dict(eig=np.int64, goff=np.int32, rvoff=np.int64, sbegin=np.int32, ssize=np.int32, voff=np.int64, blk_g0=np.int32,
                  list=np.int32, desc=np.int32, vcol=np.int32, is_active=np.int8, active_set=np.int32, dcol=np.int32, st_f=np.float64,
                  st_i=np.int64)


def device_call(hip, mode, dtype, a):
    """Runs one call on the device.  `a`: field name -> contiguous numpy array (written in place where the mode writes) or
    scalar.  Returns info."""
    from adelie_amd import _abi

    s = _abi.GroupPiece()
    s.dtype, s.mode = DT_CODE[dtype], mode
    for k, v in a.items():
        if k in POINTERS:
            if v is None:
                continue
            want = ARRAY_TYPE.get(k, NP_TYPE[dtype])
            assert v.dtype == want and v.flags.c_contiguous, k
            setattr(s, k, v.ctypes.data)
        else:
            setattr(s, k, v)
    for k in ("src", "vars", "V"):
        if a.get(k) is not None:
            setattr(s, k + "_elems", a[k].size)
    info = np.full(4, -1, dtype=np.int64)
    hip.check(hip.fn("group_piece_test")(C.byref(s), info.ctypes.data))
    return info


# ---- EIG --------------------------------------------------------------------------------------------------------------------
# groups: (q, kind, scale); place: 'tight' (ld = q + 3, blocks one behind the other) or 'slot' (ld = 128, inside 128 x 128 slots)
EigCase = namedtuple("EigCase", "name groups place max_q")


def _eig_cases():
    out = []
    for q in (2, 3, 16, 17, 63, 64, 65, 96):
        out.append(EigCase("gram-q%d" % q, [(q, "gram", 1.0)], "tight", q))
    out.append(EigCase("mixed-1-5-96", [(1, "gram", 1.0), (5, "gram", 1.0), (96, "gram", 1.0)], "tight", 96))
    out.append(EigCase("slot-ld128", [(7, "gram", 1.0), (1, "gram", 1.0), (33, "gram", 1.0), (1, "indef", 1.0)], "slot", 33))
    out.append(EigCase("kinds-q12", [(12, k, 1.0) for k in ("diag", "dup", "cluster", "zeros", "indef")], "tight", 12))
    out.append(EigCase("scaled-q12", [(12, "gram", 1e-6), (12, "gram", 1.0), (12, "gram", 1e6)], "tight", 20))
    return out


EIG_CASES = _eig_cases()


def eig_block(rng, q, kind, scale, T):
    """A symmetric (q, q) block of the kind, representable in T, as float64."""
    n = max(3 * q, 40)
    X = rng.normal(size=(n, q))
    w = rng.uniform(0.5, 1.5, size=n)
    A = (X * w[:, None]).T @ X / n
    if kind == "diag":
        A = np.diag(np.diag(A))
    elif kind == "dup" and q > 3:
        X[:, q - 1] = X[:, 0]
        X[:, q - 2] = X[:, 1]
        A = (X * w[:, None]).T @ X / n
    elif kind == "cluster":
        Q, _ = np.linalg.qr(rng.normal(size=(q, q)))
        A = (Q * (1.0 + 1e-9 * np.arange(q))) @ Q.T
    elif kind == "zeros" and q > 3:
        h = q // 2
        A[:h, h:] = 0
        A[h:, :h] = 0
    elif kind == "indef":
        A = A - np.mean(np.diag(A)) * np.eye(q)
    A = (A + A.T) / 2 * scale
    A = A.astype(T).astype(np.float64)
    return np.triu(A) + np.triu(A, 1).T


def eig_inputs(case, dtype):
    T = NP_TYPE[dtype]
    rng = _rng("eig " + case.name)  # (the same blocks for both dtypes, up to rounding)
    blocks, desc = [], []
    src_pos = 5
    vpos, voff = 2, 3
    for y, (q, kind, scale) in enumerate(case.groups):
        A = eig_block(rng, q, kind, scale, T)
        if case.place == "slot":
            ld = G
            src = y * SLOT + ((G - q) // 3) * (G + 1)
            src_pos = (y + 1) * SLOT
        else:
            ld = q + 3
            src = src_pos
            src_pos = src + (q - 1) * (ld + 1) + 1 + 5
        blocks.append(A)
        desc.append((src, vpos, voff, ld, q))
        vpos += q + 2
        voff += (q * q if q > 1 else 0) + 3
    src = prefill(dtype, src_pos)  # NaN wherever the kernel has no business reading
    for A, (s0, _, _, ld, q) in zip(blocks, desc):
        for c in range(q):
            src[s0 + c * ld:s0 + c * ld + q] = A[:, c]
    return dict(count=len(desc), max_q=case.max_q, eig=np.array(desc, dtype=np.int64).ravel(), src=src,
                vars=prefill(dtype, vpos), V=prefill(dtype, voff)), blocks, desc


def eig_figures(A, lam, V):
    """(defect, residual, eigenvalue error) of an eigen-decomposition of the float64 block A, in longdouble."""
    q = A.shape[0]
    Al, Vl, ll = A.astype(LD), V.astype(LD), lam.astype(LD)
    nf = np.sqrt((Al * Al).sum())
    nf = nf if nf > 0 else LD(1)
    ref = np.linalg.eigvalsh(A)
    defect = np.abs(Vl.T @ Vl - np.eye(q, dtype=LD)).max()
    R = np.abs(Al @ Vl - Vl * ll[None, :])
    pos = ref > 0
    resid = (R[:, pos].max() / nf) if pos.any() else LD(0)
    everr = np.abs(ll - np.maximum(ref, 0).astype(LD)).max() / nf
    return float(defect), float(resid), float(everr)


def _sorted_clamped(lam, V):
    o = np.argsort(lam, kind="stable")
    return np.maximum(lam[o], 0.0), V[:, o]


def eig_check(case, dtype, inp, blocks, desc, orc):
    """Asserts footprint and order, returns {width class: worst figure / bound} and whether f64 matched the CPU checker's Jacobi
    bit for bit."""
    u32 = 2.0 ** -24
    vars_, V = inp["vars"], inp["V"]
    foot_vars = np.zeros(vars_.size, bool)
    foot_V = np.zeros(V.size, bool)
    ratios, same = {}, True
    for A, (_, vp, vo, _, q) in zip(blocks, desc):
        foot_vars[vp:vp + q] = True
        lam = vars_[vp:vp + q].astype(np.float64)
        assert np.isfinite(lam).all(), "%s: variances of a group of %d not written" % (case.name, q)
        if q == 1:
            assert lam[0] == max(A[0, 0], 0.0), case.name
            continue
        foot_V[vo:vo + q * q] = True
        Vk = V[vo:vo + q * q].astype(np.float64).reshape(q, q).T  # column-major
        assert np.isfinite(Vk).all(), "%s: eigenbasis of a group of %d not written" % (case.name, q)
        assert (np.diff(lam) >= 0).all() and (lam >= 0).all(), "%s: variances not ascending / clamped" % case.name
        got = eig_figures(A, lam, Vk)
        lo, Vo = _sorted_clamped(*orc.eigh(A))
        ln, Vn = np.linalg.eigh(A)
        fo, fn = eig_figures(A, lo, Vo), eig_figures(A, np.maximum(ln, 0.0), Vn)
        n2, nf = np.linalg.norm(A, 2), np.linalg.norm(A)
        extra = (0.0, 0.0, 0.0) if dtype == "f64" else (2.1 * u32, u32 * n2 * np.sqrt(q) / nf, u32 * np.abs(lam).max() / nf)
        if dtype == "f64":
            same = same and (bits(lam) == bits(lo)).all() and (bits(np.ascontiguousarray(Vk)) == bits(np.ascontiguousarray(Vo))).all()
        for which in range(3):
            bound = 8 * max(fo[which], fn[which], q * 2.0 ** -52) + extra[which]
            key = (("defect", "residual", "eigenvalue")[which], width_class(q))
            ratios[key] = max(ratios.get(key, 0.0), got[which] / bound)
    assert is_prefill(vars_[~foot_vars]).all(), case.name + ": vars written outside the groups' footprint"
    assert is_prefill(V[~foot_V]).all(), case.name + ": V written outside the groups' footprint"
    return ratios, same


def jacobi_numpy(A):
    """The kernel's cyclic Jacobi, sequential and without fma, in float64: (eigenvalues ascending and clamped, V)."""
    q = A.shape[0]
    A = A.copy()
    V = np.eye(q)
    for _ in range(100):
        d2 = float((np.diag(A) ** 2).sum())
        off = float((np.triu(A, 1) ** 2).sum())
        if off == 0 or off <= 1e-32 * (d2 + off):
            break
        for r in range(q - 1):
            for c in range(r + 1, q):
                arc = A[r, c]
                if arc == 0.0:
                    continue
                theta = (A[c, c] - A[r, r]) / (2.0 * arc)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                x, y = A[:, r].copy(), A[:, c].copy()
                A[:, r], A[:, c] = cs * x - sn * y, sn * x + cs * y
                x, y = A[r, :].copy(), A[c, :].copy()
                A[r, :], A[c, :] = cs * x - sn * y, sn * x + cs * y
                x, y = V[:, r].copy(), V[:, c].copy()
                V[:, r], V[:, c] = cs * x - sn * y, sn * x + cs * y
    return _sorted_clamped(np.diag(A).copy(), V)


def emulate_eig(dtype, a, defect=None):
    T = NP_TYPE[dtype]
    d = a["eig"].reshape(-1, 5)
    for y, (src, vp, vo, ld, q) in enumerate(d):
        A = np.array([[a["src"][src + r + c * ld] for c in range(q)] for r in range(q)], dtype=np.float64)
        if q == 1:
            a["vars"][vp] = max(A[0, 0], 0)
            continue
        lam, V = jacobi_numpy(A)
        if defect == "eigvec-1e-9" and y == len(d) - 1:
            V[:, q - 1] += 1e-9 * V[:, 0]
        a["vars"][vp:vp + q] = lam.astype(T)
        a["V"][vo:vo + q * q] = V.T.ravel().astype(T)


# ---- ROTATE -----------------------------------------------------------------------------------------------------------------
RotCase = namedtuple("RotCase", "name sizes inplace")


def _rot_cases():
    shapes = [("narrow-mixed", [5, 1, 7]), ("narrow-16s", [16, 1, 16, 2, 16, 3, 13]), ("narrow-127", [16] * 7 + [15]),
              ("narrow-128", [16] * 8), ("two", [2]), ("wide-17", [3, 1, 17, 1, 4]), ("wide-64", [64, 1, 9]),
              ("wide-128", [128]), ("wide-odd", [1, 40, 1, 21])]
    out = []
    for nm, sizes in shapes:
        for inplace in (True, False):
            out.append(RotCase("%s-%s" % (nm, "inplace" if inplace else "dsrc"), sizes, inplace))
    return out


ROT_CASES = _rot_cases()


def rot_inputs(case, dtype, leg):
    T = NP_TYPE[dtype]
    rng = _rng("rot %s %s" % (case.name, leg))
    sizes = case.sizes
    nval = sum(sizes)
    goff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rvoff, vo = [], 1
    for q in sizes:
        rvoff.append(vo if q > 1 else -12345)  # (ignored for q == 1)
        vo += (q * q if q > 1 else 0) + 1
    V = prefill(dtype, vo)
    if leg == "exact":
        Dfull = rng.randint(-3, 4, size=(G, G)).astype(np.float64)
    else:
        X = rng.normal(size=(400, G))
        X[:, 1:] += 0.5 * X[:, :-1]
        X = (X - X.mean(0)) / X.std(0)
        Dfull = (X.T @ X / 400).astype(T).astype(np.float64)
    R = np.eye(G)
    for k, q in enumerate(sizes):
        if q == 1:
            continue
        o = goff[k]
        if leg == "exact":
            Vk = rng.randint(-2, 3, size=(q, q)).astype(np.float64)
        else:
            Vk = np.linalg.eigh(Dfull[o:o + q, o:o + q])[1].astype(T).astype(np.float64)
        V[rvoff[k]:rvoff[k] + q * q] = Vk.T.ravel()
        R[o:o + q, o:o + q] = Vk
    data = np.ascontiguousarray(Dfull.T.ravel()).astype(T)  # column-major slot, data in all 128 x 128 entries
    a = dict(ng=len(sizes), goff=goff, rvoff=np.array(rvoff, dtype=np.int64), V=V)
    if case.inplace:
        a["D"], a["Dsrc"] = data.copy(), None
    else:
        a["D"], a["Dsrc"] = prefill(dtype, SLOT), data
    return a, Dfull, R, nval


def rot_check(case, dtype, leg, a, Dfull, R, nval):
    """Asserts the exact leg, the copies and the footprint; returns {width class: worst error / bound} of the rounding leg."""
    T = NP_TYPE[dtype]
    u = UNIT[dtype]
    got = a["D"].reshape(G, G).T  # [row, col]
    src = Dfull.astype(T)
    Rn = R[:nval, :nval]
    ref = Rn.astype(LD).T @ Dfull[:nval, :nval].astype(LD) @ Rn.astype(LD)
    inner = got[:nval, :nval]
    assert np.isfinite(inner).all(), case.name + ": entries of the leading block not written"
    qv = np.repeat(case.sizes, case.sizes)
    qmax = np.maximum(qv[:, None], qv[None, :])
    copies = qmax == 1
    assert (bits(np.ascontiguousarray(inner))[copies] == bits(np.ascontiguousarray(src[:nval, :nval]))[copies]).all(), \
        case.name + ": an entry between two groups of one value was not copied bit for bit"
    outside = np.ones((G, G), bool)
    outside[:nval, :nval] = False
    gb, sb = bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(src))
    if case.inplace:
        assert (gb[outside] == sb[outside]).all(), case.name + ": in place, an entry outside the leading block changed"
    else:
        may = np.zeros((G, G), bool)
        if nval % 2 == 1 and max(case.sizes) <= ROT_QM:
            may[nval, :nval] = True
        pre = gb == NAN_BITS[dtype]
        assert (pre | (may & (gb == sb)))[outside].all(), case.name + ": an entry outside the footprint was written"
    ratios = {}
    if leg == "exact":
        bad = bits(np.ascontiguousarray(inner)) != bits(np.ascontiguousarray(ref.astype(T)))
        assert not bad.any(), "%s: %d entries differ from the exact R^T D R" % (case.name, bad.sum())
        return ratios
    g = gamma(qmax.astype(np.float64), u)
    bound = (2 * g + g * g) * (np.abs(Rn).T @ np.abs(Dfull[:nval, :nval]) @ np.abs(Rn))
    err = np.abs(inner.astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(copies, 0.0, err / bound)
    for cls in set(width_class(q) for q in case.sizes if q > 1):
        m = np.vectorize(width_class)(qmax) == cls
        ratios[cls] = float(r[m].max())
    return ratios


def emulate_rotate(dtype, a, defect=None):
    """Two passes in the dtype, sequential accumulation without fma; writes exactly the leading nval x nval entries."""
    T = NP_TYPE[dtype]
    goff = a["goff"]
    ng = a["ng"]
    nval = goff[ng]
    src = a["D"] if a.get("Dsrc") is None else a["Dsrc"]
    D = src.reshape(G, G).T[:nval, :nval].copy()
    Vs = []
    for k in range(ng):
        q = goff[k + 1] - goff[k]
        Vk = a["V"][a["rvoff"][k]:a["rvoff"][k] + q * q].reshape(q, q).T if q > 1 else np.ones((1, 1), T)
        Vs.append(Vk.T if defect == "v-transposed" else Vk)
    Tm = D.copy()
    for k in range(ng):
        o, q = goff[k], goff[k + 1] - goff[k]
        if q == 1:
            continue
        acc = np.zeros((nval, q), T)
        for t in range(q):
            acc = acc + D[:, o + t, None] * Vs[k][t, None, :]
        Tm[:, o:o + q] = acc
    out = Tm.copy()
    for k in range(ng):
        o, q = goff[k], goff[k + 1] - goff[k]
        if q == 1:
            continue
        acc = np.zeros((q, nval), T)
        for t in range(q):
            acc = acc + Vs[k][t, :, None] * Tm[o + t, None, :]
        out[o:o + q, :] = acc
    dst = a["D"].reshape(G, G)  # [col, row]
    dst[:nval, :nval] = out.T
    if defect == "outside-footprint":
        dst[min(nval, G - 1), G - 1] = T(1.0)


# ---- LAYOUT -----------------------------------------------------------------------------------------------------------------
LayCase = namedtuple("LayCase", "name blocks perm")  # blocks: group sizes per block; perm: visit through a permuted list

LAY_CASES = [
    LayCase("ragged", [[1, 3, 4, 5, 8, 9, 12, 13, 16, 1, 17], [40, 2, 1], [7]], False),
    LayCase("ragged-list", [[1, 3, 4, 5, 8, 9, 12, 13, 16, 1, 17], [40, 2, 1], [7]], True),
    LayCase("one-128", [[128], [128]], True),
    LayCase("128-ones", [[1] * 128, [1] * 5], False),
    LayCase("mixed-list", [[64, 64], [65, 1, 62], [1] * 100 + [28]], True),
]


def layout_tables(blocks, perm, rng, extra_groups=0):
    """Screen groups of the blocks' sizes (plus `extra_groups` that no block visits), laid out in screen order; the list and
    blk_g0 that visit them block by block."""
    sizes_visit = [q for b in blocks for q in b]
    n_vis = len(sizes_visit)
    ns = n_vis + extra_groups
    pos = rng.permutation(ns) if perm else np.arange(ns)  # list position i -> screen group
    ssize = np.zeros(ns, np.int32)
    for i, q in enumerate(sizes_visit):
        ssize[pos[i]] = q
    for i in range(n_vis, ns):
        ssize[pos[i]] = [2, 1, 5][i % 3]
    sbegin = np.concatenate([[0], np.cumsum(ssize)[:-1]]).astype(np.int32)
    voff = np.zeros(ns, np.int64)
    vo = 2
    for s in range(ns):
        voff[s] = vo if ssize[s] > 1 else -777  # (ignored for q == 1)
        vo += (ssize[s] ** 2 if ssize[s] > 1 else 0) + 1
    blk_g0 = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int32)
    lst = pos[:n_vis].astype(np.int32) if perm else None
    return dict(ns=ns, nv=int(ssize.sum()), nblk=len(blocks), n_list=n_vis if perm else 0, sbegin=sbegin, ssize=ssize, voff=voff,
                blk_g0=blk_g0, list=lst), int(vo)


def layout_reference(a):
    nblk = a["nblk"]
    d = np.zeros((nblk, GD["STRIDE"]), np.int32)
    for j in range(nblk):
        g0, g1 = a["blk_g0"][j], a["blk_g0"][j + 1]
        ng = g1 - g0
        o = 0
        d[j, GD["VQ"]:GD["VQ"] + G] = 1
        for k in range(ng):
            ss = a["list"][g0 + k] if a["list"] is not None else g0 + k
            q, b = a["ssize"][ss], a["sbegin"][ss]
            d[j, GD["GOFF"] + k] = o
            d[j, GD["GQ"] + k] = q
            d[j, GD["GSS"] + k] = ss
            sl = slice(o, o + q)
            d[j, GD["VMAP"]:][sl] = b + np.arange(q)
            d[j, GD["VGRP"]:][sl] = k
            d[j, GD["VSS"]:][sl] = ss
            d[j, GD["VOFF"]:][sl] = a["voff"][ss] if q > 1 else 0
            d[j, GD["VPOS"]:][sl] = np.arange(q)
            d[j, GD["VQ"]:][sl] = q
            o += q
        d[j, GD["GOFF"] + ng:GD["GOFF"] + G + 1] = o
        d[j, GD["NG"]], d[j, GD["NVAL"]] = ng, o
    return d


def layout_check(name, a, desc):
    ref = layout_reference(a)
    got = desc.reshape(a["nblk"], GD["STRIDE"])
    named = np.ones(GD["STRIDE"], bool)
    named[GAPS] = False
    bad = (got != ref)[:, named]
    assert not bad.any(), "%s: %d descriptor words differ (first: block %d word %d)" % (
        name, bad.sum(), np.argwhere(bad)[0][0], np.flatnonzero(named)[np.argwhere(bad)[0][1]])


def emulate_layout(dtype, a, defect=None):
    a["desc"][:] = layout_reference(a).ravel()


# ---- the solves -------------------------------------------------------------------------------------------------------------
# blocks: group sizes per block; alpha; kind: None, 'dbeta' (dbeta_tol = 1e3), 'max_active', 'newton' (newton_max_iters = 1, a
# group with eigenvalues spread 100 x), 'chained' (PANEL_SOLVE on the device's own EIG and ROTATE outputs); scale: lambda as a
# multiple of the median over the groups of ||g_k|| / pen_k, chosen on the CPU so that every width class has groups on both
# sides of the threshold over the table (tests/test_group_checks_host.py asserts it)
SolveCase = namedtuple("SolveCase", "name mode blocks alpha kind scale")
ALL_WIDTHS = [1, 3, 4, 5, 8, 9, 12, 13, 16, 1, 17]

SOLVE_CASES = [
    SolveCase("panel-all-widths", MODE_PANEL, [ALL_WIDTHS, [40, 2, 1, 13], [7, 1, 30]], 0.5, None, 1.0),
    SolveCase("panel-all-widths-lasso", MODE_PANEL, [ALL_WIDTHS, [40, 2, 1, 13], [7, 1, 30]], 1.0, None, 0.4),
    SolveCase("panel-64-64", MODE_PANEL, [[64, 64], [65, 1, 62]], 1.0, None, 0.35),
    SolveCase("panel-128", MODE_PANEL, [[128], [1] * 128, [96, 5]], 0.5, None, 1.0),
    SolveCase("panel-wide-zero", MODE_PANEL, [[64, 40], [65, 17], [128]], 0.5, None, 2.5),
    SolveCase("panel-chained", MODE_PANEL, [ALL_WIDTHS, [64, 3, 33]], 0.5, "chained", 1.0),
    SolveCase("panel-dbeta", MODE_PANEL, [[2, 3, 4, 16, 17, 40], [65, 20]], 0.5, "dbeta", 1.0),
    SolveCase("panel-max-active", MODE_PANEL, [ALL_WIDTHS, [5, 1]], 0.5, "max_active", 0.3),
    SolveCase("panel-newton", MODE_PANEL, [[3, 13, 1], [6]], 0.5, "newton", 0.05),
    SolveCase("gram-narrow", MODE_GRAM, [[1, 3, 4, 5, 8, 9, 12, 13, 16, 1], [16, 2, 1, 13, 7], [11, 1]], 0.5, None, 1.0),
    SolveCase("gram-max-active", MODE_GRAM, [[3, 4, 1, 16], [5, 1]], 1.0, "max_active", 0.3),
]
SOLVE_BY_NAME = {c.name: c for c in SOLVE_CASES}


def solve_inputs(case, dtype):
    """The arrays of one solve call (dict for device_call / emulate_call) and what the checker needs next to them."""
    T = NP_TYPE[dtype]
    rng = _rng("solve " + case.name)
    gram = case.mode == MODE_GRAM
    a, v_elems = layout_tables(case.blocks, True, rng, extra_groups=4 if gram else 0)
    ns, nv = a["ns"], a["nv"]
    n = 400
    X = rng.normal(size=(n, nv))
    X[:, 1:] += 0.6 * X[:, :-1]  # correlated neighbours
    X = (X - X.mean(0)) / X.std(0)
    if case.kind == "newton":
        X = X * np.where(np.arange(nv) % 2 == 0, 10.0, 1.0)  # eigenvalues of every group spread ~100 x
    Cm = (X.T @ X / n).astype(T).astype(np.float64)
    Cm = np.triu(Cm) + np.triu(Cm, 1).T
    vars_ = np.zeros(nv, T)
    V = prefill(dtype, v_elems)
    for s in range(ns):
        b, q = a["sbegin"][s], a["ssize"][s]
        if q == 1:
            vars_[b] = max(Cm[b, b], 0)
        else:
            lam, Vk = np.linalg.eigh(Cm[b:b + q, b:b + q])
            vars_[b:b + q] = np.maximum(lam, 0)
            V[a["voff"][s]:a["voff"][s] + q * q] = Vk.T.ravel()
    spen = rng.uniform(0.5, 1.5, size=ns).astype(T)
    spen[a["list"][min(3, len(a["list"]) - 1)]] = 0
    beta0 = (0.3 * rng.normal(size=nv)).astype(T)
    for s in range(0, ns, 2):
        beta0[a["sbegin"][s]:a["sbegin"][s] + a["ssize"][s]] = 0
    btrue = rng.normal(size=nv) * (rng.uniform(size=nv) < 0.3)
    y = X @ btrue / np.sqrt(nv) + 0.5 * rng.normal(size=n)
    g = (X.T @ (y - X @ beta0.astype(np.float64)) / n).astype(T)
    gn = np.array([np.linalg.norm(g[a["sbegin"][s]:a["sbegin"][s] + a["ssize"][s]].astype(np.float64)) / max(float(spen[s]), 0.5)
                   for s in a["list"]])
    lmda = float(np.median(gn)) * case.scale
    a.update(vars=vars_, V=V, xmean=rng.uniform(-1, 1, size=nv).astype(T), spen=spen, vcol=(7 + 3 * rng.permutation(nv)).astype(np.int32),
             beta=beta0.copy(), is_active=np.zeros(ns, np.int8), active_set=np.full(ns, -1, np.int32),
             l1=lmda * case.alpha, l2=lmda * (1 - case.alpha), newton_tol=NEWTON_TOL[dtype], dbeta_tol=0.0, newton_max_iters=1000,
             max_active_size=ns, mark=1, rsq=0.25, resid_sum=-0.5, n_updates=11, active_size=0,
             desc=np.full(a["nblk"] * GD["STRIDE"], -1, np.int32), st_f=np.full(3 * a["nblk"], np.nan), st_i=np.full(4 * a["nblk"], -1, np.int64))
    # part of the groups active on entry, in the order of the screen set
    act = [s for s in range(ns) if s % 3 == 0]
    a["is_active"][act] = 1
    a["active_set"][:len(act)] = act
    a["active_size"] = len(act)
    if case.kind == "dbeta":
        a["dbeta_tol"] = 1e3
    if case.kind == "max_active":
        a["max_active_size"] = a["active_size"] + 2
    if case.kind == "newton":
        a["newton_max_iters"] = 1
    if gram:
        a.update(C=np.ascontiguousarray(Cm.T.ravel()).astype(T), ldc=nv, g=g.copy())
    else:
        nblk = a["nblk"]
        a.update(Dblk=prefill(dtype, nblk * SLOT), gblk=prefill(dtype, nblk * G), dcol=np.full(nblk * G, -1, np.int32),
                 dlt=prefill(dtype, nblk * G), dd=prefill(dtype, nblk * G))
        for j in range(nblk):
            idx = block_values(a, j)
            nval = len(idx)
            a["gblk"][j * G:j * G + nval] = g[idx]
            R = block_R(a, j)
            Dt = (R.astype(LD).T @ Cm[np.ix_(idx, idx)].astype(LD) @ R.astype(LD)).astype(T)
            slot = a["Dblk"][j * SLOT:(j + 1) * SLOT].reshape(G, G)  # [col, row]
            low = np.tril(np.ones((nval, nval), bool), -1)  # the solve reads below the diagonal only: the rest stays NaN
            slot[:nval, :nval][low.T] = Dt.T[low.T]
    return a, dict(C=Cm, g=g.astype(np.float64), beta0=beta0.copy())


def block_groups(a, j):
    g0, g1 = a["blk_g0"][j], a["blk_g0"][j + 1]
    return [int(a["list"][i]) if a["list"] is not None else i for i in range(g0, g1)]


def block_values(a, j):
    return np.concatenate([a["sbegin"][s] + np.arange(a["ssize"][s]) for s in block_groups(a, j)])


def group_V(a, s):
    q = a["ssize"][s]
    return a["V"][a["voff"][s]:a["voff"][s] + q * q].astype(np.float64).reshape(q, q).T if q > 1 else np.ones((1, 1))


def block_R(a, j):
    idx = block_values(a, j)
    R = np.eye(len(idx))
    o = 0
    for s in block_groups(a, j):
        q = a["ssize"][s]
        R[o:o + q, o:o + q] = group_V(a, s)
        o += q
    return R


def threshold_margins(case, dtype, a, aux, out):
    """Per visited group of a finished call: (| ||u|| - l1p | / l1p, min(Lambda) + l2p), from `solve_check`'s own u."""
    return solve_check(case, dtype, a, aux, out, margins_only=True)


def solve_check(case, dtype, a_in, aux, a, margins_only=False):
    """`a_in`: the call's arrays before it ran (solve_inputs), `a`: after.  Asserts the exact legs and the bookkeeping; returns
    {(kind, width class): worst error / bound}."""
    T = NP_TYPE[dtype]
    u = UNIT[dtype]
    gram = case.mode == MODE_GRAM
    nblk, nv = a["nblk"], a["nv"]
    Cm = aux["C"].astype(LD)
    beta0, beta1 = aux["beta0"], a["beta"]
    delta = beta1.astype(LD) - beta0.astype(LD)
    l1, l2 = LD(a["l1"]), LD(a["l2"])
    tol = a["newton_tol"]
    ratios, margins = {}, []

    def put(key, err, bound):
        r = float(err / bound) if bound > 0 else (0.0 if err == 0 else np.inf)
        ratios[key] = max(ratios.get(key, 0.0), r)

    rsq, rsum, cm = LD(a_in["rsq"]), LD(a_in["resid_sum"]), LD(0)
    rsq_b, rsum_b, cm_b = LD(0), LD(0), LD(0)       # bounds accumulated along the call
    rsq_abs, rsum_abs = abs(rsq), abs(rsum)
    n_upd, asz = a_in["n_updates"], a_in["active_size"]
    is_act = a_in["is_active"].copy()
    act_set = list(a_in["active_set"][:asz])
    status = CD_OK
    visited = np.zeros(nv, bool)
    nvis = 0
    if not gram:
        layout_check(case.name, a, a["desc"])
    if case.kind == "newton" and not margins_only:
        assert (a["st_i"][2::4][:1 if gram else nblk] == CD_NEWTON).all(), case.name + ": status is not CD_NEWTON"
        return ratios
    for j in range(nblk):
        groups = block_groups(a, j)
        idx = block_values(a, j)
        nval = len(idx)
        nvis += nval
        o = 0
        for s in groups:
            q, b = a["ssize"][s], a["sbegin"][s]
            vk = b + np.arange(q)
            if status != CD_OK:
                assert (bits(beta1[vk]) == bits(beta0[vk])).all(), case.name + ": a group behind the failing one was visited"
                o += q
                continue
            Vk = group_V(a, s).astype(LD)
            lam = a["vars"][vk].astype(LD)
            pen = LD(a["spen"][s])
            l1p, l2p = l1 * pen, l2 * pen
            bvec = lam + l2p
            # earlier values: of this block (PANEL_SOLVE: its gradient was handed over for the block) / of the pass (GRAM_PASS)
            prev = np.flatnonzero(visited) if gram else idx[:o]
            gk = (aux["g"][vk] if gram else a_in["gblk"][j * G + o:j * G + o + q]).astype(LD)
            Dkm = Cm[np.ix_(vk, prev)]
            grad = gk - Dkm @ delta[prev]
            bt0 = Vk.T @ beta0[vk].astype(LD)
            uu = Vk.T @ grad + lam * bt0
            nu = np.sqrt((uu * uu).sum())
            gnk = gamma(nval + q, u) if not gram else gamma(len(prev) + q + 2 * nblk, u)
            e_u = gnk * (np.abs(Vk).T @ (np.abs(gk) + np.abs(Dkm) @ np.abs(delta[prev])) + lam * (np.abs(Vk).T @ np.abs(beta0[vk].astype(LD))))
            e_V = LD(0)
            for m in (groups[:groups.index(s)] if not gram else []):
                Vm = group_V(a, m).astype(LD)
                Em = np.sqrt(((Vm.T @ Vm - np.eye(len(Vm))) ** 2).sum())
                vm = a["sbegin"][m] + np.arange(a["ssize"][m])
                e_V += np.sqrt((Cm[np.ix_(vk, vm)] ** 2).sum()) * Em * np.sqrt((beta0[vm].astype(LD) ** 2).sum())
                if not gram:  # the rotated block was rounded to the dtype (chained: it is the device's own rotation)
                    Q = max(q, len(vm))
                    f = u + ((2 * gamma(Q, u) + gamma(Q, u) ** 2) if case.kind == "chained" else 0)
                    e_u = e_u + f * ((np.abs(Vk).T @ np.abs(Cm[np.ix_(vk, vm)]) @ np.abs(Vm)) @ np.abs(Vm.T @ delta[vm]))
            Ek = np.sqrt(((Vk.T @ Vk - np.eye(q)) ** 2).sum())
            bt = Vk.T @ beta1[vk].astype(LD)
            nbt = np.sqrt((bt * bt).sum())
            e_V += Ek * (bvec.max() * nbt + 2 * l1p + lam.max() * np.sqrt((bt0 * bt0).sum()))
            ne_u = np.sqrt((e_u * e_u).sum())
            margins.append((s, q, float(abs(nu - l1p) / l1p) if l1p > 0 else np.inf, float(bvec.min())))
            cls = width_class(q)
            zero_new = not beta1[vk].any()
            changed = bool((bits(beta1[vk]) != bits(beta0[vk])).any())
            if a["dbeta_tol"] > 0 and q > 1 and not changed:
                pass  # (the change test declined the update: nothing to measure)
            elif nu + ne_u + e_V < l1p:
                assert zero_new, "%s: group of %d below the threshold (||u|| = %.6e, l1 p = %.6e) is not exactly zero" % (
                    case.name, q, nu, l1p)
            elif zero_new:
                put(("threshold", cls), nu - l1p, ne_u + e_V)
            elif dtype == "f64" or q <= 16:
                res = uu - bvec * bt - l1p * bt / nbt
                bound = l1p * tol + ne_u + gamma(q + 4, u) * (np.sqrt(((bvec * bt) ** 2).sum()) + l1p) + bvec.max() * gamma(q, u) * nbt + e_V
                put(("visit", cls), np.sqrt((res * res).sum()), bound)
            if changed:
                dt = Vk.T @ delta[vk]
                gg = uu - lam * bt0
                e_d = (Ek + q * gamma(q, u)) * (nbt + np.sqrt((bt0 * bt0).sum()))
                terms = dt * (2 * gg - dt * lam)
                rsq += terms.sum()
                rsq_abs += (np.abs(dt) * (2 * np.abs(gg) + np.abs(dt) * lam)).sum()
                rsq_b += 2 * (np.abs(dt) * e_u).sum() + e_d * 2 * np.sqrt(((np.abs(gg) + np.abs(dt) * lam) ** 2).sum())
                xm = a["xmean"][vk].astype(LD)
                rsum -= (xm * delta[vk]).sum()
                xt = Vk.T @ xm
                rsum_abs += (np.abs(xt) * np.abs(dt)).sum()
                rsum_b += (Ek * np.sqrt((dt * dt).sum()) + e_d) * np.sqrt((xm * xm).sum()) * (1 + Ek)
                c1 = (lam * dt * dt).sum() / q
                c1_b = gamma(q + 4, u) * c1 + 2 * np.sqrt(((lam * np.abs(dt)) ** 2).sum()) * e_d / q + lam.max() * e_d * e_d / q
                cm, cm_b = max(cm, c1), max(cm_b, c1_b)  # |max(x + e) - max(x)| <= max |e|
                if a["mark"] and not is_act[s]:
                    if asz >= a["max_active_size"]:
                        status = CD_MAX_ACTIVE
                    else:
                        is_act[s] = 1
                        act_set.append(s)
                        asz += 1
                if status == CD_OK:
                    n_upd += 1
            visited[vk] = True
            o += q
        if margins_only:
            continue
        sf = a["st_f"][3 * j:3 * j + 3] if not gram else a["st_f"][:3]
        si = a["st_i"][4 * j:4 * j + 4] if not gram else a["st_i"][:4]
        if not gram:  # the bit-for-bit bookkeeping of the block
            b0, b1 = beta0[idx], beta1[idx]
            ch = bits(b1) != bits(b0)
            nz = int(ch.sum())
            d = (b1 - b0).astype(T)
            dd = a["dd"][j * G:(j + 1) * G]
            assert (bits(dd[:nval]) == bits(d)).all(), case.name + ": dd is not beta_new - beta0 bit for bit"
            assert not dd[nval:].any(), case.name + ": dd is not zero beyond the block"
            if status == CD_OK:
                assert si[3] == nz, "%s: nz = %d, %d values changed" % (case.name, si[3], nz)
                assert (bits(a["dlt"][j * G:j * G + nz]) == bits(d[ch])).all(), case.name + ": dlt is not the changes bit for bit"
                assert (a["dcol"][j * G:j * G + nz] == a["vcol"][idx[ch]]).all(), case.name + ": dcol is not vcol of the changed values"
                assert is_prefill(a["dlt"][j * G + nz:(j + 1) * G]).all() and (a["dcol"][j * G + nz:(j + 1) * G] == -1).all(), \
                    case.name + ": dlt / dcol written beyond nz"
        if gram and j < nblk - 1:
            continue
        assert si[2] == status, "%s: status %d, expected %d" % (case.name, si[2], status)
        if status == CD_OK:
            assert si[0] == n_upd, "%s: n_updates %d, expected %d" % (case.name, si[0], n_upd)
            assert si[1] == asz, "%s: active_size %d, expected %d" % (case.name, si[1], asz)
            gN = gamma(nvis + 8, u)
            put(("rsq", "state"), abs(LD(sf[0]) - rsq), gN * rsq_abs + rsq_b)
            put(("resid_sum", "state"), abs(LD(sf[1]) - rsum), gN * rsum_abs + rsum_b)
            put(("cm", "state"), abs(LD(sf[2]) - cm), cm_b + gamma(4, u) * cm)
    if margins_only:
        return margins
    if status == CD_OK:
        assert (a["is_active"] == is_act).all(), case.name + ": is_active"
        assert (a["active_set"][:asz] == np.array(act_set, np.int32)).all(), case.name + ": active_set does not follow visit order"
        assert (a["active_set"][asz:] == -1).all(), case.name + ": active_set written beyond active_size"
    else:
        assert status == CD_MAX_ACTIVE and (a["st_i"][1::4][:1 if gram else nblk] == a["max_active_size"]).all(), case.name
    if case.kind == "dbeta":
        assert (bits(beta1) == bits(beta0)).all() and (a["st_i"][3::4] == 0).all() and (a["st_i"][0::4] == a_in["n_updates"]).all()
        assert (a["st_f"][0::3] == a_in["rsq"]).all() and (a["st_f"][1::3] == a_in["resid_sum"]).all(), case.name
    untouched = ~visited
    assert (bits(beta1[untouched]) == bits(beta0[untouched])).all(), case.name + ": a value outside the visited blocks changed"
    if gram and status == CD_OK:
        Cd = np.abs(Cm) @ np.abs(delta)
        nzt = int((delta != 0).sum())
        bound = gamma(nzt + 2, u) * Cd + nblk * u * (np.abs(aux["g"].astype(LD)) + Cd)
        err = np.abs(a["g"].astype(LD) - (aux["g"].astype(LD) - Cm @ delta))
        for inside in (True, False):
            m = visited == inside
            if m.any():
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where(bound[m] > 0, err[m] / bound[m], np.where(err[m] == 0, 0, np.inf))
                ratios[("g", "visited" if inside else "unvisited")] = float(r.max())
    return ratios


# ---- numpy emulation of the solves (target dtype, sequential, no fma) ---------------------------------------------------------
def _newton(T, v, b, l1p, tol, max_iters, accept=1.0):
    """x of the group update for ||v|| > l1p > 0: Newton on f(h) = sum v^2 / (b h + l1p)^2 - 1 from h = 0, in dtype T."""
    h = T(0)
    it = 0
    while True:
        b2 = T(1) / (b * h + l1p)
        x = (v * b2) ** 2
        t = x.sum(dtype=T)
        sx = (x * b * b2).sum(dtype=T)
        fh = t - T(1)
        if abs(fh) <= tol or it >= max_iters:
            break
        h = max(h + t * (np.sqrt(t) - T(1)) / sx, T(0))
        it += 1
    if accept != 1.0:  # planted defect: the point left of the root with f = accept * tol  (f' = -2 sx)
        h = T(h - (accept * tol - fh) / (2 * sx))
        b2 = T(1) / (b * h + l1p)
    return h * v * b2, it


def emulate_solve(mode, dtype, a, defect=None):
    """The sequential group visits of one call in dtype T, in original coordinates with per-visit rotations (the reference's
    form); fills every output of the mode.  `defect` plants one of the defects of tests/test_group_checks_host.py."""
    T = NP_TYPE[dtype]
    gram = mode == MODE_GRAM
    nblk = a["nblk"]
    emulate_layout(dtype, a)
    rsq, rsum, cm = T(a["rsq"]), T(a["resid_sum"]), T(0)
    n_upd, asz, status = a["n_updates"], a["active_size"], CD_OK
    l1, l2 = T(a["l1"]), T(a["l2"])
    beta = a["beta"]
    C = a["C"].reshape(a["nv"], a["ldc"]).astype(np.float64) if gram else None  # symmetric
    for j in range(nblk):
        groups = block_groups(a, j)
        idx = block_values(a, j)
        nval = len(idx)
        if gram:
            D = C[np.ix_(idx, idx)].astype(T)
            g = a["g"][idx].copy()
        else:
            R = block_R(a, j).astype(T)
            Dt = a["Dblk"][j * SLOT:(j + 1) * SLOT].reshape(G, G).T[:nval, :nval]
            Dt = np.tril(np.nan_to_num(Dt), -1)
            g = a["gblk"][j * G:j * G + nval].copy()
        b0 = beta[idx].copy()
        bnew = b0.copy()
        gT = g.copy()  # PANEL_SOLVE: rotated gradient, kept current with the rotated block
        bT = b0.copy()
        if not gram:
            o = 0
            for s in groups:
                q = a["ssize"][s]
                Vk = R[o:o + q, o:o + q]
                gT[o:o + q] = (Vk.T @ g[o:o + q]).astype(T)
                bT[o:o + q] = (Vk.T @ b0[o:o + q]).astype(T)
                o += q
        o = 0
        if j == 0:
            cm = T(0)
        for s in groups:
            q = a["ssize"][s]
            if status != CD_OK:
                break
            sl = slice(o, o + q)
            Vk = group_V(a, s).astype(T)
            lam = a["vars"][idx[sl]]
            pen = a["spen"][s]
            l1p, l2p = l1 * pen, (T(0) if defect == "no-l2" else l2 * pen)
            if gram:
                gk_rot = (Vk.T @ gT[sl]).astype(T)
                ako = (Vk.T @ bnew[sl]).astype(T)
            else:
                gk_rot, ako = gT[sl].copy(), bT[sl].copy()
            v = (gk_rot + lam * ako).astype(T)
            nrm = np.sqrt((v * v).sum(dtype=T))
            bvec = (lam + l2p).astype(T)
            if nrm <= l1p:
                x = np.zeros(q, T)
            elif l1p <= 0:
                x = (v / bvec).astype(T)
            else:
                x, it = _newton(T, v, bvec, l1p, T(a["newton_tol"]), a["newton_max_iters"], 10.0 if defect == "loose-root" else 1.0)
                if it >= a["newton_max_iters"]:
                    status = CD_NEWTON
                    break
            d = (x - ako).astype(T)
            thr = T(a["dbeta_tol"]) * np.sqrt(T(q))
            if (q == 1 and x[0] != ako[0]) or (q > 1 and not np.sqrt((d * d).sum(dtype=T)) <= thr):
                c1 = (lam * d * d).sum(dtype=T) / T(q)
                cm = max(cm, c1)
                if not (defect == "rsq-skip" and q == 13):
                    rsq = rsq + (d * (T(2) * gk_rot - d * lam)).sum(dtype=T)
                if gram:
                    new = (Vk @ x).astype(T)
                    dl = (new - bnew[sl]).astype(T)
                    bnew[sl] = new
                else:
                    bT[sl] = x
                    bnew[sl] = (Vk @ x).astype(T)
                if a["mark"] and not a["is_active"][s]:
                    if asz >= a["max_active_size"]:
                        status = CD_MAX_ACTIVE
                        break
                    a["is_active"][s] = 1
                    a["active_set"][asz] = s
                    asz += 1
                if gram:
                    rsum = rsum - (a["xmean"][idx[sl]] * dl).sum(dtype=T)
                    qq = q - 1 if (defect == "grad-skip" and q == 13) else q
                    gT = (gT - D[:, o:o + qq] @ dl[:qq]).astype(T)
                else:
                    rsum = rsum - ((Vk.T @ a["xmean"][idx[sl]]).astype(T) * d).sum(dtype=T)
                    qq = q - 1 if (defect == "grad-skip" and q == 13) else q
                    gT[o + q:] = (gT[o + q:] - Dt[o + q:, o:o + qq] @ d[:qq]).astype(T)
                n_upd += 1
            o += q
        ch = bits(bnew) != bits(b0)
        nz = int(ch.sum())
        dvec = (bnew - b0).astype(T)
        beta[idx] = bnew
        if gram:
            a["g"][:] = (a["g"] - C[:, idx[ch]].astype(T) @ dvec[ch]).astype(T)
            a["st_f"][:3] = [rsq, rsum, cm]
            a["st_i"][:4] = [n_upd, asz, status, nz]
        else:
            a["dd"][j * G:(j + 1) * G] = 0
            a["dd"][j * G:j * G + nval] = dvec
            a["dlt"][j * G:j * G + nz] = dvec[ch]
            if defect == "dlt-ulp" and nz:
                a["dlt"][j * G] = np.nextafter(a["dlt"][j * G], T(np.inf))
            a["dcol"][j * G:j * G + nz] = a["vcol"][idx[ch]]
            a["st_f"][3 * j:3 * j + 3] = [rsq, rsum, cm]
            a["st_i"][4 * j:4 * j + 4] = [n_upd, asz, status, nz]


def emulate_call(mode, dtype, a, defect=None):
    if mode == MODE_EIG:
        emulate_eig(dtype, a, defect)
    elif mode == MODE_ROTATE:
        emulate_rotate(dtype, a, defect)
    elif mode == MODE_LAYOUT:
        emulate_layout(dtype, a, defect)
    else:
        emulate_solve(mode, dtype, a, defect)


def copy_inputs(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


def chain_eig_rotate(call, dtype, a, aux):
    """The chained case: replaces vars / V / Dblk of a PANEL_SOLVE call by what `call`'s own EIG and ROTATE give on the
    unrotated blocks.  `call(mode, dtype, arrays)` is device_call with a backend bound, or emulate_call."""
    T = NP_TYPE[dtype]
    Cm = aux["C"]
    for j in range(a["nblk"]):
        idx = block_values(a, j)
        nval = len(idx)
        src = np.zeros(SLOT, T)
        src.reshape(G, G)[:nval, :nval] = Cm[np.ix_(idx, idx)].T
        groups = block_groups(a, j)
        desc, goff, rvoff = [], [0], []
        o = 0
        for s in groups:
            q = a["ssize"][s]
            desc.append((o * (G + 1), a["sbegin"][s], a["voff"][s] if q > 1 else 0, G, q))
            rvoff.append(a["voff"][s] if q > 1 else 0)
            o += q
            goff.append(o)
        e = dict(count=len(desc), max_q=min(max(a["ssize"][s] for s in groups), EIG_MAX_Q), eig=np.array(desc, np.int64).ravel(), src=src,
                 vars=a["vars"], V=a["V"])
        call(MODE_EIG, dtype, e)
        r = dict(ng=len(groups), goff=np.array(goff, np.int32), rvoff=np.array(rvoff, np.int64), V=a["V"],
                 D=a["Dblk"][j * SLOT:(j + 1) * SLOT], Dsrc=src)
        r["D"][:] = prefill(dtype, SLOT)
        call(MODE_ROTATE, dtype, r)
