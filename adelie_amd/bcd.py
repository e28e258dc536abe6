"""``adelie.bcd``: the group elastic net update

    minimise  1/2 sum_i quad_i x_i^2 - linear' x + l1 ||x||_2 + l2 / 2 ||x||_2^2

which every group engine runs inside its visit, offered on its own: ``h = ||x||_2`` is the non-negative root of
:func:`root_function` (with ``quad + l2`` for ``quad``) and ``x = h linear / ((quad + l2) h + l1)``.

* :func:`solve` and :func:`root` have the reference's keyword arguments, defaults and return dictionaries (``adelie/bcd.py``,
  ``py_bcd.cpp``).  ``solver`` is ``"newton"`` (Newton from ``h = 0``) or ``"newton_abs"`` (Newton from adaptive bisection
  starts, the default); both run in a HIP kernel (``csrc/kernels_bcd.hip``) that restates ``bcd/unconstrained/newton.hpp`` and
  ``optimization/newton.hpp`` operation for operation within a problem.  A solve that stops at ``max_iters`` returns what it has
  with ``iters == max_iters``, as the reference's binding does.
* :func:`solve_many` is new here: any number of independent problems, of one length or of any mix of lengths, in one native
  call.  That is the shape of a proximal-gradient step over many groups, and the shape at which the device earns its keep.  A
  problem's ``beta`` and ``iters`` have the same bits whatever batch it is solved in and wherever it sits in it.
* :func:`root_lower_bound`, :func:`root_upper_bound`, :func:`root_function` and :func:`objective` restate ``bcd/utils.hpp`` in
  numpy: O(d) scalar host routines with nothing in them for a device.

Out of scope, on purpose: the solvers ``"newton_brent"``, ``"brent"``, ``"ista"``, ``"fista"``, ``"fista_adares"`` (the reference
documents the last four as converging poorly) and ``"newton_abs_debug"``; they raise ``NotImplementedError``.
"""
import numpy as np

from . import _abi

__all__ = ["root_lower_bound", "root_upper_bound", "root_function", "objective", "solve", "solve_many", "root"]

_UNSUPPORTED = ("newton_brent", "brent", "ista", "fista", "fista_adares", "newton_abs_debug")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def root_lower_bound(*, quad, linear, l1):
    """``h >= 0`` with ``root_function(h) >= 0`` whenever ``||linear||_2 > l1`` (``bcd/utils.hpp:22-41``)."""
    quad, linear, l1 = _f64(quad), _f64(linear), float(l1)
    b = l1 * float(np.sum(quad))
    a = float(np.sum(quad * quad))
    v_l1 = float(np.sum(np.abs(linear)))
    c = l1 * l1 * quad.size - v_l1 * v_l1
    discr = b * b - a * c
    with np.errstate(divide="ignore", invalid="ignore"):
        h_min = float((-b + np.sqrt(max(discr, 0.0))) / np.float64(a)) if discr > -1e-12 else 0.0
    return max(h_min, 0.0)


def _root_upper_bound(quad, linear, l1, zero_tol):
    """``(h_max, smallest entry of quad above zero_tol)`` (``bcd/utils.hpp:61-96``)."""
    q_min = float(np.min(quad))
    with np.errstate(divide="ignore", invalid="ignore"):
        if q_min <= zero_tol:
            nz = quad > zero_tol
            v2 = linear * linear
            h_max = float(np.sum(v2[nz] / (quad[nz] * quad[nz])))
            v_S = float(np.sum(v2[quad <= 0]))
            min_nnz = float(np.min(quad[nz])) if nz.any() else np.inf
            h_max = float(np.sqrt(max(np.float64(h_max) / (1 - np.float64(v_S) / (l1 * l1)), 0.0)))
            return h_max, min_nnz
        return float(np.sqrt(np.sum((linear / quad) ** 2))), q_min


def root_upper_bound(*, quad, linear, l1, zero_tol=1e-14):
    """``h >= 0`` that bounds the root from above when ``||linear_S||_2 < l1`` on ``S = {i : quad_i = 0}``; with ``zero_tol > 0``
    entries up to ``zero_tol`` count as zero and ``root_function(h) <= 0`` is no longer guaranteed."""
    return _root_upper_bound(_f64(quad), _f64(linear), float(l1), float(zero_tol))[0]


def root_function(h, *, quad, linear, l1):
    """``phi(h) = sum_i linear_i^2 / (quad_i h + l1)^2 - 1``."""
    quad, linear = _f64(quad), _f64(linear)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum((linear / (quad * float(h) + float(l1))) ** 2) - 1)


def objective(beta, *, quad, linear, l1, l2):
    """The objective of the group update at ``beta``."""
    beta_norm = np.linalg.norm(beta)
    return 0.5 * quad @ beta ** 2 - linear @ beta + l1 * beta_norm + 0.5 * l2 * beta_norm ** 2


def _solver_code(solver):
    if solver in _UNSUPPORTED:
        raise NotImplementedError(f'solver "{solver}" is not implemented: the solvers that exist are "newton" and "newton_abs".')
    try:
        return _abi.BCD_SOLVER[solver]
    except (KeyError, TypeError):
        raise ValueError(f'unknown solver {solver!r}: the solvers that exist are "newton" and "newton_abs".') from None


def _is_torch(a):
    return not isinstance(a, (np.ndarray, list, tuple)) and type(a).__module__.startswith("torch")


def _torch_dtype(t):
    try:
        return np.dtype({"torch.float64": np.float64, "torch.float32": np.float32}[str(t.dtype)])
    except KeyError:
        raise TypeError("quad and linear must be float32 or float64.") from None


def _values(name, a, dtype):
    """``(keep, pointer, is_dev, lengths or (B, d), device)`` of one of quad / linear."""
    if _is_torch(a):
        if a.dim() != 2 or not a.is_cuda or not a.is_contiguous():
            raise TypeError(f"{name}: a torch tensor must be 2-D, C-contiguous and in device memory.")
        if _torch_dtype(a) != dtype:
            raise TypeError(f"{name} must have quad's dtype ({dtype}).")
        return a, int(a.data_ptr()), True, tuple(int(n) for n in a.shape), a.device.index or 0
    if isinstance(a, np.ndarray) and a.ndim == 2:
        a = np.ascontiguousarray(a, dtype=dtype)
        return a, a.ctypes.data, False, a.shape, None
    rows = [np.asarray(r, dtype=dtype) for r in a]
    if any(r.ndim != 1 for r in rows):
        raise TypeError(f"{name} must be a (B, d) array or a sequence of 1-D arrays.")
    flat = np.concatenate(rows) if rows else np.empty(0, dtype=dtype)
    flat = np.ascontiguousarray(flat, dtype=dtype)
    return flat, flat.ctypes.data, False, [r.size for r in rows], None


def _penalty(name, a, B, dtype):
    a = np.asarray(a, dtype=dtype)
    if a.ndim > 1 or (a.ndim == 1 and a.size != B):
        raise TypeError(f"{name} must be a scalar or (B,).")
    return np.ascontiguousarray(np.broadcast_to(a, (B,)))


def solve_many(*, quad, linear, l1, l2, tol=1e-12, max_iters=1000, solver="newton_abs", device=0):
    """Solves ``B`` independent group updates in one native call.

    ``quad`` / ``linear`` are ``(B, d)`` arrays, or sequences of ``B`` one-dimensional arrays of any mix of lengths; ``l1`` /
    ``l2`` are scalars or ``(B,)``.  The dtype is ``quad``'s (float32 or float64; anything else is taken as float64).  A
    rectangular ``quad`` / ``linear`` may be a C-contiguous torch tensor in device memory: it is read in place, and ``beta`` then
    comes back as a tensor on that device.

    Returns ``{"beta", "iters", "time_elapsed"}``: ``beta`` in the shape of the input (a list of arrays for ragged input),
    ``iters`` the ``(B,)`` int64 Newton steps taken, ``time_elapsed`` the seconds of the native call.
    """
    code = _solver_code(solver)
    if _is_torch(quad):
        dtype = _torch_dtype(quad)
    else:
        first = quad if isinstance(quad, np.ndarray) else (np.asarray(quad[0]) if len(quad) else np.empty(0))
        dtype = np.dtype(np.float32) if first.dtype == np.float32 else np.dtype(np.float64)
    q_keep, q_ptr, q_dev, q_shape, q_where = _values("quad", quad, dtype)
    v_keep, v_ptr, v_dev, v_shape, v_where = _values("linear", linear, dtype)
    if isinstance(q_shape, tuple) != isinstance(v_shape, tuple) or list(q_shape) != list(v_shape):
        raise ValueError("quad and linear must have the same shape (the same lengths, problem by problem).")
    rect = isinstance(q_shape, tuple)
    if q_where is not None and v_where is not None and q_where != v_where:
        raise RuntimeError("quad and linear must live on one device.")
    for where in (q_where, v_where):
        if where is not None:
            device = where
    B = q_shape[0] if rect else len(q_shape)
    offsets = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.full(B, q_shape[1], dtype=np.int64) if rect else np.asarray(q_shape, dtype=np.int64), out=offsets[1:])
    l1 = _penalty("l1", l1, B, dtype)
    l2 = _penalty("l2", l2, B, dtype)
    tol, max_iters = float(tol), int(max_iters)
    if tol < 0:
        raise RuntimeError("adelie_core solver: tol must be >= 0.")
    if max_iters < 0:
        raise TypeError("max_iters must be non-negative.")
    iters = np.zeros(B, dtype=np.int64)
    if q_dev:
        import torch

        beta = torch.empty_like(quad)
        beta_ptr = int(beta.data_ptr())
    else:
        beta = np.empty(int(offsets[-1]), dtype=dtype)
        beta_ptr = beta.ctypes.data
    elapsed = _abi.C.c_double(0.0)
    if B > 0:
        if q_dev or v_dev:
            import torch

            torch.cuda.current_stream(device).synchronize()  # the native call runs on a stream of its own
        C = _abi.C
        args = _abi.BcdArgs(
            dtype=_abi.dtype_code(dtype), device=int(device), solver=code, _pad0=0, n_problems=B, offsets=_abi.ptr(offsets),
            quad=q_ptr, linear=v_ptr, l1=_abi.ptr(l1), l2=_abi.ptr(l2), quad_is_dev=int(q_dev), linear_is_dev=int(v_dev),
            l1_is_dev=0, l2_is_dev=0, tol=tol, max_iters=max_iters, beta=beta_ptr, beta_is_dev=int(q_dev), _pad1=0,
            iters=_abi.ptr(iters), status=None, time_elapsed=C.cast(C.pointer(elapsed), C.c_void_p))
        backend = _abi.hip_backend()
        backend.check(backend.fn("bcd_solve")(C.byref(args)))
    del q_keep, v_keep  # (alive until the call has returned)
    if not q_dev:
        beta = beta.reshape(q_shape) if rect else [beta[offsets[k]:offsets[k + 1]] for k in range(B)]
    return {"beta": beta, "iters": iters, "time_elapsed": elapsed.value}


def solve(*, quad, linear, l1, l2, tol=1e-12, max_iters=1000, solver="newton_abs"):
    """Solves one group update (:func:`solve_many` with ``B = 1``); returns ``{"beta", "iters", "time_elapsed"}``.

    The solution exists finitely if and only if ``||linear||_2 <= l1`` or ``||linear_S||_2 < l1`` on
    ``S = {i : quad_i + l2 = 0}``."""
    _solver_code(solver)
    quad, linear = np.asarray(quad), np.asarray(linear)
    if quad.ndim != 1 or linear.ndim != 1:
        raise TypeError("quad and linear must be 1-D.")
    out = solve_many(quad=quad[None], linear=linear[None], l1=l1, l2=l2, tol=tol, max_iters=max_iters, solver=solver)
    return {"beta": out["beta"][0], "iters": int(out["iters"][0]), "time_elapsed": out["time_elapsed"]}


def root(*, quad, linear, l1, tol=1e-12, max_iters=1000, solver="newton_abs"):
    """The non-negative root of :func:`root_function`, which exists only when ``||linear_S||_2 < l1 < ||linear||_2`` on
    ``S = {i : quad_i = 0}``; returns ``{"root", "iters"}`` with ``root`` ``None`` when it does not."""
    _solver_code(solver)
    quad, linear = np.asarray(quad), np.asarray(linear)
    if (np.linalg.norm(linear) <= l1) or (np.linalg.norm(linear[quad <= 0]) >= l1):
        return {"root": None, "iters": 0}
    out = solve(quad=quad, linear=linear, l1=l1, l2=0, tol=tol, max_iters=max_iters, solver=solver)
    return {"root": np.linalg.norm(out["beta"]), "iters": out["iters"]}
