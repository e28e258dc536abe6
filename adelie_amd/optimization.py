"""``adelie.optimization``: coordinate descents on ``min 1/2 x'Qx - v'x + pen(x)`` with ``Q`` a full ``(d, d)`` matrix, solved on
the device, and two small host routines.

* :class:`StateNNQPFull`, :class:`StateLassoFull`, :class:`StatePinballFull` have the reference's constructor arguments
  (``py_optimization.cpp``), checks and messages (``nnqp_full.hpp:43-64``, ``lasso_full.hpp:44-70``, ``pinball_full.hpp:50-80``).
  ``.solve()`` runs the reference's cyclic coordinate descent in a HIP kernel (``csrc/kernels_qp_full.hip``) and updates the
  caller's ``x`` and ``grad`` in place; ``grad`` must hold ``v - Q x`` on entry and does on exit.  Every operation of a visit is
  the reference's, in its order and in ``quad``'s dtype, so the result has the bits of the scalar loop.
* :func:`solve_many` solves a list of states of one class and dtype -- of any mix of dimensions -- in one native call: a
  wavefront per problem with ``d <= 64``, a workgroup per larger one.  Many small problems at once is the shape at which the
  device earns its keep on them.
* ``quad`` may be a torch tensor in device memory (float32 / float64, F- or C-contiguous); it is read in place, as
  ``matrix.dense`` adopts one, and only the vectors cross PCIe.
* :func:`search_pivot` and :func:`symmetric_penalty` restate ``search_pivot.hpp`` and ``symmetric_penalty.hpp`` in numpy: O(n)
  scalar host routines with nothing in them for a device.

Out of scope, on purpose: ``StateLinQPFull`` (a log-barrier Newton method with a Cholesky factorisation per step, which nothing in
the reference's solvers calls: a different kernel, so the name is left undefined here rather than routed to numpy); the signed
NNQP variant, which the reference's Python does not export either; and the constraint objects, which keep their own device code
and are not rewired onto this kernel.
"""
import bisect

import numpy as np

from . import _abi

__all__ = ["StateNNQPFull", "StateLassoFull", "StatePinballFull", "solve_many", "search_pivot", "symmetric_penalty"]

_KIND_NNQP, _KIND_LASSO, _KIND_PINBALL = (_abi.QP_FULL_KIND[k] for k in ("nnqp", "lasso", "pinball"))


def _solver_error(msg):
    return RuntimeError("adelie_core solver: " + msg)


def _is_torch(a):
    return not isinstance(a, np.ndarray) and type(a).__module__.startswith("torch")


class _StateFull:
    """What the three states share: the adopted arguments, the reference's checks and the native call."""

    _kind = None
    _penalties = ()

    def _init(self, quad, penalties, y_var, max_iters, tol, x, grad):
        if _is_torch(quad):
            if quad.dim() != 2 or not quad.is_cuda:
                raise TypeError("quad: a torch tensor must be 2-D and in device memory.")
            try:
                dtype = np.dtype({"torch.float64": np.float64, "torch.float32": np.float32}[str(quad.dtype)])
            except KeyError:
                raise TypeError("quad must be float32 or float64.") from None
            rows, cols = (int(v) for v in quad.shape)
            if not (quad.is_contiguous() or quad.t().is_contiguous()):
                raise TypeError("quad must be F- or C-contiguous.")
            self._quad_ptr, self._quad_dev, self._device = int(quad.data_ptr()), True, quad.device.index or 0
        else:
            if not isinstance(quad, np.ndarray) or quad.ndim != 2 or quad.dtype not in (np.float32, np.float64):
                raise TypeError("quad must be a 2-D float32 or float64 ndarray (or a torch tensor in device memory).")
            if not (quad.flags.f_contiguous or quad.flags.c_contiguous):
                raise TypeError("quad must be F- or C-contiguous.")
            dtype = quad.dtype
            rows, cols = quad.shape
            self._quad_ptr, self._quad_dev, self._device = quad.ctypes.data, False, None
        self._quad, self._dtype = quad, np.dtype(dtype)

        def vec(name, v, out):
            if not isinstance(v, np.ndarray) or v.ndim != 1 or v.dtype != self._dtype:
                raise TypeError(f"{name} must be a 1-D ndarray of quad's dtype ({self._dtype}).")
            if out and not v.flags.writeable:
                raise TypeError(f"{name} must be writable.")
            if not v.flags.c_contiguous:
                raise TypeError(f"{name} must be contiguous.")
            return v

        pens = [vec(n, v, False) for n, v in zip(self._penalties, penalties)]
        x, grad = vec("x", x, True), vec("grad", grad, True)
        max_iters = int(max_iters)
        if max_iters < 0:
            raise TypeError("max_iters must be non-negative.")
        tol = float(self._dtype.type(tol))
        # the reference's checks, in its order
        d = rows
        if cols != d:
            raise _solver_error("quad must be (d, d). ")
        for n, v in zip(self._penalties, pens):
            if v.size != d:
                raise _solver_error(f"{n} must be (d,) where quad is (d, d). ")
        if tol < 0:
            raise _solver_error("tol must be >= 0.")
        if x.size != d:
            raise _solver_error("x must be (d,) where quad is (d, d). ")
        if grad.size != d:
            raise _solver_error("grad must be (d,) where quad is (d, d). ")
        self._pens, self._x, self._grad = pens, x, grad
        self._y_var = None if y_var is None else float(self._dtype.type(y_var))
        self._max_iters, self._tol = max_iters, tol
        self._iters, self._time_elapsed = 0, 0.0

    quad = property(lambda self: self._quad)
    max_iters = property(lambda self: self._max_iters)
    tol = property(lambda self: self._tol)
    x = property(lambda self: self._x)
    grad = property(lambda self: self._grad)
    iters = property(lambda self: self._iters)
    time_elapsed = property(lambda self: self._time_elapsed)

    @classmethod
    def _max_iters_message(cls):
        return f"adelie_core solver: {cls.__name__}: max iterations reached!"

    def solve(self, *, device=0):
        """Runs the descent from the current ``x`` / ``grad``, which are updated in place."""
        if _run([self], device)[0]:
            raise RuntimeError(self._max_iters_message())


class StateNNQPFull(_StateFull):
    """``min 1/2 x'Qx - v'x  s.t.  x >= 0``; a sweep ends the solve when ``max_i q_ii del_i^2 < d * tol``."""

    _kind = _KIND_NNQP

    def __init__(self, quad, max_iters, tol, x, grad):
        self._init(quad, (), None, max_iters, tol, x, grad)


class StateLassoFull(_StateFull):
    """``min 1/2 x'Qx - v'x + sum_i penalty_i |x_i|``; a sweep ends the solve when ``max_i q_ii del_i^2 < tol``."""

    _kind = _KIND_LASSO
    _penalties = ("penalty",)

    def __init__(self, quad, penalty, max_iters, tol, x, grad):
        self._init(quad, (penalty,), None, max_iters, tol, x, grad)

    penalty = property(lambda self: self._pens[0])


class StatePinballFull(_StateFull):
    """``min 1/2 x'Qx - v'x + sum_i penalty_pos_i max(x_i, 0) + penalty_neg_i max(-x_i, 0)``; a sweep ends the solve when
    ``max_i q_ii del_i^2 < y_var * tol``."""

    _kind = _KIND_PINBALL
    _penalties = ("penalty_neg", "penalty_pos")

    def __init__(self, quad, penalty_neg, penalty_pos, y_var, max_iters, tol, x, grad):
        self._init(quad, (penalty_neg, penalty_pos), y_var, max_iters, tol, x, grad)

    penalty_neg = property(lambda self: self._pens[0])
    penalty_pos = property(lambda self: self._pens[1])
    y_var = property(lambda self: self._y_var)


def _run(states, device):
    """One native call over `states` (one class, one dtype); returns the per-state "stopped at max_iters" flags."""
    C = _abi.C
    n = len(states)
    first = states[0]
    for s in states:
        if s._device is not None:
            device = s._device
            break
    for s in states:
        if s._device is not None and s._device != device:
            raise RuntimeError("every adopted quad of a batch must live on one device.")
    i64 = np.int64
    d = np.array([s._x.size for s in states], dtype=i64)
    ptrs = lambda vals: np.array(vals, dtype=np.uint64)
    quad = ptrs([s._quad_ptr for s in states])
    is_dev = np.array([s._quad_dev for s in states], dtype=np.uint8)
    npen = len(first._penalties)
    pa = ptrs([s._pens[0].ctypes.data for s in states]) if npen >= 1 else None
    pb = ptrs([s._pens[1].ctypes.data for s in states]) if npen >= 2 else None
    x = ptrs([s._x.ctypes.data for s in states])
    g = ptrs([s._grad.ctypes.data for s in states])
    tol = np.array([s._tol for s in states], dtype=np.float64)
    y_var = np.array([s._y_var for s in states], dtype=np.float64) if first._kind == _KIND_PINBALL else None
    max_iters = np.array([s._max_iters for s in states], dtype=i64)
    iters = np.zeros(n, dtype=i64)
    status = np.zeros(n, dtype=np.int32)
    elapsed = C.c_double(0.0)
    args = _abi.QpFullArgs(
        kind=first._kind, dtype=_abi.dtype_code(first._dtype), device=int(device), _pad0=0, n_problems=n,
        d=_abi.ptr(d), quad=_abi.ptr(quad), quad_is_dev=_abi.ptr(is_dev), penalty_a=_abi.ptr(pa), penalty_b=_abi.ptr(pb),
        x=_abi.ptr(x), grad=_abi.ptr(g), tol=_abi.ptr(tol), y_var=_abi.ptr(y_var), max_iters=_abi.ptr(max_iters),
        iters=_abi.ptr(iters), status=_abi.ptr(status), time_elapsed=C.cast(C.pointer(elapsed), C.c_void_p))
    backend = _abi.hip_backend()
    backend.check(backend.fn("qp_full_solve")(C.byref(args)))
    for k, s in enumerate(states):
        s._iters = int(iters[k])
        s._time_elapsed = elapsed.value / n
    return [int(v) == _abi.QP_FULL_MAX_ITERS for v in status]


def solve_many(states, *, device=0):
    """Solves every state of the list in one native call; each ends as its own ``.solve()`` would have left it.

    The states must be of one class and one dtype; their dimensions may differ.  If any stopped at ``max_iters`` one
    ``RuntimeError`` naming their (0-based) positions is raised after all states are filled in.  Each state's ``time_elapsed`` is
    the batch's time over the batch's size.  An empty list is a no-op.
    """
    states = list(states)
    if not states:
        return
    cls, dtype = type(states[0]), states[0]._dtype if isinstance(states[0], _StateFull) else None
    for s in states:
        if not isinstance(s, _StateFull) or type(s) is not cls:
            raise TypeError("solve_many: the states must be of one class (StateNNQPFull, StateLassoFull or StatePinballFull).")
        if s._dtype != dtype:
            raise TypeError("solve_many: the states must be of one dtype.")
    if len({id(s) for s in states}) != len(states):
        raise RuntimeError("solve_many: a state appears twice.")
    failed = [k for k, f in enumerate(_run(states, device)) if f]
    if failed:
        raise RuntimeError(f"{cls._max_iters_message()} (states {failed})")


def search_pivot(x, y):
    """``(argmin, mses)`` of the piecewise-linear fit ``y = b0 + b1 (p - x) 1(x <= p)`` over the pivots ``p = x[i]``
    (``search_pivot.hpp:18-62``): ``x`` increasing, ``mses[i]`` the (shifted) error with pivot ``x[i]``, ``mses[0] = inf``."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = x.size
    mses = np.empty(n)
    if n <= 0:
        return -1, mses
    mses[0] = np.inf
    if n == 1:
        return 0, mses
    y_mean = float(np.mean(y))
    x_sum, xsq_sum, y_sum, yx_sum = float(x[0]), float(x[0] * x[0]), float(y[0]), float(y[0] * x[0])
    min_mse, argmin = np.inf, 0
    for i in range(1, n):
        xi, yi = float(x[i]), float(y[i])
        x_sum += xi
        xsq_sum += xi * xi
        y_sum += yi
        yx_sum += yi * xi
        t_bar = ((i + 1) * xi - x_sum) / n
        var_t = (i + 1) * xi * xi - 2 * xi * x_sum + xsq_sum - n * t_bar * t_bar
        cov_ty = xi * (y_sum - (i + 1) * y_mean) - (yx_sum - y_mean * x_sum)
        with np.errstate(divide="ignore", invalid="ignore"):
            beta1_hat = float(np.float64(cov_ty) / np.float64(var_t))
        mses[i] = -beta1_hat * beta1_hat * var_t
        if mses[i] < min_mse:
            argmin, min_mse = i, mses[i]
    return argmin, mses


def symmetric_penalty(x, alpha):
    """The minimiser ``t`` of ``sum_i (1 - alpha) / 2 (x_i - t)^2 + alpha |x_i - t|`` for increasing ``x`` and ``alpha`` in
    [0, 1] (``symmetric_penalty.hpp:16-94``)."""
    knots = np.ascontiguousarray(x, dtype=np.float64)
    alpha = float(alpha)
    K = knots.size
    if K <= 0:
        return 0.0
    med = float(0.5 * (knots[K // 2 - 1] + knots[K // 2])) if K % 2 == 0 else float(knots[K // 2])
    if alpha >= 1:
        return med
    mean = float(np.mean(knots))
    if alpha <= 0:
        return mean
    a_left, a_right = min(med, mean), max(med, mean)
    if a_right <= a_left:
        return a_left
    a_begin = bisect.bisect_left(knots, a_left)
    a_end = bisect.bisect_left(knots, a_right, lo=a_begin)
    sq_mean = float(np.mean(knots * knots))
    alpha_ratio = alpha / (1 - alpha)

    def quad_min(i, lower, upper, partial_mean):
        t_star = mean + alpha_ratio * (1 - 2 * i / K)
        argmin = lower if t_star <= lower else (t_star if t_star <= upper else upper)
        return argmin, argmin * (argmin - 2 * t_star) + sq_mean + 2 * alpha_ratio * partial_mean

    partial_mean = mean - 2 * float(np.sum(knots[:a_begin])) / K
    argmin, f_min = quad_min(a_begin, a_left, float(knots[a_begin]), partial_mean)
    for i in range(a_begin + 1, a_end):
        partial_mean -= 2 * float(knots[i - 1]) / K
        cur_argmin, cur_f_min = quad_min(i, float(knots[i - 1]), float(knots[i]), partial_mean)
        if cur_f_min > f_min:
            return argmin
        argmin, f_min = cur_argmin, cur_f_min
    partial_mean -= 2 * float(knots[a_end - 1]) / K
    cur_argmin, cur_f_min = quad_min(a_end, float(knots[a_end - 1]), a_right, partial_mean)
    return argmin if cur_f_min > f_min else cur_argmin
