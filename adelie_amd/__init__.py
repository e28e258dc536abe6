"""adelie_amd — an MI355X-native group-elastic-net path solver behind adelie's Python API.

Mirrors the user-facing surface of JamesYang007/adelie for the ``grpnet`` hot path only
(``solver.grpnet``, ``cv.cv_grpnet``, ``matrix.dense`` / ``matrix.snp_unphased`` / ``matrix.kronecker_eye``,
``glm.gaussian`` / ``glm.binomial`` / ``glm.multigaussian`` / ``glm.multinomial``, the naive State objects), the covariance
method (``solver.gaussian_cov``), the pin solvers on a fixed screen set (``state.gaussian_pin_naive`` /
``state.gaussian_pin_cov``), column subset selection on a resident covariance (``solver.css_cov``,
``sklearn.CSSModelSelection``), bounded-variable least squares (``solver.bvls``) and pinball least squares on a resident
constraint matrix (``solver.pinball``, ``matrix.dense(method="constraint")``), and the full-matrix NNQP / lasso / pinball
descents, one or a batch per call (``optimization.StateNNQPFull`` / ``StateLassoFull`` / ``StatePinballFull``,
``optimization.solve_many``).  All numerics run in hand-written HIP
kernels for gfx950 behind the C ABI declared in ``include/adelie_hip.h``.
"""
from . import configs
from . import constraint
from . import glm
from . import matrix
from . import state
from . import solver
from . import diagnostic
from . import cv
from . import data
from . import io
from . import optimization
try:  # the estimator wrapper needs scikit-learn's base classes; everything else does not
    from . import sklearn
except ImportError:  # pragma: no cover
    pass
from .configs import set_configs
from .cv import cv_grpnet
from .solver import bvls, css_cov, gaussian_cov, grpnet, pinball

__version__ = "0.1.0"
