"""irbfn_amd -- MI355X-native (gfx950) implementation of the IRBFN hot path of hzheng40/irbfn.

Host side is Python (like the reference) over a C-ABI shared library of hand-written HIP kernels
(``libirbfn_hip.so``, ``include/irbfn_hip.h``).  The module names mirror the reference's:

* ``irbfn_amd.flax_rbf``      basis-function tokens (``gaussian``, ``inverse_quadratic`` ...)
* ``irbfn_amd.model``         ``WCRBFNet(**model_card).apply(params, x)``
* ``irbfn_amd.dynamics``      ``integrate_st_mult``, ``dynamic_st_onestep_aux``, ``integrate_frenet_mult``
* ``irbfn_amd.planner_utils`` ``integrate_path_mult``
* ``irbfn_amd.evaluate``      ``evaluate_table`` / ``rollout_errors``: roll-out error statistics of a net on a whole table
* ``irbfn_amd.kmeans``        ``fit`` / ``assign``: centres and cluster labels from a table (k-means on the device)
* ``irbfn_amd.widths``        ``nearest_neighbour`` / ``cluster_spread`` / ``select_scale``: RBF widths from the centres and the table
* ``irbfn_amd.linear_fit``    ``fit_linear``: the output layer in closed form (float64 normal equations on the device)
* ``irbfn_amd.ols``           ``select`` / ``fit_ols``: centres chosen by what they explain (OLS forward selection on the Gram matrix)
* ``irbfn_amd.loo``           ``factor`` / ``loo`` / ``leverage`` / ``select_ridge``: leave-one-out errors and leverages of the closed-form fit
* ``irbfn_amd.simulate``      ``Track`` / ``closed_loop``: B cars driven by a net along a race line, plant and way-point search on the device
* ``irbfn_amd.nmpc``          ``solve`` / ``make_table`` / ``closed_loop`` and their ``_frenet`` forms: batched NMPC solver (label tables, the MPC baseline of the closed loop)
* ``irbfn_amd.autograd``      ``torch.autograd`` wrappers (the ``jax.grad`` surface)
* ``irbfn_amd.distributed``   one-process-per-GPU sharding, RCCL broadcast of the parameters

There is no CPU fallback: every entry point raises if the HIP library or a GPU is missing.
"""
__version__ = "0.1.0"

from . import flax_rbf  # noqa: F401
from . import kmeans  # noqa: F401
from . import linear_fit  # noqa: F401
from . import ols  # noqa: F401
from . import widths  # noqa: F401
from . import loo  # noqa: F401
from . import simulate  # noqa: F401
from . import nmpc  # noqa: F401
from .model import WCRBFNet, pred_step  # noqa: F401
