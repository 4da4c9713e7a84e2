"""pysparselp_amd: the first-order sparse-LP hot path of PySparseLP on AMD MI355X.

``SparseLP.solve(method="admm" | "chambolle_pock_ppd" | "admm_blocks")`` with the reference's
signature (modules mirror the reference's: ``SparseLP``, ``ADMM``, ``ChambollePockPPD``, ``ADMMBlocks``,
``gaussSiedel``, ``MPSparser``, ``netlib``, ``tools``; ``device`` / ``scale`` / ``problems`` / ``parallel`` hold the
device-resident, at-scale and multi-GPU entry points); the inner loops run in hand-written HIP kernels (libslp_hip.so,
C ABI in include/slp_hip.h).  ``SparseLP.solve_batch`` / ``chambolle_pock_ppd_batch`` solve many cost vectors over one
constraint matrix together (Chambolle-Pock, all instances per launch; ``SparseLP.solve_batch_certified`` /
``chambolle_pock_ppd_batch_certified`` stop every instance on its own, by a certified duality gap and the primal violation evaluated on
the device, both handed back); ``SparseLP.solve_admm_batch`` / ``lp_admm_batch``
do the same for ADMM with the projected Gauss-Seidel x-step (``SparseLP.solve_admm_batch_until`` / ``lp_admm_batch_until`` stop every
instance on its own, by a test on the residual and the step inside the kernels), ``SparseLP.solve_dga_batch`` / ``dual_gradient_ascent_batch`` for dual
gradient ascent (certified lower bounds of B LPs over one matrix; ``SparseLP.solve_dga_batch_until`` /
``dual_gradient_ascent_batch_until`` stop every instance on its own, on the step of its multipliers or once its bound has reached a
cut-off, tested on the device); ``SparseLP.solve_dga_batch_rhs`` / ``dual_gradient_ascent_batch_rhs`` and
``SparseLP.solve_admm_batch_rhs`` / ``lp_admm_batch_rhs`` give every instance right-hand sides of its own as well
(``DeviceDGABatch.set_rhs``, ``ADMMBatchState.set_rhs``), with or without those stopping tests; ``solve_many`` / ``chambolle_pock_ppd_many`` solve a list of
LPs whose matrices differ, one workgroup per LP (Chambolle-Pock; ``solve_many_until`` / ``chambolle_pock_ppd_many_until`` stop every
LP on its own, by a test on the step inside the kernel; ``solve_many_certified`` / ``chambolle_pock_ppd_many_certified`` by a
certified duality gap and the primal violation, both handed back), ``solve_dga_many`` / ``dual_gradient_ascent_many`` do the same
for dual gradient ascent (a certified lower bound per LP; ``solve_dga_many_until`` / ``dual_gradient_ascent_many_until`` stop every
LP on its own, by a test on the step of its multipliers inside the kernel; ``solve_dga_many_cutoff`` /
``dual_gradient_ascent_many_cutoff`` also once its bound has reached a cut-off; ``solve_dga_many_compact`` /
``dual_gradient_ascent_many_compact`` are those with the LPs still moving handed consecutive workgroups in every launch), ``solve_admm_many`` / ``lp_admm_many`` for ADMM with the projected
Gauss-Seidel x-step (``solve_admm_many_until`` / ``lp_admm_many_until`` stop every LP on its own, by a test on the residual and
the step inside the kernel).  ``CPManyState.set_compaction`` / ``ADMMManyState.set_compaction`` make every launch of an armed
list state run over the LPs not yet stopped, with the same results bit for bit.  ``SparseLP.solve_certified`` /
``chambolle_pock_ppd_certified`` stop the single Chambolle-Pock solver, on every format and row-partitioned over ranks, on that
certified duality gap (``CPState.set_stop_gap`` / ``DeviceCP.set_stop_gap``, ``certificate``, ``gap_state``).
``SparseLP.solve_admm_certified`` / ``lp_admm_certified`` do the same for the two single ADMM solvers, with a multiplier repaired
into a dual feasible vector (``ADMMState`` / ``ADMMCGState`` / ``ADMMCGLPState`` / ``DeviceADMM`` ``.set_stop_gap``,
``.certificate``, ``.gap_state``).  There is no CPU fallback: without the built
library and a HIP device every solver call raises ``SlpError``.
"""
from ._lib import ORDER_AUTO, ORDER_SEQUENTIAL, ORDER_TREE, SlpError  # noqa: F401
from .ADMM import ADMMBatchState, ADMMManyState, lp_admm_batch, lp_admm_batch_until, lp_admm_many, lp_admm_many_until  # noqa: F401
from .ADMM import lp_admm_batch_rhs  # noqa: F401
from .ChambollePockPPD import (CPBatchState, CPManyState, chambolle_pock_ppd_batch, chambolle_pock_ppd_batch_certified,  # noqa: F401
                               chambolle_pock_ppd_many, chambolle_pock_ppd_many_certified, chambolle_pock_ppd_many_until)
from .DualGradientAscent import (DeviceDGABatch, DeviceDGAMany, dual_gradient_ascent_batch, dual_gradient_ascent_batch_until,  # noqa: F401
                                 dual_gradient_ascent_many, dual_gradient_ascent_many_compact, dual_gradient_ascent_many_cutoff,
                                 dual_gradient_ascent_many_until)
from .DualGradientAscent import dual_gradient_ascent_batch_rhs  # noqa: F401
from .SparseLP import solve_admm_many, solve_admm_many_until, solve_dga_many, solve_dga_many_until, solve_many, solve_many_until  # noqa: F401
from .SparseLP import solve_dga_many_compact, solve_dga_many_cutoff, solve_many_certified  # noqa: F401
from .ChambollePockPPD import chambolle_pock_ppd_certified  # noqa: F401
from .ADMM import lp_admm_certified  # noqa: F401

__all__ = ["ORDER_AUTO", "ORDER_SEQUENTIAL", "ORDER_TREE", "SlpError", "CPBatchState", "chambolle_pock_ppd_batch",
           "ADMMBatchState", "lp_admm_batch", "DeviceDGABatch", "dual_gradient_ascent_batch", "CPManyState", "chambolle_pock_ppd_many",
           "solve_many", "DeviceDGAMany", "dual_gradient_ascent_many", "solve_dga_many", "ADMMManyState", "lp_admm_many",
           "solve_admm_many", "chambolle_pock_ppd_many_until", "solve_many_until", "lp_admm_many_until", "solve_admm_many_until",
           "dual_gradient_ascent_many_until", "solve_dga_many_until", "chambolle_pock_ppd_many_certified", "solve_many_certified",
           "chambolle_pock_ppd_batch_certified", "lp_admm_batch_until", "dual_gradient_ascent_batch_until",
           "dual_gradient_ascent_many_cutoff", "solve_dga_many_cutoff", "dual_gradient_ascent_many_compact", "solve_dga_many_compact",
           "dual_gradient_ascent_batch_rhs", "lp_admm_batch_rhs", "chambolle_pock_ppd_certified", "lp_admm_certified"]
