"""smcp_amd -- MI355X-native chordal cone-program Newton-KKT kernels behind SMCP's API.

Only the hot path of cvxopt/smcp is implemented natively (HIP, gfx950): the chordal
multifrontal kernels (cholesky, completion, projected_inverse, hessian, llt, trsm, dot) and
the KKT/Schur-complement layer around them.  The interior-point drivers stay in Python.
"""
from .symbolic import Symbolic, symbolic, maxcardsearch, mindegree  # noqa: F401
from .cspmatrix import cspmatrix  # noqa: F401
from . import base, solvers  # noqa: F401
from .base import SDP, band_SDP, mtxnorm_SDP, completion  # noqa: F401  (smcp.__init__: same four names)
from .base import mrcompletion, maxcut_round, edmcompletion, psdcompletion  # noqa: F401
from .base import cone_margin, max_step  # noqa: F401  (scipy matrices; the cspmatrix forms are smcp_amd.chordal.cone_margin / max_step)
from .base import dual_max_step, dual_margin  # noqa: F401  (scipy matrices; the cspmatrix forms are smcp_amd.chordal.dual_max_step / dual_margin)
from .chordal import cholesky, projected_inverse, hessian, llt, trsm, trmm, syr2k, syrk, syr2, symm, dot, logdiagsum, lowrank_factor, LowRankFactor  # noqa: F401
from .chordal import clique_eigvalsh, clique_extremes  # noqa: F401
from .chordal import clique_ptr, clique_block, clique_gather, clique_scatter, clique_multiplicity, clique_eigh, clique_project  # noqa: F401
from .base import cone_project  # noqa: F401  (scipy matrices; the cspmatrix form is smcp_amd.chordal.cone_project)
from .base import chol_update  # noqa: F401  (V in the original order; the device form is smcp_amd.chordal.chol_update)
from .chordal import clique_support  # noqa: F401
from .base import clique_decompose  # noqa: F401  (scipy matrices; the cspmatrix form is smcp_amd.chordal.clique_decompose)
# the CHOMPACK-level in-place completion (factor of the inverse) is smcp_amd.chordal.completion

__version__ = "0.1.0"
