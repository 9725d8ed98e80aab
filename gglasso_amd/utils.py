"""Utilities of the Functional Graphical Lasso on the device (reference: helper/utils.py:69-107 of fabian-sp/GGLasso)."""
import numpy as np

from . import _lib
from ._lib import as_c, check, ptr


def frob_norm_per_block(S, M, off_diag=False):
    """helper/utils.py:69-87: the (p,p) table of Frobenius norms of the M x M blocks of the (pM,pM) matrix S (the upper
    blocks decide, the lower ones mirror them); ``off_diag``: zero diagonal."""
    S = as_c(S)
    assert S.ndim == 2 and S.shape[0] == S.shape[1]
    pM = S.shape[0]
    assert pM % M == 0
    p = pM // int(M)
    out = np.empty((p, p))
    _lib.require_gpu()
    check(_lib.load().ggl_frob_norm_per_block(pM, int(M), ptr(S), int(bool(off_diag)), ptr(out)))
    return out


def lambda_max_fsgl(S, M):
    """helper/utils.py:89-107: the smallest lambda1 for which every off-diagonal block of the FSGL solution is zero,
    max_{j != l} |S^M_jl|_F."""
    return frob_norm_per_block(S, M, off_diag=True).max()
