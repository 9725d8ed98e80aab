"""TEST-ONLY helpers of the glasso_problem tests: the oracle engine with the data entry points, and NumPy stand-ins for the
two device calls the class makes outside an engine (scaling by a diagonal, sample covariance), so that the class's host
logic runs without a GPU."""
import numpy as np

from oracle_engine import OracleEngine


class DataOracleEngine(OracleEngine):
    """OracleEngine + HipEngine.set_data / get_S (numpy.cov(bias=True) per instance)."""

    def set_data(self, X, N=None, center=True, scale=False):
        Xs = [np.asarray(x, dtype=np.float64) for x in X]
        assert len(Xs) == self.K and all(x.shape[0] == self.p for x in Xs)
        S, var = covariance_call_numpy(Xs, (1 if center else 0) | (2 if scale else 0))
        self.S, self._var = S, var

    def get_S(self):
        return self.S.copy() if getattr(self, "_var", None) is None else (self.S.copy(), self._var.copy())


def covariance_call_numpy(Xs, flags, device=0):
    """gglasso_amd.utils._covariance_call on the host."""
    S = []
    for x in Xs:
        xc = x - x.mean(axis=1, keepdims=True) if flags & 1 else x
        S.append(xc @ xc.T / x.shape[1])
    S = np.stack(S)
    if not flags & 2:
        return S, None
    var = np.stack([np.diag(s).copy() for s in S])
    return scale_by_diagonal_numpy(S, var)[0], var


def scale_by_diagonal_numpy(X, d=None, device=0):
    """gglasso_amd.ops._scale_by_diagonal on the host: (X_ij / (sqrt(d_i) sqrt(d_j)), d)."""
    X = np.asarray(X, dtype=np.float64)
    if d is None:
        d = np.diagonal(X, axis1=-2, axis2=-1).copy()
    d = np.asarray(d, dtype=np.float64)
    assert np.all(d > 0) and np.all(np.isfinite(d))
    s = np.sqrt(d)
    return X / (s[..., :, None] * s[..., None, :]), d


def on_host(monkeypatch):
    """Route every device call of gglasso_amd.problem to the oracle / NumPy."""
    from gglasso_amd import ops, solver, utils
    monkeypatch.setattr(solver, "ENGINE", DataOracleEngine)
    monkeypatch.setattr(ops, "_scale_by_diagonal", scale_by_diagonal_numpy)
    monkeypatch.setattr(utils, "_covariance_call", covariance_call_numpy)
