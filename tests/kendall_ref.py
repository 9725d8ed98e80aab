"""TEST-ONLY reference of the rank correlation: the integers G = Z Z^T of Kendall's tau by brute force in numpy, and tau-b and
the skeptic matrix computed from them.  Z[i,(a,b)] = sign(x_ia - x_ib) over the sample pairs a < b; the loop takes one a (the
chunk of pairs (a, b > a)) at a time and sums the sign products in int64."""
import numpy as np


def counts_ref(X):
    X = np.asarray(X, dtype=np.float64)
    p, n = X.shape
    G = np.zeros((p, p), dtype=np.int64)
    for a in range(n - 1):
        Z = np.sign(X[:, a:a + 1] - X[:, a + 1:]).astype(np.int64)
        G += Z @ Z.T
    return G


def tau_ref(G):
    """tau-b = G_ij / sqrt(G_ii G_jj) (a constant variable gives nan / inf, as the definition does)."""
    d = np.diag(G).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return G / np.sqrt(np.outer(d, d))


def skeptic_ref(G):
    """sin(pi/2 tau-b) with the diagonal set to 1."""
    S = np.sin(np.pi / 2 * tau_ref(G))
    np.fill_diagonal(S, 1.0)
    return S


def make_data(p, N, kind, seed=0):
    """(p,N) test data.  'continuous': no ties; 'tied': values from {0,1,2} with each variable's own probabilities, so every
    variable has its own tie pattern (and at least two values); 'constant': tied data whose variable p // 2 is constant."""
    rng = np.random.default_rng([20250301, p, N, seed])
    if kind == 'continuous':
        return rng.standard_normal((p, N)) + 0.5 * rng.standard_normal((1, N))
    probs = rng.dirichlet(np.ones(3), size=p)
    X = np.stack([rng.choice(3, size=N, p=probs[i]) for i in range(p)]).astype(np.float64)
    for i in range(p):                                  # (no variable constant by chance)
        X[i, i % N], X[i, (i + 1) % N] = 0.0, 1.0 + i % 2
    if kind == 'constant':
        X[p // 2] = 1.0
    else:
        assert kind == 'tied'
    return X
