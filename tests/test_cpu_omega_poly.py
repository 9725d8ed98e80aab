"""The direct family of the Omega-step (GGL_OPT_OMEGA_POLY): Omega = W/2 + (sqrt(c)/2) p(X), one polynomial in A' = W^2 + 4 beta I
evaluated by Paterson-Stockmeyer in products of commuting symmetric matrices (csrc/newton_schulz.hip, ns_plan).  Host only: the
plan comes from ggl_dev_omega_poly_plan, the launch chain is emulated in NumPy with the coefficients the device launches get,
in the I / A' / B' form of the product epilogues."""
import ctypes

import numpy as np
import pytest

from gglasso_amd import _lib as lib

TOLS = (1e-9, 2e-12)


def plan(a, tol, degrees=9):
    deg, units = ctypes.c_int(), ctypes.c_int()
    out = (ctypes.c_double * 18)()
    taken = lib.load().ggl_dev_omega_poly_plan(float(a), float(tol), int(degrees), ctypes.byref(deg), out, ctypes.byref(units))
    assert taken in (0, 1)
    return taken, deg.value, np.array(out[:16]), units.value, out[16], out[17]


def launch_coefs(co, d, aq, c):
    """ns_plan's rows for one instance with bound c: start {A', B', I} of G, then per launch {cI, cAcc, cE(B'), cE2(A'),
    dI, dC, dE(B'), dE2(A')} (the last launch: {0, sqrt(c)/2, E = G})."""
    J = d // 3
    m, h = 0.5 * (1 + aq), 0.5 * (1 - aq)
    u, hc = 1.0 / h ** 3, 0.5 * np.sqrt(c)

    def digit(j):
        a0, a1, a2 = co[3 * j], co[3 * j + 1], co[3 * j + 2]
        return (a0 - a1 * (m / h) + a2 * (m / h) * (m / h), a1 / (c * h) - 2.0 * a2 * m / (c * h * h), a2 / (c * c * h * h))

    al, be, ga = digit(0)
    start = (hc * be, hc * ga, hc * al)
    al, be, ga = digit(J - 1)
    rows = [dict(cI=-m ** 3 * u, cAcc=u / c ** 3, cE=-3 * m * u / c ** 2, cE2=3 * m * m * u / c, dI=al, dC=co[3 * J], dE=ga, dE2=be)]
    for j in range(J - 2, 0, -1):
        al, be, ga = digit(j)
        rows.append(dict(cI=al, cAcc=1.0, cE=ga, cE2=be))
    rows.append(dict(cI=0.0, cAcc=hc, cE=1.0))
    return start, rows


def emulate(W, beta, c, co, d, aq):
    """the launch chain of ns_run's direct branch on one matrix (or on eigenvalues: W diagonal as a vector)"""
    vec = W.ndim == 1
    I = np.ones_like(W) if vec else np.eye(len(W))
    mul = (lambda x, y: x * y) if vec else (lambda x, y: x @ y)
    Ap = mul(W, W) + 4 * beta * I
    Bp = mul(Ap, Ap)
    start, rows = launch_coefs(co, d, aq, c)
    G = 0.5 * W + start[0] * Ap + start[1] * Bp + start[2] * I
    r = rows[0]
    Y = r["cAcc"] * mul(Ap, Bp) + r["cE"] * Bp + r["cE2"] * Ap + r["cI"] * I
    H = r["dC"] * Y + r["dE"] * Bp + r["dE2"] * Ap + r["dI"] * I
    for r in rows[1:-1]:
        H = r["cAcc"] * mul(H, Y) + r["cE"] * Bp + r["cE2"] * Ap + r["cI"] * I
    r = rows[-1]
    return r["cAcc"] * mul(H, Y) + r["cE"] * G


@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("a", [0.3, 0.4, 0.5, 0.55, 0.6, 0.7, 0.8, 0.9, 0.95])
def test_chain_error_on_grid_and_matrices(a, tol):
    taken, d, co, units, aq, err = plan(a, tol)
    if d == 0:
        assert taken == 0 and units == -1
        return
    assert d in (6, 9, 12, 15) and units == 2 + d // 3 and 0.0 < aq <= a and err + 2e-14 <= tol
    beta = 0.25
    c = 4 * beta / a                                     # lambda_min(A') / c = a: the interval's left end is reached
    # eigenvalues: A' = w^2 + 4 beta over the whole interval [a c, c] (dense grid), Omega = phiplus(w)
    s = np.linspace(a, 1.0, 20001)
    w = np.sqrt(np.maximum(s * c - 4 * beta, 0.0)) * np.where(np.arange(s.size) % 2, 1.0, -1.0)
    om = emulate(w, beta, c, co, d, aq)
    ref = 0.5 * (w + np.sqrt(w * w + 4 * beta))
    assert np.max(np.abs(om - ref)) <= tol * np.sqrt(c) / 2
    # random symmetric W with that spectrum of A', against an eigh square root
    rng = np.random.default_rng(int(a * 1000) + int(-np.log10(tol)))
    p = 60
    Q, _ = np.linalg.qr(rng.standard_normal((p, p)))
    sv = np.concatenate([[a, 1.0], rng.uniform(a, 1.0, p - 2)])
    wv = np.sqrt(np.maximum(sv * c - 4 * beta, 0.0)) * rng.choice([-1.0, 1.0], p)
    W = (Q * wv) @ Q.T
    W = 0.5 * (W + W.T)
    d_, V = np.linalg.eigh(W)
    ref = (V * (0.5 * (d_ + np.sqrt(d_ * d_ + 4 * beta)))) @ V.T
    Ap = W @ W + 4 * beta * np.eye(p)
    lam = np.linalg.eigvalsh(Ap)
    om = emulate(W, beta, c, co, d, aq)
    assert np.linalg.norm(om - ref, 2) <= tol * np.sqrt(lam[-1]) / 2 * 1.05 + 1e-13


def test_choice_rule():
    L = lib.load()
    for a in np.linspace(0.3, 0.95, 27):
        for tol in (1e-9, 2e-12, 1e-12, 0.0):
            taken, d, co, units, aq, err = plan(a, tol)
            ns = L.ggl_dev_ns_units(float(np.sqrt(a)), 9, float(tol))
            # strictly cheaper only; ties and wider intervals keep Newton-Schulz
            assert taken == (1 if (d > 0 and ns > 0 and units < ns) else 0), (a, tol, d, units, ns)
            if tol == 0.0:
                assert taken == 0 and d == 0            # 4e-16 is below the evaluation floor
    for a in np.linspace(0.50, 0.62, 13):
        taken, d, co, units, aq, err = plan(a, 2e-12)
        assert taken == 1 and units == 6 and d == 12, (a, d, units)


def test_plan_is_a_function_of_the_quantised_interval():
    # the same key from any point of the quantisation cell, in any order of queries and tolerances
    r1 = plan(0.55, 2e-12)
    plan(0.7, 1e-9)
    r2 = plan(0.55, 2e-12)
    assert r1[0] == r2[0] and r1[1] == r2[1] and np.array_equal(r1[2], r2[2]) and r1[4] == r2[4]
    aq = r1[4]
    r3 = plan(aq * 1.0000001, 2e-12)
    assert r3[4] == aq and np.array_equal(r3[2], r1[2])
