"""The batched epilogue of the direct-to-LDS product kernels (csrc/gemm_sym.hip symm_dl_tile: the E / E2 loads of a batch of
trips issued together, one wait, the mirror pass fed from the staged tile) against the serial epilogue, which the
development library keeps behind ggl_dev_set_symm_epilogue(1): the same bits, everywhere.

Kernel level (ggl_dev_symm, ggl_dev_symm_full, ggl_dev_symm_bounds): the 64x64 kernels (16, 17), the 32x32 kernel (20) and the eight-wave
instances (22, 23), with E and the second output, with E alone, without E, with E, E2 and every coefficient; shapes, one purpose each: (2, 64) a single diagonal
tile, (2, 130) diagonal, off-diagonal and a two-column edge tile at BM = 64, (3, 129) odd p (the last column as half a pair),
(2, 200), (9, 70) the XCD remainder dealing, (1, 500) the headline's tile grid.  Every variant of the development library that
is not a timing ablation, at (3, 130) and (2, 97): a symmetric C within rounding of numpy's, bound partials that are C's.
Step level (ggl_admm_step, where E2 and the fused second output exist): 8 iterations of (8, 301) at ns_tol 1e-9 and of
(16, 400) with every speculation missed, both epilogues, every iterate and the five norms of every step."""
import numpy as np
import pytest

SHAPES = [(2, 64), (2, 130), (3, 129), (2, 200), (9, 70), (1, 500)]
VARIANTS = [16, 17, 20, 22, 23]


def _both(dev, fn):
    """fn() under the batched and under the serial epilogue; the switch is restored"""
    out = []
    was = dev.ggl_dev_set_symm_epilogue(0)
    try:
        for serial in (0, 1):
            dev.ggl_dev_set_symm_epilogue(serial)
            out.append(fn())
    finally:
        dev.ggl_dev_set_symm_epilogue(was)
    return out


def _sym(rng, K, p):
    X = rng.standard_normal((K, p, p))
    return 0.5 * (X + X.transpose(0, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("K,p", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_kernel_bitwise(dev_library, variant, K, p):
    from gglasso_amd import _lib
    from gglasso_amd._lib import ptr
    rng = np.random.default_rng(1000 * variant + p)
    A, B, E = _sym(rng, K, p), _sym(rng, K, p), _sym(rng, K, p)       # E bitwise symmetric, as every E of the solvers is
    coef = np.ascontiguousarray(rng.uniform(0.5, 1.5, (K, 5)))

    def run(with_e, with_c2):
        def call():
            C = np.full_like(A, np.nan)
            C2 = np.full_like(A, np.nan) if with_c2 else None
            _lib.check(dev_library.ggl_dev_symm(K, p, ptr(A), ptr(B), ptr(E) if with_e else None, ptr(coef), ptr(C),
                                                ptr(C2) if with_c2 else None, variant))
            return C, C2
        return call

    for with_e, with_c2 in ((True, True), (True, False), (False, False)):
        (Cb, C2b), (Cs, C2s) = _both(dev_library, run(with_e, with_c2))
        assert np.isfinite(Cs).all()
        assert np.array_equal(Cb, Cs), (with_e, with_c2, float(np.abs(Cb - Cs).max()))
        if with_c2:
            assert np.isfinite(C2s).all()
            assert np.array_equal(C2b, C2s), (with_e, float(np.abs(C2b - C2s).max()))
    # the yardstick itself: the serial epilogue's last result (no E) is cI I + cAcc A B on the upper triangle
    iu = np.triu_indices(p)
    ref = coef[:, 0, None, None] * np.eye(p)[None] + coef[:, 1, None, None] * (A @ B)
    assert np.abs(Cs[:, iu[0], iu[1]] - ref[:, iu[0], iu[1]]).max() <= 1e-12 * np.abs(ref).max() * p


def _same_bits(x, y):
    """stricter than array_equal: the sign of a zero counts"""
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("K,p", [(2, 130), (3, 129), (1, 500)])
@pytest.mark.parametrize("variant", [16, 17, 20, 22])
def test_kernel_every_operand_bitwise(dev_library, variant, K, p):
    """ggl_dev_symm_full: E, E2 and the second output with dE, dE2 != 0 -- the mirror pass's own batched loads of E / E2 (and
    their half-column shift for odd p), which ggl_dev_symm's five coefficients leave out -- and with dE = dE2 = 0, where the
    serial epilogue still multiplies the loaded values by zero."""
    from gglasso_amd import _lib
    from gglasso_amd._lib import ptr
    rng = np.random.default_rng(31 * variant + p)
    A, B, E, E2 = (_sym(rng, K, p) for _ in range(4))
    iu = np.triu_indices(p)
    eye = np.eye(p)[None]
    for zero_d in (False, True):
        coef = rng.uniform(0.5, 1.5, (K, 8)) * rng.choice([-1.0, 1.0], (K, 8))
        if zero_d:
            coef[:, 5] = coef[:, 7] = 0.0
        coef = np.ascontiguousarray(coef)
        for e2 in (E2, None):
            def call():
                C, C2 = np.full_like(A, np.nan), np.full_like(A, np.nan)
                _lib.check(dev_library.ggl_dev_symm_full(K, p, ptr(A), ptr(B), ptr(E), None if e2 is None else ptr(e2), ptr(coef),
                                                         ptr(C), ptr(C2), variant))
                return C, C2
            (Cb, C2b), (Cs, C2s) = _both(dev_library, call)
            assert np.isfinite(Cs).all() and np.isfinite(C2s).all()
            assert _same_bits(Cb, Cs) and _same_bits(C2b, C2s), (zero_d, e2 is None)
            # the yardstick itself
            c = [coef[:, i, None, None] for i in range(8)]
            z = 0.0 if e2 is None else 1.0
            ref = c[0] * eye + c[1] * (A @ B) + c[2] * E + z * c[6] * E2
            ref2 = c[3] * eye + c[4] * ref + c[5] * E + z * c[7] * E2
            tol = 1e-12 * np.abs(ref).max() * p
            assert np.abs(Cs[:, iu[0], iu[1]] - ref[:, iu[0], iu[1]]).max() <= tol
            assert np.abs(C2s[:, iu[0], iu[1]] - ref2[:, iu[0], iu[1]]).max() <= 4.0 * tol     # |dC| <= 1.5, plus its own terms
            assert np.array_equal(Cs, Cs.transpose(0, 2, 1)) and np.array_equal(C2s, C2s.transpose(0, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("K,p", [(2, 130), (1, 500)])
@pytest.mark.parametrize("variant", [16, 17, 20])
def test_bound_partials_bitwise(dev_library, variant, K, p):
    from gglasso_amd import _lib
    from gglasso_amd._lib import ptr
    rng = np.random.default_rng(77 * variant + p)
    A, B = _sym(rng, K, p), _sym(rng, K, p)

    def call():
        C, rows, fro2, bound = np.full_like(A, np.nan), np.empty((K, p)), np.empty(K), np.empty(K)
        _lib.check(dev_library.ggl_dev_symm_bounds(K, p, ptr(A), ptr(B), variant, ptr(C), ptr(rows), ptr(fro2), ptr(bound)))
        return C, rows, fro2, bound

    got, ref = _both(dev_library, call)
    iu = np.triu_indices(p)                    # the yardstick itself: the upper triangle of A B, mirrored
    assert np.isfinite(ref[0]).all() and np.array_equal(ref[0], ref[0].transpose(0, 2, 1))
    assert np.abs(ref[0][:, iu[0], iu[1]] - (A @ B)[:, iu[0], iu[1]]).max() <= 1e-12 * np.abs(ref[0]).max() * p
    for nm, x, y in zip(("C", "row sums", "Frobenius", "bound"), got, ref):
        assert np.array_equal(x, y), nm


# What a variant number is, restated here on purpose (csrc/gemm_sym.hip keeps it in one table): the timing ablations, whose
# results are wrong by design, and the direct-to-LDS variants, the only ones that leave bound partials.
ABLATIONS = {6, 7, 10, 14, 15, 21} | set(range(30, 38))
DIRECT_TO_LDS = set(range(16, 40))


@pytest.mark.gpu
@pytest.mark.parametrize("K,p", [(3, 130), (2, 97)])
@pytest.mark.parametrize("variant", [v for v in range(40) if v not in ABLATIONS])
def test_every_variant_computes_the_product(dev_library, variant, K, p):
    """Every row of the variant table that is not an ablation: a bitwise symmetric C = cI I + cAcc A B + cE E, and -- where the
    variant leaves bound partials -- row sums and Frobenius norm that are those of the C it returned.  (3, 130): even p, two
    64-tiles and a remainder, an off-diagonal tile with its mirror even at tile edge 128, K outside the XCD-sharing cases;
    (2, 97): odd p, the last-column pair rule and a partial tile at every edge."""
    from gglasso_amd import _lib
    from gglasso_amd._lib import ptr
    rng = np.random.default_rng(500 * variant + p)
    A, B, E = _sym(rng, K, p), _sym(rng, K, p), _sym(rng, K, p)
    coef = np.ascontiguousarray(rng.uniform(0.5, 1.5, (K, 5)))
    C = np.full_like(A, np.nan)
    _lib.check(dev_library.ggl_dev_symm(K, p, ptr(A), ptr(B), ptr(E), ptr(coef), ptr(C), None, variant))
    assert np.isfinite(C).all()
    assert np.array_equal(C, C.transpose(0, 2, 1))
    iu = np.triu_indices(p)
    ref = coef[:, 0, None, None] * np.eye(p)[None] + coef[:, 1, None, None] * (A @ B) + coef[:, 2, None, None] * E
    err = np.abs(C[:, iu[0], iu[1]] - ref[:, iu[0], iu[1]]).max()
    print("variant", variant, "K", K, "p", p, "max error", err, "bound", 1e-12 * np.abs(ref).max() * p)
    assert err <= 1e-12 * np.abs(ref).max() * p
    Cb, rows, fro2, bound = np.full_like(A, np.nan), np.empty((K, p)), np.empty(K), np.empty(K)
    rc = dev_library.ggl_dev_symm_bounds(K, p, ptr(A), ptr(B), variant, ptr(Cb), ptr(rows), ptr(fro2), ptr(bound))
    if variant not in DIRECT_TO_LDS:
        assert rc == _lib.E_ARG and "no bound partials" in dev_library.ggl_last_error().decode()
        return
    _lib.check(rc)
    assert np.array_equal(Cb, Cb.transpose(0, 2, 1))
    # (the tolerances of test_product_epilogue_bound_partials, tests/test_gpu_ops.py)
    assert np.allclose(rows, np.abs(Cb).sum(axis=2), rtol=1e-13, atol=0)
    assert np.allclose(fro2, (Cb ** 2).sum(axis=(1, 2)), rtol=1e-13)


def _steps(S, options, iters=8):
    """`iters` ADMM iterations with the rho rule (tests/test_gpu_omega_poly.py _run): the state and the norms after every step"""
    from gglasso_amd import solver
    K, p = S.shape[0], S.shape[-1]
    eye = np.repeat(np.eye(p)[None], K, axis=0)
    eng = solver.HipEngine(S, eye, eye, np.zeros_like(S), options=options)
    nk = np.ones(K)
    rho, trail = 1.0, []
    try:
        for it in range(iters):
            if it == iters - 1:
                eng.hint_last_step()
            sq = eng.step(rho, 0.05, 0.01, "GGL", False, None, nk).copy()
            st = eng.state()
            trail.append((sq, st["Omega"].copy(), st["Theta"].copy(), st["X"].copy()))
            r_t, s_t, _, _ = solver.residuals_from_norms(sq, rho, 1e-20, 1e-20, 1.0)
            new = solver.next_rho(rho, r_t, s_t)
            if new != rho and it < iters - 1:
                eng.scale_X(rho / new)
            rho = new
        return trail, eng.poly_stats(), eng.ns_stats()
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K,p,seed,opts", [(8, 301, 77, {"ns_tol": 1e-9}), (16, 400, 2416, {"spec_factor": 0.9})])
def test_step_bitwise(dev_library, K, p, seed, opts):
    """E2 and the second output of the fused start exist at step level only: the direct family must really run (seqs > 0)"""
    from gglasso_amd import synth
    S, _ = synth.make_problem("GGL", K, p, N=2 * p, seed=seed)
    (tb, pb, nb), (ts, ps, ns) = _both(dev_library, lambda: _steps(S, opts))
    print("poly", pb, ps, "spec_misses", nb["spec_misses"], ns["spec_misses"], "variant", nb["last_variant"])
    assert pb["seqs"] > 0 and ps["seqs"] > 0, (pb, ps)
    assert len(tb) == len(ts) == 8
    for it, (b, s) in enumerate(zip(tb, ts)):
        for nm, x, y in zip(("norms", "Omega", "Theta", "X"), b, s):
            assert np.array_equal(x, y), (it, nm, float(np.abs(x - y).max()))
