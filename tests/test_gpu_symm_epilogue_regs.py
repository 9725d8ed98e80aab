"""The register epilogue of the direct-to-LDS product kernels (csrc/gemm_sym.hip symm_dl_tile, selector 0 of
ggl_dev_set_symm_epilogue: an off-diagonal tile and its mirror written from the accumulator registers, pairs exchanged with
lane ^ 1, the mirror transposed with v_permlane32_swap / v_permlane16_swap) against the serial epilogue (1) and the batched
one that stages the tile in LDS (2): the same bits, everywhere.

Three-way equality through ggl_dev_symm_full with E, E2, C2 and all eight coefficients, dE = dE2 = 0 as well, on the bit
patterns (the sign of a zero counts).  Shapes, one purpose each: (1, 128) one full off-diagonal tile, (2, 130) a two-column edge
tile, (3, 129) and (1, 65) the odd last column as half a pair and as the tile's only column, (2, 96) a wave whose whole column
half lies outside the matrix, (9, 70) the XCD remainder dealing.
Placement: A = I, cAcc = 1, no E, B[i][j] = 1024 min(i, j) + max(i, j): C must be B exactly, both triangles -- a misplaced lane
shows as a wrong index."""
import numpy as np
import pytest

SHAPES = [(1, 128), (2, 130), (3, 129), (1, 65), (2, 96), (9, 70)]
VARIANTS = [16, 17, 20, 22]
NAMES = {0: "register", 1: "serial", 2: "staged"}


def _each(dev, fn):
    """fn() under the register, the serial and the staged epilogue; the switch is restored"""
    out = []
    was = dev.ggl_dev_set_symm_epilogue(0)
    try:
        for mode in (0, 1, 2):
            dev.ggl_dev_set_symm_epilogue(mode)
            out.append(fn())
    finally:
        dev.ggl_dev_set_symm_epilogue(was)
    return out


def _sym(rng, K, p):
    X = rng.standard_normal((K, p, p))
    return 0.5 * (X + X.transpose(0, 2, 1))


def _bits(x):
    return x.view(np.int64)


def _first_diff(x, y):
    d = np.argwhere(_bits(x) != _bits(y))
    return None if d.size == 0 else (len(d), tuple(int(i) for i in d[0]))


@pytest.mark.gpu
def test_selector_round_trip(dev_library):
    """the selector keeps 0, 1 and 2 apart and returns the previous mode"""
    was = dev_library.ggl_dev_set_symm_epilogue(2)
    try:
        assert dev_library.ggl_dev_set_symm_epilogue(1) == 2
        assert dev_library.ggl_dev_set_symm_epilogue(0) == 1
        assert dev_library.ggl_dev_set_symm_epilogue(0) == 0
    finally:
        dev_library.ggl_dev_set_symm_epilogue(was)


@pytest.mark.gpu
@pytest.mark.parametrize("K,p", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_three_way_bitwise(dev_library, variant, K, p):
    from gglasso_amd import _lib
    from gglasso_amd._lib import ptr
    rng = np.random.default_rng(53 * variant + 7 * p + K)
    A, B, E, E2 = (_sym(rng, K, p) for _ in range(4))       # E, E2 bitwise symmetric, as every E of the solvers is
    iu = np.triu_indices(p)
    eye = np.eye(p)[None]
    for zero_d in (False, True):
        coef = rng.uniform(0.5, 1.5, (K, 8)) * rng.choice([-1.0, 1.0], (K, 8))
        if zero_d:
            coef[:, 5] = coef[:, 7] = 0.0
        coef = np.ascontiguousarray(coef)

        def call():
            C, C2 = np.full_like(A, np.nan), np.full_like(A, np.nan)
            _lib.check(dev_library.ggl_dev_symm_full(K, p, ptr(A), ptr(B), ptr(E), ptr(E2), ptr(coef), ptr(C), ptr(C2), variant))
            return C, C2

        (Cr, C2r), (Cs, C2s), (Ct, C2t) = _each(dev_library, call)
        assert np.isfinite(Cs).all() and np.isfinite(C2s).all()
        for nm, (x, x2) in (("register", (Cr, C2r)), ("staged", (Ct, C2t))):
            print(f"variant {variant} ({K}, {p}) zero_d {zero_d} {nm} vs serial: C {_first_diff(x, Cs)} C2 {_first_diff(x2, C2s)}")
        assert np.array_equal(_bits(Cr), _bits(Cs)) and np.array_equal(_bits(C2r), _bits(C2s)), ("register", zero_d)
        assert np.array_equal(_bits(Ct), _bits(Cs)) and np.array_equal(_bits(C2t), _bits(C2s)), ("staged", zero_d)
        # the yardstick itself
        c = [coef[:, i, None, None] for i in range(8)]
        ref = c[0] * eye + c[1] * (A @ B) + c[2] * E + c[6] * E2
        ref2 = c[3] * eye + c[4] * ref + c[5] * E + c[7] * E2
        tol = 1e-12 * np.abs(ref).max() * p
        assert np.abs(Cs[:, iu[0], iu[1]] - ref[:, iu[0], iu[1]]).max() <= tol
        assert np.abs(C2s[:, iu[0], iu[1]] - ref2[:, iu[0], iu[1]]).max() <= 4.0 * tol     # |dC| <= 1.5, plus its own terms
        assert np.array_equal(Cs, Cs.transpose(0, 2, 1)) and np.array_equal(C2s, C2s.transpose(0, 2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("K,p", [(1, 128), (1, 129), (1, 200)])
@pytest.mark.parametrize("variant", [17, 20])
def test_placement(dev_library, variant, K, p):
    from gglasso_amd import _lib
    from gglasso_amd._lib import ptr
    i = np.arange(p)
    B = np.ascontiguousarray(np.broadcast_to(1024.0 * np.minimum.outer(i, i) + np.maximum.outer(i, i), (K, p, p)))
    A = np.ascontiguousarray(np.broadcast_to(np.eye(p), (K, p, p)))
    coef = np.zeros((K, 8))
    coef[:, 1] = 1.0                                        # C = A B, nothing else
    C = np.full_like(B, np.nan)
    was = dev_library.ggl_dev_set_symm_epilogue(0)
    try:
        _lib.check(dev_library.ggl_dev_symm_full(K, p, ptr(A), ptr(B), None, None, ptr(coef), ptr(C), None, variant))
    finally:
        dev_library.ggl_dev_set_symm_epilogue(was)
    bad = np.argwhere(C != B)
    if bad.size:
        k, r, c = (int(x) for x in bad[0])
        got = C[k, r, c]
        where = (int(got) // 1024, int(got) % 1024) if np.isfinite(got) else got
        print(f"{len(bad)} misplaced; first at C[{k}][{r}][{c}]: holds the entry of (min, max) = {where}")
    assert np.array_equal(C, B)
