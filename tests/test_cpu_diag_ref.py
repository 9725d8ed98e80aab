"""CPU twin of tests/test_gpu_diagnostics.py: the reference of tests/diag_ref.py against the oracle on every case of its table.
No case may test a zero (every applicable term of a generic state is at least FLOOR), the maximum of the four reference terms is
the oracle's kkt_stopping_criterion, and the three objective parts add up to the oracle's f_obj + P_val."""
import numpy as np
import pytest

from oracle import ggl_oracle as orc
import diag_ref as dr


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(c):
        if c.name not in cache:
            cache[c.name] = dr.build_case(c)
        return cache[c.name]
    return get


def test_case_names_are_unique():
    for table in (dr.CASES, dr.OBJ_CASES):
        names = [c.name for c in table]
        assert len(set(names)) == len(names)


@pytest.mark.parametrize("c", dr.CASES, ids=lambda c: c.name)
def test_kkt_terms_reference_against_the_oracle(built, c):
    b = built(c)
    st = b["state"]
    for nm in ("Omega", "Theta", "L", "X"):
        assert np.array_equal(st[nm], st[nm].transpose(0, 2, 1)), nm
    if not c.latent:
        assert not st["L"].any()
    ref = dr.kkt_ref_of(c, b)
    n_terms = 4 if c.latent else 3
    t = ref.terms.astype(np.float64)
    assert t[3] == 0.0 or c.latent
    if c.generic:
        assert t[:n_terms].min() >= dr.FLOOR, t
    else:
        # near a fixed point: terms of the size of the noise, none of them a zero
        assert 1e-8 <= t[:n_terms].min() and t[:n_terms].max() <= 1e-4, t
    want = dr.oracle_kkt(c.reg, st["Omega"], st["Theta"], st["L"], st["X"], b["S"], b["rho"], b["lambda1"], b["lambda2"], b["nk"],
                         c.latent, b["mu1"], b["mask"])
    assert abs(float(t.max()) - want) <= 1e-12 * want, (t, want)
    # the derived bounds of terms 1 and 2 are far below the terms they guard
    assert np.all(ref.bounds[:2] <= 1e-6 * t[:2]), (ref.bounds, t)


def test_per_instance_masks_differ_from_the_scalar_threshold(built):
    """the per-instance-mask cases can tell a call that ignored the masks: term 1 with the scalar lambda1 is far off"""
    for c in dr.CASES:
        if c.mask != "k":
            continue
        b = built(c)
        t_mask = float(dr.kkt_ref_of(c, b).terms[0])
        t_scalar = float(dr.kkt_ref_of(c, dict(b, mask=None)).terms[0])
        t_first = float(dr.kkt_ref_of(c, dict(b, mask=b["mask"][0])).terms[0])
        assert abs(t_mask - t_scalar) >= 1e-3 * t_mask and abs(t_mask - t_first) >= 1e-3 * t_mask, (t_mask, t_scalar, t_first)


@pytest.mark.parametrize("c", [c for c in dr.OBJ_CASES if c.reg != "FSGL"], ids=lambda c: c.name)
def test_objective_parts_add_up_to_the_oracle(built, c):
    """after one oracle step from the generic start (the state the GPU test evaluates, up to the device's rounding)"""
    b = built(c)
    st = b["state"]
    K = c.K
    nk = np.asarray(b["nk"]).reshape(K, 1, 1)
    rho = b["rho"]
    Om, _ = orc.phiplus_stack(st["Theta"] - st["L"] - st["X"] - (nk / rho) * b["S"], nk[:, 0, 0] / rho)
    Th = orc.prox_p(Om + st["L"] + st["X"], b["lambda1"] / rho, b["lambda2"] / rho, c.reg)
    ref = dr.obj_ref(c.reg, Om, Th, b["S"], b["lambda1"], b["lambda2"])
    want = orc.f_obj(Om, b["S"]) + orc.P_val(Th, b["lambda1"], b["lambda2"], c.reg)
    assert abs(float(ref.parts.sum()) - want) <= 1e-12 * max(1.0, abs(want)), (ref.parts, want)
    assert abs(float(ref.parts[2]) - orc.P_val(Th, b["lambda1"], b["lambda2"], c.reg)) <= 1e-12 * max(1.0, float(ref.parts[2]))
    if c.p == 1:
        assert ref.parts[2] == 0.0
    assert np.isfinite(ref.kappa) and ref.kappa < 1e4


def test_p_val_reads_the_upper_triangle_only():
    rng = np.random.default_rng(5)
    Th = dr.sym(rng.standard_normal((3, 9, 9)))
    bad = Th.copy()
    il = np.tril_indices(9, -1)
    bad[:, il[0], il[1]] = 1e3 * rng.standard_normal((3, len(il[0])))
    for reg in ("GGL", "FGL"):
        assert dr.p_val(reg, bad, 0.05, 0.02)[0] == dr.p_val(reg, Th, 0.05, 0.02)[0]
        assert orc.P_val(bad, 0.05, 0.02, reg) == orc.P_val(Th, 0.05, 0.02, reg)
