"""Every launch route of the Newton-Schulz Omega-step (omega_step and its per-route functions, capi_omega.hip), named, proven
taken, and checked against eigh.  The route is picked from the shape and from state no drawn shape controls: the split
(omega_split: one launch sequence, two parts of a small batch, K >= 16 concurrent parts, or contiguous groups with their own
schedules), speculative or validated (omega_finish_spec / omega_finish_validated), a fresh chain or the RESUME of an early
first part (ggl_ctx::EarlyA, which keeps the part's OmegaChainPlan) launched behind the previous iteration's Theta-step, and
the product-kernel variant, which also fixes the tile layout of the bound partials the B' launch leaves behind.

Each case runs ggl_admm_step with the reference's rho rule (solver/admm_solver.py:227-233), so that the residual ratio settles
and early parts fire, on heterogeneous instances (S scaled per instance), and
  1. asserts, after every call that resumed an early part, the split, the group count and the kernel variant the dispatch rule
     predicts (the arithmetic is below) -- the stats after a call describe the last Omega-step it launched, which is the
     resumed one (maybe_prelaunch);
  2. compares the iterates with the plain route (no groups, no early part) under the same rho sequence;
  3. compares the last Omega-step with phi^+ of the plain run's W computed by eigh;
  4. checks the spectral bound the last step validated: lambda_max(A') <= c <= |A'|_F, A' = W^2 + 4 beta I."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import pytest

ITERS = 40
LAM1, LAM2 = 0.05, 0.02

# ---- the dispatch rule, restated (gemm_sym.hip: symm_auto_variant, symm_effective_variant, symm_bounds_tile;
# capi_omega.hip: omega_step) ----------------------------------------------------------------------------------------------
SMALL_BATCH_TILES = 800        # up to here the 32x32-tile kernel (variant 20), above it the 64x64 one (16)
PARTS_MIN_TILES, PARTS_MAX_TILES = 600, 2048
PARTS_SMALL = 8                # default GGL_OPT_PARTS_SMALL


def tile_pairs(K, p):
    """64x64 tile pairs of the upper triangles of K p x p products."""
    t = -(-p // 64)
    return t * (t + 1) // 2 * K


def auto_variant(K, p):
    return 20 if tile_pairs(K, p) <= SMALL_BATCH_TILES else 16


def grouped_variant(K, p):
    """Groups share one kernel instance: the one the WHOLE batch would take, 64x64 with three DMA stages (17)."""
    v = auto_variant(K, p)
    return 17 if v == 16 else v


def effective_variant(v, p, odd_dl=True):
    """What runs: without the direct-to-LDS kernel for this p (odd p with odd_dl off), the register-staged one of the tile."""
    if 16 <= v <= 39 and not (p % 2 == 0 or odd_dl):
        return 9 if (v == 20 or v >= 24) else 0
    return v


def bounds_tile(v, p, odd_dl=True):
    if not (p % 2 == 0 or odd_dl):
        return 0
    return 32 if v == 20 else 64


def predicted_parts(K, p, parts_small=PARTS_SMALL):
    if K >= 16 and PARTS_MIN_TILES <= tile_pairs(K, p) <= PARTS_MAX_TILES:
        return min(2, K // 8)
    if parts_small and parts_small <= K < 16 and p >= 384:
        return 2
    return 1


def unfixed_resume_variant(K, p, Kh0):
    """The variant a resumed grouped step took while EarlyA did not keep it: the split was restored, `grouped` was not, so the
    rule for concurrent parts (K >= 16: 17) or the size rule of the first group decided."""
    if K >= 16:
        return 17
    return auto_variant(Kh0, p)


@dataclass
class Case:
    name: str
    K: int
    p: int
    opts: dict = field(default_factory=dict)
    route: str = "grouped"               # grouped | parts | single
    rho0: float = 1.0
    odd_dl: tuple = (1,)
    spec_miss: bool = False              # R5: every speculative step rejected
    rho_change_grouped: bool = False     # R6: a validated step after a rho change ran as groups
    default_rule: bool = False           # R4: the default time model groups this shape


G13 = {"group_sched": 13.0}
CASES = [
    Case("R1", 16, 400, G13),
    Case("R2", 7, 1000, G13),
    Case("R3", 15, 640, {**G13, "parts_small": 0.0}),
    Case("R4", 7, 1000, {}, default_rule=True),
    Case("R5", 16, 400, {**G13, "spec_factor": 0.9}, spec_miss=True),
    Case("R6", 16, 400, G13, rho0=16.0, rho_change_grouped=True),
    Case("R7", 16, 401, G13, odd_dl=(1, 0)),
    Case("R8", 8, 400, {}, route="parts"),
    Case("R9", 16, 576, {}, route="parts"),
    Case("R10", 6, 256, {"group_sched": 0.0}, route="single"),
]


def test_the_cases_discriminate():
    """The arithmetic the cases stand on (no GPU needed, but kept with the cases): R1-R3 are shapes where a resumed grouped
    step that forgot it was grouped takes another variant and another bound-partial layout than its early part wrote."""
    # R1: 28 pairs x 16 = 448 <= 800: 32-tiles (bT = 13), but K >= 16 parts take 17: 64-tiles (bT = 7)
    assert tile_pairs(16, 400) == 448 and grouped_variant(16, 400) == 20 and unfixed_resume_variant(16, 400, 5) == 17
    assert -(-400 // bounds_tile(20, 400)) == 13 and -(-400 // bounds_tile(17, 400)) == 7
    # R2: 136 x 7 = 952 > 800: the whole batch takes 17; a group of <= 5 alone takes 20 (680)
    assert tile_pairs(7, 1000) == 952 and grouped_variant(7, 1000) == 17
    assert all(auto_variant(n, 1000) == 20 for n in range(1, 6)) and auto_variant(6, 1000) == 16
    # R3: 55 x 15 = 825 > 800, groups of <= 14 -> 770: 20
    assert tile_pairs(15, 640) == 825 and grouped_variant(15, 640) == 17 and auto_variant(14, 640) == 20
    assert predicted_parts(15, 640) == 2 and predicted_parts(15, 640, parts_small=0) == 1
    # controls: two parts of a small batch, K >= 16 concurrent parts (720 pairs), one sequence
    assert predicted_parts(8, 400) == 2 and auto_variant(4, 400) == 20
    assert tile_pairs(16, 576) == 720 and predicted_parts(16, 576) == 2
    assert predicted_parts(6, 256) == 1 and auto_variant(6, 256) == 20
    # R7: odd p on the DMA kernel, and without it the register-staged 32x32 kernel and no bound partials
    assert effective_variant(20, 401) == 20 and effective_variant(20, 401, odd_dl=False) == 9
    assert bounds_tile(20, 401, odd_dl=False) == 0
    # the grouped cases run as one launch sequence before grouping (groups are cut only from a single sequence)
    for c in CASES:
        if c.route == "grouped":
            assert predicted_parts(c.K, c.p, int(c.opts.get("parts_small", PARTS_SMALL))) == 1, c.name


def _problem(K, p, seed):
    from gglasso_amd import synth
    S, _ = synth.make_problem("GGL", K, p, N=2 * p, seed=seed)
    return S * np.geomspace(0.2, 2.5, K)[:, None, None]


def _stats(eng):
    return eng.ns_stats(), eng.group_stats(), eng.pipeline_stats()


def _run(S, options, rho0, iters, mid=None):
    """ADMM iterations through ggl_admm_step with the rho rule; the last step is announced (no chain behind it).  Returns the
    final state, the rho of every step, the stats after every call, the state after `mid` steps (if asked: reading it drops a
    pre-launched chain, so only the plain run asks) and the spectral bounds of the last validated step."""
    from gglasso_amd import solver
    K, p = S.shape[0], S.shape[-1]
    eye = np.repeat(np.eye(p)[None], K, axis=0)
    eng = solver.HipEngine(S, eye, eye, np.zeros_like(S), options=options)
    nk = np.ones(K)
    rho, rhos, trail, st_mid = rho0, [], [_stats(eng)], None
    try:
        for it in range(iters):
            if it == mid:
                st_mid = eng.state()
            if it == iters - 1:
                eng.hint_last_step()
            rhos.append(rho)
            sq = eng.step(rho, LAM1, LAM2, "GGL", False, None, nk).copy()
            trail.append(_stats(eng))
            r_t, s_t, _, _ = solver.residuals_from_norms(sq, rho, 1e-20, 1e-20, 1.0)
            new = solver.next_rho(rho, r_t, s_t)
            if new != rho and it < iters - 1:
                eng.scale_X(rho / new)
            rho = new
        return eng.state(), rhos, trail, st_mid, eng.spectral_bounds()
    finally:
        eng.close()


def _d(trail, t, which, key):
    return trail[t][which][key] - trail[t - 1][which][key]


def _check_route(case, trail, rhos, odd_dl):
    K, p = case.K, case.p
    ns, gs, ps = trail[-1]
    resumed = [t for t in range(1, len(trail)) if _d(trail, t, 2, "early_used") > 0]
    info = (case.name, odd_dl, ps, ns, gs)
    if case.spec_miss:
        # spec_factor 0.9: the schedule assumes 90 % of the last bound, the validation rejects it, the step is repeated
        # bounds first and the early part launched behind it is forgotten
        validated_spec = ns["spec_calls"] - ns["pre_dropped"]
        assert ns["spec_misses"] >= 3 and ns["spec_misses"] == validated_spec, info
        assert ps["early_launched"] >= 1 and ps["early_used"] == 0, info
        return
    assert len(resumed) >= 3 and ps["early_used"] == len(resumed), info
    if case.route == "grouped":
        want = effective_variant(grouped_variant(K, p), p, odd_dl)
        for t in resumed:
            ns_t, gs_t, _ = trail[t]
            # a resumed step runs the split of its early part, as groups with their own schedules, on the kernel the whole
            # batch would take -- and is counted as a grouped step
            assert ns_t["last_parts"] >= 2 and gs_t["groups"] == ns_t["last_parts"], (t, info)
            assert sum(gs_t["len"]) == K and len(gs_t["len"]) == gs_t["groups"], (t, info)
            assert ns_t["last_variant"] == want, (t, want, info)
            assert _d(trail, t, 1, "steps") >= 1, (t, info)
        lens = trail[resumed[-1]][1]["len"]
        if case.name in ("R2", "R3"):
            # a group alone would take the 32x32 kernel, the batch takes 17: the resume must not ask the size rule again
            assert grouped_variant(K, p) == 17 and min(auto_variant(n, p) for n in lens) == 20, lens
        if case.name == "R1":
            assert unfixed_resume_variant(K, p, lens[0]) != grouped_variant(K, p)
    else:
        parts = predicted_parts(K, p, int(case.opts.get("parts_small", PARTS_SMALL)))
        assert parts == (2 if case.route == "parts" else 1)
        for t in resumed:
            ns_t, gs_t, _ = trail[t]
            assert ns_t["last_parts"] == parts and gs_t["groups"] == 1, (t, info)
            Kh0 = K - K // 2 if parts == 2 else K
            want = 17 if (parts > 1 and K >= 16) else auto_variant(Kh0, p)
            assert ns_t["last_variant"] == effective_variant(want, p, odd_dl), (t, want, info)
        assert gs["steps"] == 0, info
    if case.rho_change_grouped:
        # a rho change drops the pre-launched chain: the step runs validated (bounds first), and the products as groups
        # chosen from THOSE bounds (plan_regroup).  Such a call launched validated steps only, or that step plus the next chain:
        # every Omega-step of the call was grouped.
        hits = [t for t in range(2, len(trail)) if rhos[t - 1] != rhos[t - 2]
                and _d(trail, t, 0, "calls") > _d(trail, t, 0, "spec_calls")
                and _d(trail, t, 1, "steps") == _d(trail, t, 0, "calls")]
        assert hits, (rhos, info)
        for t in hits:
            if _d(trail, t, 0, "spec_calls") == 0:
                assert trail[t][0]["last_variant"] == effective_variant(grouped_variant(K, p), p, odd_dl), (t, info)
    return resumed


def _default_rule_groups(bounds, p):
    """The default time model (sum_g U_g (F + len_g I(p)), ns_group_partition) applied to the units of the last bounds as a
    speculative schedule sees them (x 1.02): the groups it cuts at this p."""
    from gglasso_amd import _lib
    lib = _lib.load()
    c, beta = bounds
    ck = np.maximum(c * 1.02 * (1 + 1e-10), 4 * beta)
    u = np.array([lib.ggl_dev_ns_units(float(np.sqrt(4 * b / x)), 9, 2e-12) for x, b in zip(ck, beta)], dtype=np.int32)
    assert np.all(u > 0), u
    out = np.zeros(3, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    g = lib.ggl_dev_group_partition(u.ctypes.data_as(ip), len(u), int(p), 3, out.ctypes.data_as(ip))
    return g, u, out[:g].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_omega_route(case):
    from gglasso_amd import _lib
    from oracle import ggl_oracle as orc
    S = _problem(case.K, case.p, 2000 + case.K + case.p)
    lib = _lib.load()
    for odd_dl in case.odd_dl:
        was = lib.ggl_set_odd_dl(odd_dl)
        try:
            route, rhos, trail, _, bounds = _run(S, case.opts, case.rho0, ITERS)
            plain, rhos_p, _, prev, _ = _run(S, {"group_sched": 0.0, "early_part": 0.0}, case.rho0, ITERS, mid=ITERS - 1)
        finally:
            lib.ggl_set_odd_dl(was)
        # 1. the route was taken
        _check_route(case, trail, rhos, odd_dl)
        if case.default_rule:
            g, u, lens = _default_rule_groups(bounds, case.p)
            assert g >= 2 and len(set(u.tolist())) >= 2, (g, u, lens)
        # 2. the iterates of the plain route, same rho sequence
        assert rhos == rhos_p
        for nm in ("Omega", "Theta", "X"):
            assert np.abs(route[nm] - plain[nm]).max() <= 1e-10, (case.name, odd_dl, nm)
        assert np.array_equal(route["Omega"], route["Omega"].transpose(0, 2, 1))
        # 3. the last Omega-step against eigh: W = Theta - X - S / rho of the plain run's state before it (nk = 1)
        rho = rhos[-1]
        W = prev["Theta"] - prev["X"] - S / rho
        Om, D = orc.phiplus_stack(W, 1.0 / rho)
        assert np.abs(route["Omega"] - Om).max() <= 1e-9, (case.name, odd_dl)
        # 4. the bound the last step validated is a bound: lambda_max(A') <= c <= |A'|_F, A' = W^2 + 4 beta I
        c, beta = bounds
        assert np.all(beta == 1.0 / rho), beta
        ev = D * D + 4.0 / rho
        lmax, fro = ev.max(axis=1), np.sqrt((ev * ev).sum(axis=1))
        assert np.all(lmax * (1 - 1e-9) <= c), (case.name, odd_dl, c / lmax)
        assert np.all(c <= fro * (1 + 1e-9)), (case.name, odd_dl, c / fro)
