"""The scalars that decide when a solve stops and that measure=True reports -- ggl_kkt_terms / ggl_kkt_residual and the three
parts of ggl_objective -- term by term against tests/diag_ref.py (reference, bounds and cases: see its docstring), on states
that are NOT ADMM iterates (on an iterate two of the four KKT terms vanish and the maximum hides the rest); and the scratch
these entry points, the exit checks, the selection statistics and ggl_finalize_L(1) use between two steps: whatever is called,
in whatever order, every number is the same in every bit and the solve that goes on is the solve that was never looked at."""
import numpy as np
import pytest

import diag_ref as dr

pytestmark = pytest.mark.gpu

NAMES = ("Omega", "Theta", "L", "X")
_WORST = {}         # quantity -> (share of its bound, deviation, bound, case)
_RATIO = {}         # 'eig' / 'logdet' -> (largest deviation / unit, case)
_SEEN = {"logdet_w": 0, "logdet_chol": 0, "logdet_eig": 0, "kkt_jacobi": 0, "kkt_rocsolver": 0, "kkt_mask": 0, "kkt_mask_k": 0,
         "prox_od": 0, "prox_p": 0}
_BUILT = {}


def _built(c):
    if c.name not in _BUILT:
        _BUILT[c.name] = dr.build_case(c)
    return _BUILT[c.name]


def _engine(c, b, options=None):
    from gglasso_amd import solver
    st = b["state"]
    eng = solver.HipEngine(b["S"], st["Omega"], st["Theta"], st["X"], st["L"] if c.latent else None, eig=c.eig, options=options)
    if c.mask == "k":
        eng.set_lambda1_mask_k(b["mask"])
    elif c.mask is not None:
        eng.set_lambda1_mask(b["mask"])
    if c.M:
        eng.set_block_size(c.M)
    return eng


def _args(c, b):
    return (b["rho"], b["lambda1"], b["lambda2"], c.reg, c.latent, b["mu1"], b["nk"])


def _note(what, dev, bound, name):
    share = dev / bound if bound > 0 else (0.0 if dev == 0 else np.inf)
    print(f"{name:34s} {what:9s} deviation {dev:.3e}  bound {bound:.3e}  ({share:.3f})")
    if what not in _WORST or share > _WORST[what][0]:
        _WORST[what] = (share, dev, bound, name)
    return share


def _ratio(kind, dev, unit, name):
    r = dev / unit
    if kind not in _RATIO or r > _RATIO[kind][0]:
        _RATIO[kind] = (r, name)
    return r


def _count(eng):
    for k, v in eng.diag_stats().items():
        _SEEN[k] += v


def _jacobi(c):
    return c.eig == dr.EIG_JACOBI or (c.eig == dr.EIG_AUTO and c.p <= 128)


# ---- values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dr.CASES, ids=lambda c: c.name)
def test_kkt_terms_against_the_reference(c):
    b = _built(c)
    eng = _engine(c, b)
    try:
        terms = eng.kkt_terms(*_args(c, b))
        res = eng.kkt_residual(*_args(c, b))
        again = eng.kkt_terms(*_args(c, b))
        st = eng.state()
        stats = eng.diag_stats()
        _count(eng)
    finally:
        eng.close()
    # the diagnostic leaves the iterate alone, and the reference is taken on what the device holds
    for nm in NAMES:
        assert np.array_equal(st[nm], b["state"][nm]), nm
    assert np.array_equal(terms, again)
    assert res == terms.max() and (c.latent or terms[3] == 0.0)
    ref = dr.kkt_ref_of(c, b, st)
    want = ref.terms.astype(np.float64)
    dev = np.abs(terms.astype(np.longdouble) - ref.terms).astype(np.float64)
    print()
    for i in (0, 1):
        assert _note(f"term{i + 1}", dev[i], ref.bounds[i], c.name) <= 1.0, (terms, want)
    for i in (2, 3) if c.latent else (2,):
        r = _ratio("eig", dev[i], ref.bounds[i], c.name)
        print(f"{c.name:34s} term{i + 1}     deviation {dev[i]:.3e}  unit  {ref.bounds[i]:.3e}  ratio {r:.3f}")
        assert _note(f"term{i + 1}", dev[i], dr.EIG_CONST * ref.bounds[i], c.name) <= 1.0, (terms, want)
    # which eigensolver and which thresholds ran
    assert (stats["kkt_jacobi"], stats["kkt_rocsolver"]) == ((3, 0) if _jacobi(c) else (0, 3))
    assert (stats["kkt_mask"], stats["kkt_mask_k"]) == {None: (0, 0), "shared": (3, 0), "zero": (3, 0), "k": (0, 3)}[c.mask]
    _SEEN["prox_od" if c.reg == "SGL" else "prox_p"] += 1


def _step_args(c, b):
    return (b["rho"], b["lambda1"], b["lambda2"], c.reg, c.latent, b["mu1"], b["nk"])


def _check_objective(c, b, obj, st, name, M=None, parts=(0, 1, 2)):
    ref = dr.obj_ref(c.reg, st["Omega"], st["Theta"], b["S"], b["lambda1"], b["lambda2"], M)
    dev = np.abs(obj.astype(np.longdouble) - ref.parts).astype(np.float64)
    if 0 in parts:
        r = _ratio("logdet", dev[0], ref.bounds[0], name)
        print(f"{name:34s} -logdet   deviation {dev[0]:.3e}  unit  {ref.bounds[0]:.3e}  ratio {r:.3f}  kappa {ref.kappa:.1f}")
        assert _note("-logdet", dev[0], dr.LOGDET_CONST * ref.bounds[0], name) <= 1.0, (obj, ref.parts)
    if 1 in parts:
        assert _note("<Omega,S>", dev[1], ref.bounds[1], name) <= 1.0, (obj, ref.parts)
    if 2 in parts:
        assert _note("P_val", dev[2], ref.bounds[2], name) <= 1.0, (obj, ref.parts)
    return ref


@pytest.mark.parametrize("c", dr.OBJ_CASES, ids=lambda c: c.name)
def test_objective_parts_after_one_step(c):
    """One step from the generic start, then the three parts against the state the device holds.  The log det comes from the
    eigenvalues of W where the Omega-step left them (p <= 8, a forced eigensolver), from the Cholesky factor elsewhere."""
    b = _built(c)
    eng = _engine(c, b)
    try:
        eng.step(*_step_args(c, b))
        obj = eng.objective(b["lambda1"], b["lambda2"], c.reg)
        again = eng.objective(b["lambda1"], b["lambda2"], c.reg)
        st = eng.state()
        stats = eng.diag_stats()
        _count(eng)
    finally:
        eng.close()
    assert np.array_equal(obj, again)
    from_w = c.eig != dr.EIG_AUTO or c.p <= 8
    assert (stats["logdet_w"], stats["logdet_chol"], stats["logdet_eig"]) == ((2, 0, 0) if from_w else (0, 2, 0)), stats
    print()
    # FSGL: the penalty part is what differs from the SGL objective; the other two are covered by every other case
    _check_objective(c, b, obj, st, c.name, M=c.M, parts=(2,) if c.reg == "FSGL" else (0, 1, 2))
    if c.p == 1:
        assert obj[2] == 0.0
    assert np.all(np.isfinite(obj))


def _pd(Om, floor=0.2):
    """the stack with every instance shifted to a smallest eigenvalue of at least `floor`"""
    mn = np.linalg.eigvalsh(Om)[:, 0]
    return Om + np.maximum(0.0, floor - mn)[:, None, None] * np.eye(Om.shape[-1])[None]


@pytest.mark.parametrize("reg,K,p", [("GGL", 3, 65), ("FGL", 3, 65), ("GGL", 2, 33)])
def test_p_val_reads_the_upper_triangle(reg, K, p):
    """A Theta with a garbage lower triangle has the P_val of its twin symmetrised from the upper triangle (ggl_helper.py:162-176
    reads i < j), over several ragged 32-tiles."""
    c = dr.Case(reg, K, p)
    b = _built(c)
    st = dict(b["state"])
    st["Omega"] = _pd(st["Omega"])
    rng = np.random.default_rng(p)
    il = np.tril_indices(p, -1)
    bad = st["Theta"].copy()
    bad[:, il[0], il[1]] = 50.0 * rng.standard_normal((K, len(il[0])))
    eng = _engine(c, dict(b, state=st))
    try:
        good = eng.objective(b["lambda1"], b["lambda2"], reg)
        eng.set_state(st["Omega"], bad, st["X"])
        got = eng.objective(b["lambda1"], b["lambda2"], reg)
    finally:
        eng.close()
    assert got[2] == good[2], (got, good)
    print()
    _check_objective(c, b, good, st, f"{c.name}-setstate")


def test_objective_of_an_indefinite_omega_then_a_definite_one():
    """potrf fails on an indefinite Omega: the eigenvalue fallback runs, the call succeeds and part 0 is not finite; the same
    ctx, given a definite state next, returns the correct finite value (the status word was left clean)."""
    c = dr.Case("GGL", 2, 33)
    b = _built(c)
    st = dict(b["state"])
    st["Omega"] = _pd(st["Omega"])
    bad = st["Omega"].copy()
    bad[1] -= 2.0 * np.linalg.eigvalsh(bad[1])[-1] * np.outer(*[np.linalg.eigh(bad[1])[1][:, 0]] * 2)
    bad[1] = 0.5 * (bad[1] + bad[1].T)
    assert np.linalg.eigvalsh(bad[1])[0] < -0.1 and np.linalg.eigvalsh(bad[0])[0] > 0.1
    eng = _engine(c, dict(b, state=dict(st, Omega=bad)))
    try:
        obj_bad = eng.objective(b["lambda1"], b["lambda2"], c.reg)
        s1 = eng.diag_stats()
        eng.set_state(st["Omega"], st["Theta"], st["X"])
        obj = eng.objective(b["lambda1"], b["lambda2"], c.reg)
        kkt = eng.kkt_terms(*_args(c, b))
        s2 = eng.diag_stats()
        back = eng.state()
        _count(eng)
    finally:
        eng.close()
    assert not np.isfinite(obj_bad[0]) and np.all(np.isfinite(obj_bad[1:]))
    assert (s1["logdet_chol"], s1["logdet_eig"]) == (0, 1) and (s2["logdet_chol"], s2["logdet_eig"]) == (1, 1)
    assert np.all(np.isfinite(obj)) and np.all(np.isfinite(kkt))
    print()
    _check_objective(c, b, obj, back, "indefinite-then-definite")


@pytest.mark.parametrize("how", ["set_state", "restore_state"])
def test_objective_after_the_state_was_replaced(how):
    """p <= 8: the Omega-step leaves the eigenvalues of W and ggl_objective reads them.  They belong to the Omega that step wrote:
    once the state is set anew (or restored), the log det is the new Omega's."""
    c = dr.Case("GGL", 5, 8, latent=True, rho=1.7)
    b = _built(c)
    st = dict(b["state"])
    st["Omega"] = _pd(st["Omega"])
    eng = _engine(c, dict(b, state=st))
    try:
        eng.save_state()
        eng.step(*_step_args(c, b))
        first = eng.objective(b["lambda1"], b["lambda2"], c.reg)
        if how == "set_state":
            eng.set_state(st["Omega"], st["Theta"], st["X"], st["L"])
        else:
            eng.restore_state()
        obj = eng.objective(b["lambda1"], b["lambda2"], c.reg)
        back = eng.state()
        stats = eng.diag_stats()
    finally:
        eng.close()
    assert (stats["logdet_w"], stats["logdet_chol"]) == (1, 1)
    for nm in NAMES:
        assert np.array_equal(back[nm], st[nm]), nm
    assert first[0] != obj[0]
    print()
    _check_objective(c, b, obj, back, f"after-{how}")


# ---- order independence ----------------------------------------------------------------------------------------------------------
TAU = np.array([0.01, 0.05, 0.2])
ORDER_CASES = [dr.Case("GGL", 2, 8, rho=1.7, tag="-order"), dr.Case("FGL", 3, 33, latent=True, tag="-order"),
               dr.Case("GGL", 2, 129, latent=True, rho=1.7, tag="-order")]


def _calls(c, b):
    """name -> function(engine) returning arrays; the snapshot statistics need the snapshots _prepare takes"""
    calls = {
        "objective": lambda e: e.objective(b["lambda1"], b["lambda2"], c.reg),
        "kkt_terms": lambda e: e.kkt_terms(*_args(c, b)),
        "kkt_residual": lambda e: np.array([e.kkt_residual(*_args(c, b))]),
        "exit_checks": lambda e: e.exit_checks(c.latent),
        "exit_checks_k": lambda e: e.exit_checks_k(c.latent),
        "exit_checks_fast": lambda e: e.exit_checks_fast(c.latent, 1e-7),
        "state": lambda e: np.stack([e.state()[nm] for nm in NAMES]),
        "selection_stats": lambda e: e.selection_stats(),
        "threshold_scan": lambda e: e.threshold_scan(TAU)[0],
    }
    if c.latent:
        calls["selection_rank"] = lambda e: e.selection_rank()
    return calls


def _finalize_snapshots(e):
    n, rk = e.finalize_L(1)
    return np.concatenate([[n], rk, np.stack([e.snapshot_L_k(k) for k in range(e.K)]).ravel()])


def _prepare(c, b, options=None, steps=2):
    eng = _engine(c, b, options)
    for _ in range(steps):
        eng.step(*_step_args(c, b))
    for k in range(c.K):
        eng.snapshot_k(k)
    return eng


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("c", ORDER_CASES, ids=lambda c: c.name)
def test_every_number_is_the_same_in_any_order(c):
    """Two steps, snapshots, then every diagnostic: in one order, in the reverse order, each twice in a row, and with
    ggl_finalize_L(1) first -- every returned number is the same in every bit.  (The rank of the snapshots' L is the one
    statistic ggl_finalize_L(1) is MEANT to change: it is compared before with before and after with after.)"""
    b = _built(c)
    calls = _calls(c, b)
    names = list(calls)
    runs = []
    for order, fin_first in ((names, False), (names[::-1], False), (names, True)):
        eng = _prepare(c, b)
        out = {}
        try:
            if fin_first and c.latent:
                out["finalize_L(1)"] = _finalize_snapshots(eng)
            for nm in order:
                key = nm if not (fin_first and c.latent and nm in ("selection_rank",)) else nm + "-after"
                out[key] = calls[nm](eng)
                assert _same(calls[nm](eng), out[key]), f"{nm} twice in a row"
            if c.latent and not fin_first:
                out["finalize_L(1)"] = _finalize_snapshots(eng)
                out["selection_rank-after"] = calls["selection_rank"](eng)
                assert eng.finalize_L(1)[0] == 0                      # nothing left to rebuild
            out["state-end"] = calls["state"](eng)
            _count(eng)
        finally:
            eng.close()
        runs.append(out)
    for other in runs[1:]:
        for key, val in other.items():
            assert _same(val, runs[0][key]), key
    assert _same(runs[0]["state"], runs[0]["state-end"])
    assert runs[0]["kkt_residual"][0] == runs[0]["kkt_terms"].max()
    if c.latent and c.p > 8:
        assert runs[0]["finalize_L(1)"][0] == c.K                    # the sign iteration's L was rebuilt in every snapshot


# ---- neutrality toward the solve ---------------------------------------------------------------------------------------------------
ROUTES = {"lds": dr.Case("GGL", 4, 40, rho=1.7, tag="-neutral"), "chain": dr.Case("FGL", 3, 130, tag="-neutral"),
          "latent": dr.Case("GGL", 3, 130, latent=True, rho=1.7, tag="-neutral")}
CONFIGS = {"pipeline0": {"early_part": 0, "pipeline": 0}, "pipeline1": {"early_part": 0, "pipeline": 1}, "default": {}}


def _solve(c, b, options, diag=None):
    """eight steps, `diag` after step 3 and step 6; returns (the five sums of every step, final state, finalize_L(0), stats)"""
    eng = _engine(c, b, options)
    sums = []
    try:
        for it in range(8):
            sums.append(eng.step(*_step_args(c, b)).copy())
            if diag is not None and it in (2, 5):
                diag(eng)
        fin = eng.finalize_L(0) if c.latent else None
        st = eng.state()
        stats = dict(ns=eng.ns_stats(), lds=eng.lds_stats(), pipe=eng.pipeline_stats())
    finally:
        eng.close()
    return np.array(sums), st, fin, stats


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_a_diagnostic_between_two_steps_leaves_the_solve_alone(route, config):
    """Eight steps with one diagnostic call after step 3 and after step 6 against eight bare steps, one run per entry point.
    Without early parts a dropped pre-launched chain is rebuilt from the same bounds: Omega, Theta, X, L, the five sums of every
    later step, and the L and ranks of ggl_finalize_L(0) are equal in every bit.  Under default options an early first part is
    dropped rather than resumed: the iterates agree to the 1e-10 of the pipelined test of test_gpu_admm.py and stay bitwise
    symmetric."""
    c = ROUTES[route]
    b = _built(c)
    opts = CONFIGS[config]
    calls = _calls(c, b)

    def with_snapshots(fn):
        def run(e):
            for k in range(c.K):
                e.snapshot_k(k)
            fn(e)
        return run

    diags = {nm: (with_snapshots(fn) if nm in ("selection_stats", "threshold_scan", "selection_rank") else fn)
             for nm, fn in calls.items()}
    if c.latent:
        diags["finalize_L(1)"] = with_snapshots(lambda e: e.finalize_L(1))
    sums0, st0, fin0, stats0 = _solve(c, b, opts)
    # the route this case is here for
    if route == "lds":
        assert stats0["lds"]["calls"] >= 8 and stats0["lds"]["misses"] == 0, stats0
    else:
        assert stats0["lds"]["calls"] == 0 and stats0["ns"]["calls"] >= 8, stats0
    if route == "latent":
        assert stats0["ns"]["rank_calls"] >= 8 and fin0[0] == c.K, (stats0, fin0)
    for nm in ("Omega", "Theta", "X") + (("L",) if c.latent else ()):
        assert np.array_equal(st0[nm], st0[nm].transpose(0, 2, 1)), nm
    for name, diag in diags.items():
        sums, st, fin, stats = _solve(c, b, opts, diag)
        if config == "default":
            for nm in NAMES:
                assert np.abs(st[nm] - st0[nm]).max() <= 1e-10, (name, nm)
                assert np.array_equal(st[nm], st[nm].transpose(0, 2, 1)), (name, nm)
        else:
            assert np.array_equal(sums, sums0), name
            for nm in NAMES:
                assert np.array_equal(st[nm], st0[nm]), (name, nm)
            if c.latent:
                assert fin[0] == fin0[0] and np.array_equal(fin[1], fin0[1]), name
        if config == "pipeline1" and route == "chain":
            # (the chain pre-launched behind step 3 and step 6 was dropped by the call; a latent step pre-launches none)
            assert stats["pipe"]["dropped"] >= 1, (name, stats["pipe"])


# ---- the module's last tests ----------------------------------------------------------------------------------------------------
def test_worst_deviations():
    """Ends the module: the largest deviation per quantity as a share of its bound, and the largest deviation / unit behind the
    two measured constants of diag_ref.py."""
    for what, (share, dev, bound, name) in sorted(_WORST.items()):
        print(f"worst {what:10s} {dev:.3e} = {share:.3f} of its bound {bound:.3e} ({name})")
    for kind, (r, name) in sorted(_RATIO.items()):
        print(f"largest deviation / unit, {kind}: {r:.3f} ({name})")
    assert all(w[0] <= 1.0 for w in _WORST.values())


def test_every_branch_ran():
    """Between them the cases above sent the log det over its three routes, term 1 through both prox branches, terms 3 and 4
    over the LDS Jacobi eigensolver and over rocSOLVER, and the SGL thresholds through the shared and the per-instance mask."""
    print(_SEEN)
    assert all(v > 0 for v in _SEEN.values()), _SEEN
