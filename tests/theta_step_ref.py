"""Step-level reference of the Theta-step, the dual update and the five stopping-test sums (a plain helper module shared by
tests/test_cpu_theta_step_ref.py and tests/test_gpu_theta_routes.py), and the generators of the cases both files use.

``step_ref`` takes the state before a step, the parameters and the Omega the step produced (the device's own, or the oracle's)
and states what the rest of the iteration must be:

  V         = (Omega + L_0) + X_0                                 admm_solver.py:191, single_admm_solver.py:169
  Theta_ref = prox(V): prox_p (GGL / FGL, ggl_helper.py:190-207), prox_od_1norm (SGL, :16-27),
              prox_sum_Frob (FSGL, :45-66), thresholds (1 / rho) * lambda
  X_ref     = (X_0 + Omega) - Theta            non-latent         admm_solver.py:208
  C         = (Theta - X_0) - Omega, X_ref = X_0 + Omega - Theta + L      latent, :197-208
  sums      = |Omega|^2, |Theta - L|^2, |X|^2, |Omega - Theta + L|^2, |Omega - Omega_prev|^2 in numpy.longdouble   :316-331

X_ref, C and the sums are formed from the arrays they are GIVEN (the device's own upstream outputs in the GPU tests), so every
comparison isolates one kernel output and the Omega-step's iteration tolerance never enters."""
import numpy as np

from oracle import ggl_oracle as orc
import fsgl_fixtures as fx

U = 2.0 ** -53                 # unit roundoff of float64
KINK_REL = 1e-10               # |V|, group norm or block norm this close (relative to max|V|) to its threshold: no zero-pattern check


def sym(A):
    """Bitwise symmetric part of a stack (a + b is commutative in floating point)."""
    return 0.5 * (A + np.swapaxes(A, -1, -2))


def _col(v, K):
    """scalar or (K,) -> (K,1,1)"""
    return np.broadcast_to(np.asarray(v, dtype=np.float64), (K,)).reshape(K, 1, 1).copy()


class StepRef:
    """What one step must produce.  V, Theta (reference), near (elements whose zero / non-zero decision lies within KINK_REL *
    max|V| of a threshold), n (reduction length behind one element of Theta), diag_blocks (FSGL: mask of the diagonal blocks)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    # -- bounds (derived, not measured) -----------------------------------------------------------------------------------
    def theta_bound(self):
        """An n-term sum in any order errs by at most n u relative, a handful of roundings follow; the prox is non-expansive,
        so the bound holds at the kinks too."""
        return 8 * self.n * U * max(1.0, float(np.abs(self.V).max()))

    def x_bound(self, Theta, L=None):
        m = np.abs(self.X_0) + np.abs(self.Omega) + np.abs(Theta)
        if L is not None:
            m = m + np.abs(L)
        return 4 * U * float(m.max())

    # -- downstream quantities from the arrays given ----------------------------------------------------------------------
    def C(self, Theta):
        return (Theta - self.X_0) - self.Omega

    def X(self, Theta, L=None):
        if not self.latent:
            return (self.X_0 + self.Omega) - Theta
        return self.X_0 + self.Omega - Theta + L

    def sums(self, Theta, X, L=None, groups=1, pk=None):
        """(groups, 5) longdouble sums over `groups` equal consecutive parts of the stack (1: the whole stack, K: per instance,
        G: per problem) and the number of terms of one sum; pk: over the leading (pk[k], pk[k]) blocks only."""
        ld = np.longdouble
        Om, Th, Xl, Op = (np.asarray(A).astype(ld) for A in (self.Omega, Theta, X, self.Omega_prev))
        Ll = np.zeros_like(Om) if L is None else np.asarray(L).astype(ld)
        terms = np.stack([Om * Om, (Th - Ll) ** 2, Xl * Xl, (Om - Th + Ll) ** 2, (Om - Op) ** 2])     # (5,K,p,p)
        K, p = Om.shape[0], Om.shape[-1]
        if pk is not None:
            idx = np.arange(p)
            inside = (idx[None, :, None] < np.asarray(pk)[:, None, None]) & (idx[None, None, :] < np.asarray(pk)[:, None, None])
            terms = terms * inside[None]
            n_terms = (np.asarray(pk, dtype=np.int64) ** 2).reshape(groups, -1).sum(axis=1)
        else:
            n_terms = np.full(groups, (K // groups) * p * p, dtype=np.int64)
        out = terms.reshape(5, groups, -1).sum(axis=2).T
        return out, n_terms

    def sums_bound(self, n_terms):
        """relative deviation of a float64 sum of N non-negative terms, each with a few roundings of its own"""
        return (np.asarray(n_terms, dtype=np.float64)[:, None] + 4.0) * U

    def nonzero_fraction(self):
        K, p = self.Theta.shape[0], self.Theta.shape[-1]
        off = ~np.eye(p, dtype=bool)
        return np.count_nonzero(self.Theta[:, off]) / float(K * off.sum())


def step_ref(reg, Omega_prev, Theta_0, X_0, L_0, Omega, rho, lambda1, lambda2=None, M=None, mask=None, latent=False, G=1):
    """reg: 'GGL' | 'FGL' | 'SGL' | 'FSGL'.  rho, lambda1, lambda2: scalars, or one value per instance (SGL / FSGL batches) or
    per problem (G problems of K/G instances, GGL / FGL).  mask: (p,p) or (K,p,p) array lambda1 * lambda1_mask (SGL; it
    replaces lambda1, as set_lambda1_mask / set_lambda1_mask_k).  Theta_0 is part of the state before the step and is kept
    for completeness: it enters the Omega-step only."""
    Omega = np.asarray(Omega, dtype=np.float64)
    K, p = Omega.shape[0], Omega.shape[-1]
    L0 = np.zeros_like(Omega) if L_0 is None else np.asarray(L_0, dtype=np.float64)
    V = (Omega + L0) + X_0
    vmax = float(np.abs(V).max())
    tol = KINK_REL * vmax
    off = ~np.eye(p, dtype=bool)
    near = np.zeros(V.shape, dtype=bool)
    diag_blocks = None
    if reg in ("GGL", "FGL"):
        Kp = K // G
        rho_g, l1_g, l2_g = (np.broadcast_to(np.asarray(v, dtype=np.float64), (G,)) for v in (rho, lambda1, lambda2))
        Theta = np.empty_like(V)
        for g in range(G):
            sl = slice(g * Kp, (g + 1) * Kp)
            l1, l2 = (1 / rho_g[g]) * l1_g[g], (1 / rho_g[g]) * l2_g[g]
            Theta[sl] = orc.prox_p(V[sl], l1, l2, reg)
            if reg == "GGL":
                Us = orc.prox_1norm(V[sl], l1)
                gn = np.sqrt((Us * Us).sum(axis=0))
                near[sl] = (np.abs(np.abs(V[sl]) - l1) <= tol) | (np.abs(gn - l2) <= tol)[None]
            else:
                # prox_1norm(prox_tv(v)): the total-variation prox is continuous, the decision is |tv| against l1; the reference
                # leaves tv = Theta + sign * l1 where Theta != 0, and a second statement of it where Theta == 0
                tv = orc.prox_p(V[sl], 1e-300, l2, reg)
                near[sl] = np.abs(np.abs(tv) - l1) <= tol
        near &= off[None]
        n = Kp
    elif reg == "SGL":
        if mask is not None:
            thr = (1 / _col(rho, K)) * np.broadcast_to(np.asarray(mask, dtype=np.float64), V.shape)
        else:
            thr = np.broadcast_to((1 / _col(rho, K)) * _col(lambda1, K), V.shape)
        Theta = np.stack([orc.prox_od_1norm(V[k], thr[k]) for k in range(K)])
        near = (np.abs(np.abs(V) - thr) <= tol) & off[None]
        n = 1
    elif reg == "FSGL":
        lk = ((1 / _col(rho, K)) * _col(lambda1, K)).reshape(K)
        Theta = np.stack([fx.prox_sum_frob_np(V[k], M, lk[k]) for k in range(K)])
        pb = p // M
        blk = np.arange(p) // M
        diag_blocks = blk[:, None] == blk[None, :]
        for k in range(K):
            bn = fx.block_norms(V[k], M)
            bn = np.triu(bn, 1) + np.triu(bn, 1).T              # the upper block decides for its mirror
            nb = (np.abs(bn - lk[k]) <= tol) & ~np.eye(pb, dtype=bool)
            near[k] = np.repeat(np.repeat(nb, M, axis=0), M, axis=1)
        n = M * M
    else:
        raise ValueError(reg)
    return StepRef(reg=reg, V=V, Theta=Theta, near=near, n=n, latent=bool(latent), Omega=Omega, Omega_prev=np.asarray(Omega_prev),
                   Theta_0=Theta_0, X_0=np.asarray(X_0), L_0=L0, diag_blocks=diag_blocks, K=K, p=p)


# ---- the cases: starts and thresholds, shared by the CPU and the GPU test ------------------------------------------------------
def make_start(K, p, seed, latent=False, pk=None):
    """A non-trivial, bitwise symmetric start: Theta_0 = I + 0.1 sym(noise), X_0 = 0.05 sym(noise), Omega_0 = I + 0.05 sym(noise),
    L_0 a small PSD matrix of rank 2 where latent (else None).  pk: instance k is the leading (pk[k], pk[k]) block of an
    identity-padded slot (Theta_0 = Omega_0 = I, X_0 = 0 behind it)."""
    rng = np.random.default_rng(seed)
    eye = np.eye(p)[None]
    Theta_0 = eye + 0.1 * sym(rng.standard_normal((K, p, p)))
    X_0 = 0.05 * sym(rng.standard_normal((K, p, p)))
    Omega_0 = eye + 0.05 * sym(rng.standard_normal((K, p, p)))
    L_0 = None
    if latent:
        B = 0.2 * rng.standard_normal((K, p, 2))
        L_0 = sym(B @ B.transpose(0, 2, 1))
    if pk is not None:
        for k, q in enumerate(pk):
            for A, fill in ((Theta_0, 1.0), (Omega_0, 1.0), (X_0, 0.0)):
                A[k, q:, :] = 0.0
                A[k, :, q:] = 0.0
                A[k, np.arange(q, p), np.arange(q, p)] = fill
    return Omega_0, Theta_0, X_0, L_0


def pad_S(S, pk):
    """S with instance k cut to its leading (pk[k], pk[k]) block and padded with the identity."""
    S = S.copy()
    p = S.shape[-1]
    for k, q in enumerate(pk):
        S[k, q:, :] = 0.0
        S[k, :, q:] = 0.0
        S[k, np.arange(q, p), np.arange(q, p)] = 1.0
    return S


def omega_cpu(S, Theta_0, X_0, L_0, rho, nk=None):
    """The oracle's Omega-step (admm_solver.py:180-187) from the start point; rho scalar or per instance."""
    K = S.shape[0]
    beta = (np.ones(K) if nk is None else np.asarray(nk, dtype=np.float64)) / np.broadcast_to(np.asarray(rho, dtype=np.float64), (K,))
    W = Theta_0 - (0.0 if L_0 is None else L_0) - X_0 - beta[:, None, None] * S
    return orc.phiplus_stack(W, beta)[0]


def _upper(V):
    iu = np.triu_indices(V.shape[-1], 1)
    return V[..., iu[0], iu[1]]


def _between(x, q):
    """a value strictly between two neighbouring order statistics of x around its q-quantile (never a sample itself, so no
    element sits on its threshold by construction)"""
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    i = min(max(int(q * len(x)), 1), len(x) - 1)
    return 0.5 * float(x[i - 1] + x[i])


def draw_mgl_thresholds(reg, V):
    """(l1, l2) = (lambda1, lambda2) / rho for one problem so that roughly half of the entries and groups survive: V is the
    Theta-step's input with the oracle's Omega."""
    A = np.abs(_upper(V))                                     # (K, pairs)
    if reg == "GGL":
        l1 = _between(A, 0.3)
        gn = np.sqrt((np.maximum(A - l1, 0.0) ** 2).sum(axis=0))
        return l1, _between(gn, 0.5)
    d = np.abs(np.diff(_upper(V), axis=0)) if V.shape[0] > 1 else A
    return _between(A, 0.4), 0.25 * float(np.median(d))


def draw_sgl_thresholds(V, quantiles, pk=None):
    """one l1 / rho per instance: the given quantile of the |off-diagonal| of its leading block (a 1 x 1 block has none and
    takes instance 0's entries)"""
    out = []
    for k, q in enumerate(quantiles):
        n = V.shape[-1] if pk is None else int(pk[k])
        out.append(_between(np.abs(_upper(V[k if n > 1 else 0][:max(n, 2), :max(n, 2)] if n > 1 else V[0])), q))
    return np.array(out)


def draw_fsgl_threshold(V, M, where="inside"):
    """l1 / rho against the norms of the upper off-diagonal blocks of the whole stack: 'inside' halfway between the two middle
    ones, 'above' all of them, 'below' all of them"""
    pb = V.shape[-1] // M
    iu = np.triu_indices(pb, 1)
    norms = np.sort(np.concatenate([fx.block_norms(V[k], M)[iu] for k in range(V.shape[0])]))
    if where == "above":
        return 1.5 * float(norms[-1])
    if where == "below":
        return 0.5 * float(norms[0])
    m = len(norms) // 2
    return 0.5 * float(norms[m - 1] + norms[m]) if len(norms) > 1 else 0.5 * float(norms[0])


class Case:
    """One route case.  kind: 'step' (HipEngine.step), 'mgl_batch' (mgl_batch_step, G problems), 'sgl_batch' (sgl_batch_step; with
    M the Functional SGL batch).  code: the dispatch code the Theta-step must report (None: k_theta_sgl and the fused LDS
    iteration have none)."""

    def __init__(self, name, kind, reg, K, p, code, opts=None, latent=False, M=None, G=1, mask=None, pk=None, fused=False):
        self.name, self.kind, self.reg, self.K, self.p, self.code = name, kind, reg, K, p, code
        self.opts, self.latent, self.M, self.G, self.mask, self.pk, self.fused = opts or {}, latent, M, G, mask, pk, fused

    @property
    def seed(self):
        return 5000 + 31 * self.K + self.p + (7 if self.latent else 0)


RHO_STEP = 1.7
RHO_BATCH = (0.8, 1.7, 2.5)


def build_case(c):
    """Everything a case needs, host side: S (synth.make_problem), the start, rho, the thresholds drawn against the Theta-step
    input formed with the ORACLE's Omega (kept as 'Omega_cpu'), the masks and dimensions."""
    from gglasso_amd import synth
    K, p = c.K, c.p
    S, _ = synth.make_problem("SGL" if c.reg in ("SGL", "FSGL") else c.reg, K, p, seed=c.seed)
    pk = None if c.pk is None else np.asarray(c.pk, dtype=np.int32)
    if pk is not None:
        S = pad_S(S, pk)
    Omega_0, Theta_0, X_0, L_0 = make_start(K, p, c.seed + 1, c.latent, pk)
    batch = c.kind != "step"
    n_par = c.G if c.kind == "mgl_batch" else K
    rho = np.array([RHO_BATCH[i % 3] for i in range(n_par)]) if batch else RHO_STEP
    rho_K = np.repeat(rho, K // n_par) if batch else np.full(K, rho)
    Om = omega_cpu(S, Theta_0, X_0, L_0, rho_K)
    V = (Om + (0.0 if L_0 is None else L_0)) + X_0
    out = dict(S=S, Omega_0=Omega_0, Theta_0=Theta_0, X_0=X_0, L_0=L_0, rho=rho, Omega_cpu=Om, pk=pk, mask=None, lambda2=None,
               mu1=np.full(K, 0.2) if c.latent else None)
    if c.reg in ("GGL", "FGL"):
        Kp = K // c.G
        l = np.array([draw_mgl_thresholds(c.reg, V[g * Kp:(g + 1) * Kp]) for g in range(c.G)])
        # different problems, different thresholds: scaled apart so that a launch that took problem 0's would be far off
        scale = np.array([1.0, 0.7, 1.4])[:c.G]
        lam1, lam2 = l[:, 0] * scale * rho, l[:, 1] * scale[::-1] * rho
        out["lambda1"], out["lambda2"] = (lam1, lam2) if batch else (float(lam1[0]), float(lam2[0]))
    elif c.reg == "SGL":
        q = (0.35, 0.5, 0.65)
        l = draw_sgl_thresholds(V, [q[k % 3] for k in range(K)], pk)
        out["lambda1"] = l * rho
        if c.mask is not None:
            rng = np.random.default_rng(c.seed + 2)
            m0 = sym(rng.uniform(0.5, 1.5, (K if c.mask == "k" else 1, p, p)))
            # the mask arrays carry lambda1 (set_lambda1_mask: lambda1 * lambda1_mask); the kernel scales them by 1 / rho_k
            lam = l * rho if c.mask == "k" else np.full(1, float(np.median(l * rho)))
            out["mask"] = lam[:, None, None] * m0 if c.mask == "k" else lam[0] * m0[0]
    else:
        if batch:
            l = np.array([draw_fsgl_threshold(V[k:k + 1], c.M, w) for k, w in zip(range(K), ("inside", "above", "below"))])
            out["lambda1"] = l * rho
        else:
            out["lambda1"] = draw_fsgl_threshold(V, c.M) * rho
    return out


def ref_of(c, b, Omega, Omega_prev=None):
    """step_ref of a built case for the Omega given"""
    return step_ref(c.reg, b["Omega_0"] if Omega_prev is None else Omega_prev, b["Theta_0"], b["X_0"], b["L_0"], Omega, b["rho"],
                    b["lambda1"], b["lambda2"], M=c.M, mask=b["mask"], latent=c.latent, G=c.G)


def fsgl_code(M):
    return 4000 + M * (32 // M) if M <= 32 else 5032


def _cases():
    C = Case
    out = []
    # GGL, theta_flat = 2 (default)
    for K, p, code in ((8, 23, 108), (9, 17, 404), (16, 16, 404), (17, 19, 408), (32, 12, 408), (33, 15, 808), (64, 13, 808),
                       (65, 11, 10216), (128, 8, 10216), (129, 9, 10416), (256, 7, 10416), (65, 180, 10216), (65, 181, 816),
                       (129, 181, 1616)):
        out.append(C(f"ggl-K{K}-p{p}", "step", "GGL", K, p, code))
    # other theta_flat settings; (51, 161): six tiles, ggl_chunks = 26 chunks of two instances, the last one holds one
    out += [C("ggl-flat1-K9-p17", "step", "GGL", 9, 17, 116, {"theta_flat": 1}),
            C("ggl-flat1-K17-p19", "step", "GGL", 17, 19, 132, {"theta_flat": 1}),
            C("ggl-flat0-K3-p33", "step", "GGL", 3, 33, 0, {"theta_flat": 0}),
            C("ggl-flat0-K51-p161", "step", "GGL", 51, 161, 0, {"theta_flat": 0})]
    # latent: the Theta kernel writes C, then the L-step and k_dual_update
    out += [C("ggl-latent-K9-p17", "step", "GGL", 9, 17, 404, latent=True),
            C("ggl-latent-K65-p11", "step", "GGL", 65, 11, 10216, latent=True),
            C("ggl-latent-K33-p15", "step", "GGL", 33, 15, 808, latent=True),
            C("ggl-latent-flat0-K3-p33", "step", "GGL", 3, 33, 0, {"theta_flat": 0}, latent=True)]
    # FGL
    out += [C("fgl-K5-p13", "step", "FGL", 5, 13, 3128), C("fgl-K149-p9", "step", "FGL", 149, 9, 3128),
            C("fgl-K150-p9", "step", "FGL", 150, 9, 3064), C("fgl-Kmax-p6", "step", "FGL", FGL_MAX_K, 6, 3064),
            C("fgl-flat0-K5-p17", "step", "FGL", 5, 17, 2016, {"theta_flat": 0}),
            C("fgl-flat0-K32-p17", "step", "FGL", 32, 17, 2016, {"theta_flat": 0}),
            C("fgl-flat0-K33-p9", "step", "FGL", 33, 9, 2008, {"theta_flat": 0}),
            C("fgl-latent-K5-p13", "step", "FGL", 5, 13, 3128, latent=True),
            C("fgl-latent-flat0-K5-p17", "step", "FGL", 5, 17, 2016, {"theta_flat": 0}, latent=True)]
    # mgl_batch_step: G = 3 problems with their own (rho, lambda1, lambda2), odd p
    out += [C("mglb-ggl-Kp4", "mgl_batch", "GGL", 12, 13, 108, G=3), C("mglb-ggl-Kp12", "mgl_batch", "GGL", 36, 13, 404, G=3),
            C("mglb-ggl-Kp20", "mgl_batch", "GGL", 60, 13, 408, G=3), C("mglb-fgl-Kp5", "mgl_batch", "FGL", 15, 13, 3128, G=3),
            C("mglb-ggl-latent-Kp12", "mgl_batch", "GGL", 36, 13, 404, G=3, latent=True),
            # the 16-wave kernels under blockIdx.y > 0 and l1G / l2G; (129, 7): 49 elements, the first 64-element chunk of the
            # only workgroup partly live, its second chunk dead
            C("mglb-ggl-Kp65", "mgl_batch", "GGL", 195, 13, 816, G=3), C("mglb-ggl-Kp129", "mgl_batch", "GGL", 387, 7, 1616, G=3)]
    # sgl_batch_step: K = 3 instances with their own (rho_k, lambda1_k)
    out += [C("sglb-p65", "sgl_batch", "SGL", 3, 65, None), C("sglb-p64-fused", "sgl_batch", "SGL", 3, 64, None, fused=True),
            C("sglb-p33-fused", "sgl_batch", "SGL", 3, 33, None, fused=True),
            C("sglb-p65-latent", "sgl_batch", "SGL", 3, 65, None, latent=True),
            C("sglb-p65-mask", "sgl_batch", "SGL", 3, 65, None, mask="shared"),
            C("sglb-p65-maskk-pk", "sgl_batch", "SGL", 3, 65, None, mask="k", pk=(65, 60, 1)),
            C("sglb-p33-maskk-pk-fused", "sgl_batch", "SGL", 3, 33, None, mask="k", pk=(33, 28, 1), fused=True)]
    # FSGL through step (two instances, so that a two-block matrix still has a block on either side of the threshold)
    for M, pM in ((1, 33), (3, 69), (5, 65), (7, 70), (16, 80), (32, 96), (33, 99), (40, 120), (64, 128), (65, 130)):
        out.append(C(f"fsgl-M{M}-pM{pM}", "step", "FSGL", 2, pM, fsgl_code(M), M=M))
    for M, pM in ((5, 65), (33, 99), (65, 130)):
        out.append(C(f"fsgl-latent-M{M}-pM{pM}", "step", "FSGL", 2, pM, fsgl_code(M), M=M, latent=True))
    for M, pM in ((5, 65), (33, 99)):
        out.append(C(f"fsglb-M{M}-pM{pM}", "sgl_batch", "FSGL", 3, pM, fsgl_code(M), M=M))
    return out


FGL_MAX_K = (160 * 1024 - 1024) // (8 * 8 * 8)      # K-vectors of an 8 x 8 tile in 159 KiB of LDS (ggl_theta_limits()['FGL'])
CASES = _cases()
# every dispatch code of the Theta-step launchers (theta_pair.hip: g_theta_kernel; theta_fsgl.hip: 4000 + T / 5000 + 32)
ALL_CODES = {0, 108, 116, 132, 404, 408, 808, 816, 1616, 10216, 10416, 2016, 2008, 3128, 3064, 4032, 4030, 4028, 5032}
