"""Step-level reference of one ext_ADMM_MGL iteration after the Omega-step (csrc/ext_group.hip: k_ext_theta, k_ext_group,
k_ext_dual; csrc/capi_ext.hip: ext_finish), and the cases tests/test_cpu_ext_step_ref.py and tests/test_gpu_ext_step.py share.

``ext_ref`` takes the padded (K,P,P) state before the step (Omega_prev, Theta, L, X0, X1, Lambda), the parameters and the Omega
the step produced, and states in numpy.longdouble, over the full padded arrays (solver/ext_admm_solver.py:196-231, :325-345):

  V          = (Omega + L + X0 + Lambda - X1) / 2
  Theta      = prox_od_1norm(V, lambda1_k / (2 rho))                       per instance slot k
  C          = Theta - X0 - Omega                                          latent: what the L-step eats
  Z          = Theta + X1
  Lambda_new = prox_2norm_G(Z, G, lambda2_g / rho)                         per group and per problem g of a batch
  X0_new     = X0 + Omega - Theta + L,   X1_new = X1 + Theta - Lambda_new
  sums       = |Omega|^2 + |Lambda|^2, |Theta - L|^2 + |Theta|^2, |X0|^2 + |X1|^2, |Omega - Theta + L|^2 + |Lambda - Theta|^2,
               |Omega - Omega_prev|^2 + |Lambda - Lambda_prev|^2           per problem, leading (p_k,p_k) blocks only

Each downstream quantity is formed from the arrays it is GIVEN (in the GPU test the device's own upstream output: Theta from the
device's Omega, Lambda from the device's Theta, X0 / X1 and the sums from the device's Theta, L and Lambda), so every comparison
isolates one kernel output and the Omega- / L-step's iteration tolerance never enters.

Bounds (derived, u = 2^-53):
  Theta                    <= 8 u max(1, max(|Omega| + |L| + |X0| + |Lambda| + |X1|))    four additions and a halving; the prox is
                              non-expansive, so the bound holds at the kinks too
  Lambda outside a group   <= 2 u max|Z|                                                 Z = Theta + X1 is one rounding
  Lambda, group of size n  <= (n + 10) u |z_in| for every member, absolute: an n-term sum of squares under a root errs by
                              (n/2 + 2) u relative, the threshold lambda2 / rho * sqrt(n) by three roundings, and a - lam cancels:
                              the error of the difference is bounded against a, so the member's error against its INPUT entry
                              z_in, not against the output (which may be arbitrarily smaller)
  X0, X1                   <= 4 u (|X0| + |Omega| + |Theta| + |L|), 4 u (|X1| + |Theta| + |Lambda|), elementwise
  sums                     relative deviation from the longdouble value <= (N + 8) u, N the number of terms: every term is a square of a
                              difference of up to three addends (up to four roundings of its own; the suite uses (N + 4) u for
                              single-rounding terms), then N additions in any order

Start states: random bitwise symmetric leading blocks, L PSD of rank 2 when latent (else zero), the padding at the iteration's
fixed point (identity in S, Omega, Theta, Lambda; zero in L, X0, X1).  Every problem of a batch has its own state, its own lambda1
per slot and its own lambda2.  Groups: distinct upper-triangle entries drawn per instance, sizes 1 .. K."""
import numpy as np

from oracle import ggl_oracle as orc
from theta_step_ref import KINK_REL, U, _between, omega_cpu, pad_S, sym

XCHUNK = 1024                  # elements per workgroup of k_ext_theta / k_ext_dual / k_ext_sq (ext_group.hip: XT * XE)
GROUP_WG = 256                 # groups per workgroup of k_ext_group
RHO = 1.7
LD = np.longdouble


def nblk(P):
    return -(-P * P // XCHUNK)


def inside_mask(pk, P):
    """(K,P,P) bool: the leading (p_k,p_k) block of every slot"""
    idx = np.arange(P)
    q = np.asarray(pk)[:, None, None]
    return (idx[None, :, None] < q) & (idx[None, None, :] < q)


def padding_masks(pk, P):
    """(cross, trailing): row < p_k <= column and its mirror; the trailing diagonal block"""
    idx = np.arange(P)
    q = np.asarray(pk)[:, None, None]
    r, c = idx[None, :, None], idx[None, None, :]
    return ((r < q) & (c >= q)) | ((r >= q) & (c < q)), (r >= q) & (c >= q)


class Case:
    """pk: the instance dimensions of ONE problem; nprob problems share them and the group table of L groups."""

    def __init__(self, name, P, pk, L, latent=False, nprob=1, steps=1, opts=None):
        self.name, self.P, self.pk, self.L, self.latent, self.nprob = name, P, tuple(pk), L, latent, nprob
        self.Kp, self.K = len(pk), len(pk) * nprob
        self.steps, self.opts = steps, opts or {}
        assert max(pk) == P

    @property
    def seed(self):
        return 7000 + 131 * self.P + 17 * self.L + 5 * self.K + (3 if self.latent else 0)

    @property
    def padded(self):
        return min(self.pk) < self.P


def _cases():
    C = Case
    out = []
    for lat in (False, True):
        t = "-latent" if lat else ""
        out += [C(f"P8-jacobi{t}", 8, (8, 5, 2, 1), 20, lat),             # Jacobi Omega route (p <= GGL_NS_MIN_P), pk = 1 holds no pair
                C(f"P32-one-full-chunk{t}", 32, (32, 20, 31), 300, lat),
                C(f"P33-two-chunks{t}", 33, (33, 17, 32), 257, lat),       # the last chunk holds 65 elements
                C(f"P46-three-chunks-L600{t}", 46, (46, 33, 40, 2), 600, lat)]
    out.append(C("P72-newton-schulz", 72, (72, 50, 64), 400, steps=3))     # the launch chain: steps 2 and 3 speculate
    out += [C(f"P46-L{L}", 46, (46, 33, 40, 2), L) for L in (0, 1, 256, 257)]
    out.append(C("K1-groups-of-one", 9, (9,), 20))
    for lat in (False, True):
        t = "-latent" if lat else ""
        out += [C(f"batch3x2-P20{t}", 20, (17, 20), 257, lat, nprob=3),
                C(f"batch2x3-P33{t}", 33, (33, 17, 32), 257, lat, nprob=2),
                C(f"batch3x2-P46{t}", 46, (33, 46), 257, lat, nprob=3)]
    return out


CASES = _cases()
SINGLE = [c for c in CASES if c.nprob == 1]
BATCH = [c for c in CASES if c.nprob > 1]
SPEC_CASE = next(c for c in CASES if c.P == 72)


# ---- groups ------------------------------------------------------------------------------------------------------------------
def draw_groups(rng, pk, L):
    """(2,L,K) int bookkeeping array: every group holds distinct upper-triangle entries (i < j < p_k) of 1 .. K instances, no entry
    twice (a first pass gives every group one member, a second one fills up to the size drawn)."""
    K = len(pk)
    G = -np.ones((2, L, K), dtype=int)
    pairs = []
    for q in pk:
        iu = np.triu_indices(int(q), 1)
        order = rng.permutation(len(iu[0]))
        pairs.append(list(zip(iu[0][order], iu[1][order])))
    assert sum(len(x) for x in pairs) >= L, "more groups than entries"
    for l in range(L):
        left = np.array([len(x) for x in pairs], dtype=float)
        k = int(rng.choice(K, p=left / left.sum()))
        G[0, l, k], G[1, l, k] = pairs[k].pop()
    for l in range(L):
        want = int(rng.integers(1, K + 1))
        for k in rng.permutation(K):
            if (G[0, l] >= 0).sum() >= want:
                break
            if G[0, l, k] < 0 and pairs[k]:
                G[0, l, k], G[1, l, k] = pairs[k].pop()
    return G


def prox_2norm_G_ld(Z, G, l2):
    """prox_2norm_G (ext_admm_solver.py:394-453) of one problem's padded (Kp,P,P) longdouble stack, groups without repeated
    entries: (Lambda, group norms, thresholds l2 * sqrt(size))."""
    out = Z.copy()
    L = G.shape[1]
    present = G[0] >= 0
    size = present.sum(axis=1)
    gn, lam = np.zeros(L, dtype=LD), LD(l2) * np.sqrt(size.astype(LD))
    for l in range(L):
        ks = np.flatnonzero(present[l])
        i, j = G[0, l, ks], G[1, l, ks]
        v = Z[ks, i, j]
        gn[l] = np.sqrt((v * v).sum())
        a = max(gn[l], lam[l])
        z = v * (a - lam[l]) / a
        out[ks, i, j] = z
        out[ks, j, i] = z
    return out, gn, lam


class ExtRef:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    # -- Theta ----------------------------------------------------------------------------------------------------------------
    def theta_bound(self):
        return 8 * U * max(1.0, float(self.mag.max()))

    def theta_zero_fraction(self):
        off = ~np.eye(self.P, dtype=bool)
        m = self.inside & off[None]
        return float((self.Theta[m] == 0).mean())

    # -- downstream, from the arrays given ------------------------------------------------------------------------------------
    def C(self, Theta):
        return np.asarray((LD(1) * Theta - self.X0) - self.Omega, dtype=np.float64)

    def lam(self, Theta):
        """Lambda_new from the Theta given: dict(Lambda float64, Z longdouble, zeroed (nprob,L) bool, near (nprob,L) bool: the
        group's norm within KINK_REL relative of its threshold)"""
        Z = np.asarray(Theta).astype(LD) + self.X1
        Lam = Z.copy()
        L, Kp = self.G.shape[1], self.Kp
        zeroed, near = np.zeros((self.nprob, L), dtype=bool), np.zeros((self.nprob, L), dtype=bool)
        for g in range(self.nprob):
            sl = slice(g * Kp, (g + 1) * Kp)
            Lam[sl], gn, thr = prox_2norm_G_ld(Z[sl], self.G, LD(self.lambda2[g]) / LD(self.rho))
            zeroed[g] = gn <= thr
            near[g] = np.abs(gn - thr) <= KINK_REL * thr
        return dict(Lambda=np.asarray(Lam, dtype=np.float64), Z=Z, zeroed=zeroed, near=near)

    def lam_bound(self, Z):
        """(K,P,P) absolute bound of Lambda_new"""
        out = np.full(Z.shape, 2 * U * float(np.abs(Z).max()))
        zin = np.asarray(np.abs(Z), dtype=np.float64)
        out[self.in_group] = ((self.gsize + 10) * U * zin)[self.in_group]
        return out

    def X0n(self, Theta, L):
        """longdouble (rounding the reference to float64 would spend one of the bound's four roundings)"""
        return self.X0 + self.Omega - np.asarray(Theta).astype(LD) + np.asarray(L).astype(LD)

    def X1n(self, Theta, Lam):
        return self.X1 + np.asarray(Theta).astype(LD) - np.asarray(Lam).astype(LD)

    def x0_bound(self, Theta, L):
        return 4 * U * np.asarray(np.abs(self.X0) + np.abs(self.Omega) + np.abs(Theta) + np.abs(L), dtype=np.float64)

    def x1_bound(self, Theta, Lam):
        return 4 * U * np.asarray(np.abs(self.X1) + np.abs(Theta) + np.abs(Lam), dtype=np.float64)

    def sums(self, Theta, L, Lam, X0n, X1n):
        """(nprob,5) longdouble sums over the leading blocks and the number of terms of one sum, per problem"""
        Th, Ll, La, A0, A1 = (np.asarray(A).astype(LD) for A in (Theta, L, Lam, X0n, X1n))
        Om = self.Omega
        t = np.stack([Om * Om + La * La, (Th - Ll) ** 2 + Th * Th, A0 * A0 + A1 * A1, (Om - Th + Ll) ** 2 + (La - Th) ** 2,
                      (Om - self.Omega_prev) ** 2 + (La - self.Lambda) ** 2])
        t = t * self.inside[None]
        out = t.reshape(5, self.nprob, -1).sum(axis=2).T
        n_terms = 2 * (np.asarray(self.pk_all, dtype=np.int64) ** 2).reshape(self.nprob, -1).sum(axis=1)
        return out, n_terms

    @staticmethod
    def sums_bound(n_terms):
        return (np.asarray(n_terms, dtype=np.float64)[:, None] + 8.0) * U


def ext_ref(state, Omega, pk_all, G, nprob, rho, lambda1, lambda2):
    """state: dict Omega (the previous one), Theta, L, X0, X1, Lambda, padded (K,P,P); Omega: the step's own; pk_all (K,); G (2,L,Kp);
    lambda1 (K,) per slot; lambda2 (nprob,) per problem."""
    Om = np.asarray(Omega).astype(LD)
    K, P = Om.shape[0], Om.shape[-1]
    Kp = K // nprob
    L0, X0, X1, Lam0 = (np.asarray(state[nm]).astype(LD) for nm in ("L", "X0", "X1", "Lambda"))
    V = (Om + L0 + X0 + Lam0 - X1) / 2
    thr = (np.asarray(lambda1).astype(LD) / (2 * LD(rho))).reshape(K, 1, 1)
    Th = np.sign(V) * np.maximum(np.abs(V) - thr, 0)
    d = np.arange(P)
    Th[:, d, d] = V[:, d, d]
    off = ~np.eye(P, dtype=bool)
    near = (np.abs(np.abs(V) - thr) <= KINK_REL * float(np.abs(V).max())) & off[None]
    mag = np.asarray(np.abs(Om) + np.abs(L0) + np.abs(X0) + np.abs(Lam0) + np.abs(X1), dtype=np.float64)
    in_group = np.zeros((K, P, P), dtype=bool)
    gsize = np.zeros((K, P, P))
    size = (G[0] >= 0).sum(axis=1)
    for g in range(nprob):
        for k in range(Kp):
            m = G[0, :, k] >= 0
            i, j = G[0, m, k], G[1, m, k]
            for a, b in ((i, j), (j, i)):
                in_group[g * Kp + k, a, b] = True
                gsize[g * Kp + k, a, b] = size[m]
    return ExtRef(V=V, Theta=np.asarray(Th, dtype=np.float64), near=near, mag=mag, Omega=Om, Omega_prev=np.asarray(state["Omega"]).astype(LD),
                  X0=X0, X1=X1, Lambda=Lam0, L0=L0, inside=inside_mask(pk_all, P), pk_all=np.asarray(pk_all), G=G, nprob=nprob,
                  Kp=Kp, K=K, P=P, rho=rho, lambda1=np.asarray(lambda1), lambda2=np.atleast_1d(np.asarray(lambda2, dtype=np.float64)),
                  in_group=in_group, gsize=gsize, group_size=size)


# ---- the cases, host side ----------------------------------------------------------------------------------------------------
def make_state(rng, K, P, pk_all, latent):
    """Bitwise symmetric leading blocks, the padding at the fixed point"""
    eye = np.eye(P)[None]
    inside = inside_mask(pk_all, P)
    st = dict(Omega=eye + 0.05 * sym(rng.standard_normal((K, P, P))), Theta=eye + 0.1 * sym(rng.standard_normal((K, P, P))),
              X0=0.05 * sym(rng.standard_normal((K, P, P))), X1=0.05 * sym(rng.standard_normal((K, P, P))),
              Lambda=eye + 0.1 * sym(rng.standard_normal((K, P, P))), L=np.zeros((K, P, P)))
    if latent:
        B = 0.2 * rng.standard_normal((K, P, 2))
        B[np.arange(P)[None, :] >= np.asarray(pk_all)[:, None]] = 0.0          # rank 2 inside the leading block, zero behind it
        st["L"] = sym(B @ B.transpose(0, 2, 1))
    for nm, fill in (("Omega", 1.0), ("Theta", 1.0), ("Lambda", 1.0), ("X0", 0.0), ("X1", 0.0), ("L", 0.0)):
        st[nm] = np.where(inside, st[nm], fill * eye)
    return st


def omega_of(S, state, rho):
    """the Omega-step by eigendecomposition (ext_admm_solver.py:200-205) from a padded state"""
    return omega_cpu(S, state["Theta"], state["X0"], state["L"], rho)


def build_case(c):
    """S, the start state, G, and the thresholds drawn against the Theta-step's input formed with the ORACLE's Omega ('Omega_cpu'):
    lambda1 per slot at its own quantile of |V|'s leading off-diagonal entries, lambda2 per problem at its own quantile of the group
    norms over sqrt(group size) -- never a sample itself, so nothing sits on its threshold by construction."""
    from gglasso_amd import synth
    rng = np.random.default_rng(c.seed)
    K, P = c.K, c.P
    pk_all = np.tile(np.asarray(c.pk, dtype=np.int32), c.nprob)
    S = pad_S(synth.make_problem("GGL", K, P, seed=c.seed)[0], pk_all)
    state = make_state(rng, K, P, pk_all, c.latent)
    G = draw_groups(rng, c.pk, c.L)
    Om = omega_of(S, state, RHO)
    V = (Om + state["L"] + state["X0"] + state["Lambda"] - state["X1"]) / 2
    q1 = (0.35, 0.5, 0.65, 0.45, 0.6, 0.4, 0.55)
    thr = np.zeros(K)
    for k in range(K):
        q = int(pk_all[k])
        src = V[k, :q, :q] if q > 1 else V[0, :int(pk_all[0]), :int(pk_all[0])]      # a 1 x 1 block holds no pair
        iu = np.triu_indices(src.shape[0], 1)
        # (a 2 x 2 block holds one pair: half of it, so that the pair survives and sits nowhere near the threshold)
        thr[k] = _between(np.abs(src[iu]), q1[k % len(q1)]) if len(iu[0]) > 1 else 0.5 * float(np.abs(src[iu][0]))
    lambda1 = thr * 2 * RHO
    Th = np.stack([orc.prox_od_1norm(V[k], thr[k]) for k in range(K)])
    Z = Th + state["X1"]
    q2 = (0.4, 0.6, 0.5)
    lambda2 = np.ones(c.nprob)
    size = (G[0] >= 0).sum(axis=1)
    for g in range(c.nprob):
        if c.L == 0:
            lambda2[g] = 0.05 * (g + 1)
            continue
        ratio = np.zeros(c.L)
        for l in range(c.L):
            ks = np.flatnonzero(G[0, l] >= 0)
            ratio[l] = np.sqrt((Z[g * c.Kp + ks, G[0, l, ks], G[1, l, ks]] ** 2).sum() / size[l])
        # one group alone: it survives, shrunk to half its norm
        lambda2[g] = (0.5 * ratio[0] if c.L == 1 else _between(ratio, q2[g % 3])) * RHO
    return dict(S=S, state=state, G=G, pk_all=pk_all, rho=RHO, lambda1=lambda1, lambda2=lambda2, Omega_cpu=Om,
                mu1=np.array([0.2 + 0.03 * (k % 4) for k in range(K)]) if c.latent else None)


def ref_of(c, b, Omega, state=None):
    return ext_ref(b["state"] if state is None else state, Omega, b["pk_all"], b["G"], c.nprob, b["rho"], b["lambda1"], b["lambda2"])


def check_inputs(c, b, ref, first_step=True, strict=True):
    """The conditions on a case's inputs, for the Omega behind `ref` (the oracle's in the CPU test: strict, nothing on a threshold;
    the device's in the GPU test, which may leave a 1e-4 share out of its zero-pattern checks); returns Lambda's reference pieces
    (ExtRef.lam of the reference's Theta)."""
    lm = ref.lam(ref.Theta)
    share = 0.0 if strict else 1e-4
    assert ref.near.mean() <= share, "elements of V on their threshold"
    assert (lm["near"].mean() if c.L else 0.0) <= share, "group norms on their threshold"
    if first_step:
        f = ref.theta_zero_fraction()
        assert 0.1 <= f <= 0.9, f
        if c.L >= 10:
            for g in range(c.nprob):
                assert 0.1 <= lm["zeroed"][g].mean() <= 0.9, (g, lm["zeroed"][g].mean())
            if c.nprob > 1:
                assert any(not np.array_equal(lm["zeroed"][0], lm["zeroed"][g]) for g in range(1, c.nprob))
    return lm


def unpad(A, pk):
    return {k: np.ascontiguousarray(A[k, :q, :q]) for k, q in enumerate(pk)}
