// Joint neighbourhood selection for K instances that share structure: the regression counterpart of the GGL
// penalty (Chiquet, Grandvalet, Ambroise 2011; Danaher, Wang, Witten 2014).  For node j, with B = (beta^(1), ..., beta^(K)):
//
//     min_B  sum_k omega_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ]
//            + lambda1 sum_k sum_{i != j} |beta^(k)_i|  +  lambda2 sum_{i != j} || (beta^(1)_i, ..., beta^(K)_i) ||_2
//
// k_mb_joint_path: one WORKGROUP per unit of work (chain c, node j), W = min(K, 8) waves; wave w owns the instances
// k = w, w + W, ... (at most IPW of them).  A chain is a list of L penalty pairs walked in order with warm starts.  Block
// coordinate descent on an active set of GROUPS (one block = the K coefficients of one variable i; Simon, Friedman, Hastie,
// Tibshirani 2013): with g^(k) = omega_k (s_j^(k) - S^(k) beta^(k)), a_k = omega_k S^(k)_ii, z_k = g^(k)_i + a_k beta^(k)_i,
// u = soft(z, lambda1):
//     ||u|| <= lambda2: b = 0;   lambda2 = 0: b_k = u_k / a_k;   else b_k = u_k nu / (a_k nu + lambda2),
//     nu = ||b|| the root of phi(nu) = sum_k u_k^2 / (a_k nu + lambda2)^2 - 1 -- Newton from nu_0 = (||u|| - lambda2) / max a_k,
//     where phi >= 0: the iterates increase to the root and the loop ends when a step no longer increases nu (or at the cap);
//     g^(k) -= omega_k (b_k - beta^(k)_i) S^(k)[i, :].
//
// Where things live.  g^(k) of an owned instance: NV = ceil(p / 64) doubles per lane (element i in lane i % 64, slot i / 64),
// as k_mb_path keeps its g; NV and IPW are template parameters so that every register array is indexed by constants.  Where
// K p is too large for the registers of one workgroup (GMEM) the same vectors live in a workspace in device memory with the
// same distribution, every element touched by one lane of one wave only.  beta:
// in the OUTPUT row the unit writes anyway (row j of matrix (c, l, k) of coef) -- it is touched one element per instance and
// block update, and K p doubles fit neither the registers beside g nor, at K = 32, p = 500, the LDS beside anything else.  At
// the start of a pair the row of the pair before is copied forward.  LDS: the ascending active list, the exchange of
// (z_k, a_k, beta_k) of one block update (double-buffered: one workgroup barrier per update) and the per-wave partial sums
// of the screen.
//
// A block update: every wave writes (z, a, beta) of its instances; ONE barrier; every wave solves the block redundantly with
// instance k in lane k -- the norms go through the fixed xor butterfly, so all lanes of all waves hold the same bits; each
// wave applies d_k to its own gradients.  The first owned row is requested before the barrier.  Every value that steers a loop
// (the active count, the variable, the largest change, the Newton trip count, the statuses) is computed by every wave from
// the same LDS words and is therefore workgroup-uniform: all waves reach all barriers.
//
// Per pair, the procedure of k_mb_path: screen (every inactive group with ||soft(g_i, lambda1)|| > lambda2 joins,
// the list is rebuilt ascending) -> sweeps until max_k |d_k| a_k <= tol -> all gradients recomputed from B in ascending
// order -> ONE further sweep -> screen again; finished only if that sweep moved nothing beyond tol and that screen found
// nothing.  Caps: max_sweeps per (unit, pair), MBJ_MAX_ROUNDS screens, MBJ_NEWTON_CAP Newton steps; every continuing
// comparison is false for a NaN.  A non-finite value is status 2: all K rows of the unit are NaN (diagonal 0) at this pair
// and every later one of the chain; nobody else is touched.
//
// Reproducibility: no atomic updates, fixed orders (the list ascending, a wave's instances ascending, the screen's sum over waves
// ascending, the butterfly).  A unit reads S and its own rows only: its bits do not depend on C, on the other chains or on the
// pairs that follow.
#include "mb_joint_body.hpp"

namespace ggl {

// (the body: mb_joint_body.hpp, shared with k_mb_fused_path; FUSED = false is the group penalty described above)
template <int NV, int IPW, bool GMEM>
__global__ __launch_bounds__(64 * MBJ_MAX_WAVES) void k_mb_joint_path(const double* __restrict__ S, int K, int p,
                                                                      const double* __restrict__ omega,
                                                                      const double* __restrict__ lam1,
                                                                      const double* __restrict__ lam2, int L, double tol,
                                                                      int max_sweeps, double* coef, double* __restrict__ resvar,
                                                                      int* __restrict__ info, double* gws)
{
    mb_joint_body<NV, IPW, GMEM, false>(S, K, p, omega, lam1, lam2, L, tol, max_sweeps, coef, resvar, info, gws);
}

// The g of a workgroup's K regressions lives in its registers where it fits: 8 waves of 256 registers hold 48 slots of 64
// doubles each beside everything else, and a wave needs ceil(K / 8) (rounded up to 1, 2, 4, 8) times ceil(p / 64) (4, 6, 8,
// 16) of them -- K <= 64 up to p = 384, K <= 32 up to p = 512, K <= 16 up to p = 1024.  Beyond that the same body runs with g
// in a workspace in device memory (GMEM), K p doubles per unit.
static bool mbj_in_registers(int K, int p) { return K <= (p <= 384 ? 64 : (p <= 512 ? 32 : 16)); }

bool mb_joint_supported(int K, int p) { return K >= 1 && p >= 1 && K <= MBJ_MAX_K && p <= MBJ_MAX_P; }

size_t mb_joint_workspace(int K, int p) { return mbj_in_registers(K, p) ? 0 : (size_t)K * p; }

// (the caller checked mb_joint_supported(K, p) and C * p < 2^31; gws: C * p * mb_joint_workspace(K, p) doubles)
void launch_mb_joint_path(hipStream_t st, const double* S, int K, int p, const double* omega, const double* lam1,
                          const double* lam2, int C, int L, double tol, int max_sweeps, double* coef, double* resvar, int* info,
                          double* gws)
{
    const int W = std::min(K, MBJ_MAX_WAVES);
    mbj_dispatch<true>(K, p, mbj_in_registers(K, p), [&](auto nv, auto ipw, auto gm) {
        hipLaunchKernelGGL((k_mb_joint_path<decltype(nv)::value, decltype(ipw)::value, decltype(gm)::value>),
                           dim3((unsigned)C * (unsigned)p), dim3(64 * W), 0, st, S, K, p, omega, lam1, lam2, L, tol, max_sweeps, coef,
                           resvar, info, gws);
    });
}

}  // namespace ggl
