// Fused joint neighbourhood selection for K ORDERED instances: time-varying neighbourhood selection (Kolar, Song,
// Ahmed, Xing 2010, TESLA) with the fused penalty of Danaher, Wang, Witten (2014) -- reg='FGL' for neighbourhood selection.
// For node j, with B = (beta^(1), ..., beta^(K)) in the instances' given order:
//
//     min_B  sum_k omega_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ]
//            + lambda1 sum_k sum_{i != j} |beta^(k)_i|  +  lambda2 sum_{i != j} sum_{k < K} |beta^(k+1)_i - beta^(k)_i|
//
// k_mb_fused_path is the body of k_mb_joint_path (mb_joint_body.hpp, FUSED = true; neighborhood_joint.hip's head says where
// things live and how a pair is walked -- all of it holds here) with another block update and another screen.
//
// Block update, majorised.  With g^(k) = omega_k (s_j^(k) - S^(k) beta^(k)) and ONE curvature a_i = max_k omega_k S^(k)_ii for
// the block of variable i:
//     v_k = beta^(k)_i + g^(k)_i / a_i,   b = soft(tv(v, lambda2 / a_i), lambda1 / a_i),   g^(k) -= omega_k (b_k - beta^(k)_i) S^(k)[i, :].
// tv is Condat's direct 1-D total-variation prox (mbf_condat; condat_inplace's arithmetic), its composition with soft the
// fused-lasso prox (Friedman, Hastie, Hoefling, Tibshirani 2007).  The block's quadratic has the diagonal Hessian
// diag(omega_k S^(k)_ii); a_i I majorises it, so the step minimises an upper bound that touches at beta: the objective never
// rises and the fixed points are the block minimisers.  Where all omega_k S^(k)_ii are equal (correlation stacks with equal
// weights) it is the exact block minimisation.  The prox of the fused penalty under a non-constant diagonal metric has no
// direct scan; that is why the step is majorised.
//
// The scan runs in every lane of every wave on the K exchanged words (v_k in lane k, read lane by lane into scalars), so what
// steers it is workgroup-uniform and no wave waits for another beyond the one barrier of the exchange.  lambda2 = 0 or
// K = 1: tv is the identity and is skipped.  Sweeps end when a_i max_k |b_k - beta_k| <= tol for every block.
//
// Screen.  A zero block stays zero exactly if soft(tv(g_i, lambda2), lambda1) = 0 (homogeneous in a_i), which is the
// feasibility of the prox's dual at 0: an interval walked along k (in the body).  The K gradients of the 64 variables of a
// slot meet in K x 64 doubles of dynamic LDS (32 KB at K = 64); the walk has K fixed trips and no branch, so it needs neither
// a divergent scan per lane nor candidates taken one by one.  Info column 2 (the Newton count of the group route) is 0.
#include "mb_joint_body.hpp"

namespace ggl {

static_assert(MBF_MAX_K <= 64 && MBF_MAX_P <= MBJ_MAX_P, "the body holds instance k in lane k and an active list of MBJ_MAX_P");

template <int NV, int IPW, bool GMEM>
__global__ __launch_bounds__(64 * MBJ_MAX_WAVES) void k_mb_fused_path(const double* __restrict__ S, int K, int p,
                                                                      const double* __restrict__ omega,
                                                                      const double* __restrict__ lam1,
                                                                      const double* __restrict__ lam2, int L, double tol,
                                                                      int max_sweeps, double* coef, double* __restrict__ resvar,
                                                                      int* __restrict__ info, double* gws)
{
    mb_joint_body<NV, IPW, GMEM, true>(S, K, p, omega, lam1, lam2, L, tol, max_sweeps, coef, resvar, info, gws);
}

// Where the gradients live: the rule of k_mb_joint_path up to p = 512.  Above, two instances per wave at 16 slots each do not
// fit beside the scan's state (the compiler reports 36 bytes of scratch), so only K <= 8 stays in registers and 8 < K <= 16
// goes to the memory-resident body as well; that variant is not instantiated (table of figures: DESIGN 31).
static bool mbf_in_registers(int K, int p) { return K <= (p <= 384 ? 64 : (p <= 512 ? 32 : 8)); }

bool mb_fused_supported(int K, int p) { return K >= 1 && p >= 1 && K <= MBF_MAX_K && p <= MBF_MAX_P; }

size_t mb_fused_workspace(int K, int p) { return mbf_in_registers(K, p) ? 0 : (size_t)K * p; }

// (the caller checked mb_fused_supported(K, p) and C * p < 2^31; gws: C * p * mb_fused_workspace(K, p) doubles)
void launch_mb_fused_path(hipStream_t st, const double* S, int K, int p, const double* omega, const double* lam1,
                          const double* lam2, int C, int L, double tol, int max_sweeps, double* coef, double* resvar, int* info,
                          double* gws)
{
    const int W = std::min(K, MBJ_MAX_WAVES);
    const size_t lds = (size_t)K * 64 * sizeof(double);                     // the screen's exchange, [k][lane]
    mbj_dispatch<false>(K, p, mbf_in_registers(K, p), [&](auto nv, auto ipw, auto gm) {
        hipLaunchKernelGGL((k_mb_fused_path<decltype(nv)::value, decltype(ipw)::value, decltype(gm)::value>),
                           dim3((unsigned)C * (unsigned)p), dim3(64 * W), lds, st, S, K, p, omega, lam1, lam2, L, tol, max_sweeps, coef,
                           resvar, info, gws);
    });
}

}  // namespace ggl
