// C ABI: Meinshausen-Buhlmann neighbourhood selection (kernels: neighborhood.hip).  ggl_neighborhood_path is the
// stateless operator, host buffers in and out; ggl_neighborhood_stability runs the same path on the B matrices a ctx holds
// (the StARS route: ggl_set_S_from_subsets and its siblings wrote them), keeps the symmetrised (L,B,p,p) stack on the device
// and reduces it with the kernel behind ggl_edge_stability.  ggl_neighborhood_refit and ggl_neighborhood_cv (below) refit a
// graph by least squares and score the regressions on held-out data (kernels: mb_refit.hip).  Each of path,
// stability and cv has ONE host function (mb_*_host); the plain entry and its _w sibling both forward into it.
#include "capi_internal.hpp"

namespace {
// what both entry points refuse about the grid and the solver's parameters
int check_mb_args(int L, const double* lam, int rule, int rule_min, double tol, int max_sweeps, int p)
{
    ARGCHK(L >= 1 && p >= 1, "L >= 1, p >= 1");
    if (p > MB_MAX_P) return fail(GGL_E_ARG, "bad argument: p = %d, k_mb_path serves p <= %d", p, MB_MAX_P);
    ARGCHK(lam, "lam must not be NULL");
    for (int l = 0; l < L; ++l) {
        if (!(lam[l] > 0.0) || !std::isfinite(lam[l]))
            return fail(GGL_E_ARG, "bad argument: lam[%d] = %g; a penalty must be positive and finite", l, lam[l]);
        if (l > 0 && !(lam[l] < lam[l - 1]))
            return fail(GGL_E_ARG, "bad argument: lam[%d] = %g does not lie below lam[%d] = %g; the grid must be strictly "
                        "descending", l, lam[l], l - 1, lam[l - 1]);
    }
    if (rule < rule_min || rule > GGL_MB_OR)
        return fail(GGL_E_ARG, "bad argument: rule = %d (%sGGL_MB_AND 1, GGL_MB_OR 2)", rule, rule_min == 0 ? "GGL_MB_RAW 0, " : "");
    ARGCHK(tol >= 0.0 && std::isfinite(tol), "tol must be non-negative and finite");
    ARGCHK(max_sweeps >= 1, "max_sweeps >= 1");
    return GGL_OK;
}

struct IntBuf {
    int* p = nullptr;
    ~IntBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(int)); }
};

// the (p,p) matrices first .. n - 1 of S on the host: every entry finite, every diagonal entry positive; what: "matrix" /
// "instance"
int check_S_host(const double* S, int n, int p, const char* what, int first = 0)
{
    const size_t pp = (size_t)p * p;
    for (int m = first; m < n; ++m) {
        const double* a = S + (size_t)m * pp;
        for (size_t e = 0; e < pp; ++e)
            if (!std::isfinite(a[e]))
                return fail(GGL_E_ARG, "bad argument: S of %s %d: the entry (%d, %d) is not finite", what, m, (int)(e / p), (int)(e % p));
        for (int i = 0; i < p; ++i)
            if (!(a[(size_t)i * p + i] > 0.0))
                return fail(GGL_E_ARG, "bad argument: S of %s %d, variable %d: the diagonal entry is %g; it must be positive", what, m,
                            i, a[(size_t)i * p + i]);
    }
    return GGL_OK;
}

int check_threshold(double t)
{
    if (!(t >= 0.0) || !(t <= 1.79769313486231570815e308))
        return fail(GGL_E_ARG, "bad argument: the edge threshold t = %g must be finite and not negative", t);
    return GGL_OK;
}

// Penalty weights and the scaled lasso: the adaptive lasso of Zou (2006, JASA 101), the scaled lasso of Sun &
// Zhang (2012, Biometrika 99; 2013, JMLR 14) / the square-root lasso of Belloni, Chernozhukov, Wang (2011, Biometrika 98), the
// estimator behind TIGER (Liu & Wang 2017, EJS 11).  A _w entry is its sibling plus (weights, weights_per_matrix, mode,
// sig_tol, max_outer) and a third int of info per node; the sibling is the same host path with (no weights, GGL_MB_LASSO).
int check_mbw_args(const double* weights, int weights_per_matrix, int M, int p, int mode, double sig_tol, int max_outer)
{
    if (mode != GGL_MB_LASSO && mode != GGL_MB_SCALED)
        return fail(GGL_E_ARG, "bad argument: mode = %d (GGL_MB_LASSO 0, GGL_MB_SCALED 1)", mode);
    if (!(sig_tol >= 0.0) || !std::isfinite(sig_tol))
        return fail(GGL_E_ARG, "bad argument: sig_tol = %g must be non-negative and finite", sig_tol);
    if (max_outer < 1) return fail(GGL_E_ARG, "bad argument: max_outer = %d; max_outer >= 1", max_outer);
    if (weights) {
        const size_t pp = (size_t)p * p;
        const int nW = weights_per_matrix ? M : 1;
        for (int m = 0; m < nW; ++m)
            for (size_t e = 0; e < pp; ++e) {
                const double v = weights[(size_t)m * pp + e];
                if (!(v >= 0.0))                                            // +inf is legal: the coordinate is excluded
                    return fail(GGL_E_ARG, "bad argument: weights of matrix %d: the entry (%d, %d) is %g; a penalty weight must "
                                "lie in [0, +inf]", m, (int)(e / p), (int)(e % p), v);
            }
    }
    return GGL_OK;
}

int mb_path_host(int device, int M, int p, const double* S_host, int L, const double* lam, int rule, double tol, int max_sweeps,
                 const double* weights, int weights_per_matrix, int mode, double sig_tol, int max_outer, int ninfo,
                 double* coef_out, double* resvar_out, int* info_out)
{
    ARGCHK(M >= 1, "M >= 1");
    RCCHK(check_mb_args(L, lam, rule, GGL_MB_RAW, tol, max_sweeps, p));
    ARGCHK(S_host && coef_out && info_out, "S, coef_out and info_out must not be NULL");
    ARGCHK((double)M * p < 2147483647.0, "M * p must stay below 2^31");
    RCCHK(check_mbw_args(weights, weights_per_matrix, M, p, mode, sig_tol, max_outer));
    RCCHK(check_S_host(S_host, M, p, "matrix"));
    HIPCHK(hipSetDevice(device));
    const size_t pp = (size_t)p * p, nML = (size_t)M * L, nW = weights ? (weights_per_matrix ? (size_t)M : 1) * pp : 0;
    DevBuf dS, dLam, dCoef, dRes, dW;
    IntBuf dInfo;
    HIPCHK(dS.alloc((size_t)M * pp));
    HIPCHK(dLam.alloc(L));
    HIPCHK(dCoef.alloc(nML * pp));
    if (resvar_out) HIPCHK(dRes.alloc(nML * p));
    if (weights) HIPCHK(dW.alloc(nW));                                  // a plain call has no table
    HIPCHK(dInfo.alloc(nML * p * ninfo));
    UP(dS.p, S_host, (size_t)M * pp);
    UP(dLam.p, lam, L);
    if (weights) UP(dW.p, weights, nW);
    HIPCHK(launch_mb_path(nullptr, dS.p, M, p, dW.p, weights_per_matrix ? pp : 0, dLam.p, L, mode, tol, max_sweeps, sig_tol,
                          max_outer, dCoef.p, dRes.p, dInfo.p, ninfo, (size_t)L, 1));
    launch_mb_symmetrize(nullptr, dCoef.p, nML, p, rule);
    HIPCHK(hipGetLastError());
    DOWN(coef_out, dCoef.p, nML * pp);
    if (resvar_out) DOWN(resvar_out, dRes.p, nML * p);
    HIPCHK(hipMemcpy(info_out, dInfo.p, nML * p * ninfo * sizeof(int), hipMemcpyDeviceToHost));
    return GGL_OK;
}

int mb_stability_host(ggl_ctx* c, int L, const double* lam, int rule, double tol, int max_sweeps, double t,
                      const double* weights, int weights_per_matrix, int mode, double sig_tol, int max_outer, int ninfo,
                      long long* num_out, int* counts_out, double* stack_out, int* info_out)
{
    ARGCHK(c && num_out && info_out, "ctx, num_out and info_out must not be NULL");
    ARGCHK(!c->has_dims, "a ctx with instance dimensions (ggl_set_instance_dims) holds no stack of one dimension");
    RCCHK(check_mb_args(L, lam, rule, GGL_MB_AND, tol, max_sweeps, c->p));
    RCCHK(check_threshold(t));
    const int B = c->K, p = c->p;
    ARGCHK(L <= 65535, "more than 65535 lambdas in one call");
    ARGCHK((double)B * p < 2147483647.0, "K * p must stay below 2^31");
    ARGCHK((double)p * (double)p * (double)B * (double)B < 7e19, "p * B too large for exact 64-bit sums");
    RCCHK(check_mbw_args(weights, weights_per_matrix, B, p, mode, sig_tol, max_outer));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    const size_t pp = (size_t)p * p, nLB = (size_t)L * B, nW = weights ? (weights_per_matrix ? (size_t)B : 1) * pp : 0;
    DevBuf dLam, dStack, dNum, dW;
    IntBuf dInfo, dCnt;
    HIPCHK(dLam.alloc(L));
    HIPCHK(dStack.alloc(nLB * pp));
    HIPCHK(dNum.alloc(L));
    if (weights) HIPCHK(dW.alloc(nW));                                  // a plain call has no table
    HIPCHK(dInfo.alloc(nLB * p * ninfo));
    if (counts_out) HIPCHK(dCnt.alloc((size_t)L * pp));
    hipStream_t st = c->stream;
    unsigned long long* num = reinterpret_cast<unsigned long long*>(dNum.p);
    HIPCHK(hipMemcpyAsync(dLam.p, lam, L * sizeof(double), hipMemcpyHostToDevice, st));
    if (weights) HIPCHK(hipMemcpyAsync(dW.p, weights, nW * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(num, 0, L * sizeof(unsigned long long), st));
    // slot (subsample r, lambda l) of the stack is l * B + r: the layout k_edge_stability reads
    HIPCHK(launch_mb_path(st, c->S, B, p, dW.p, weights_per_matrix ? pp : 0, dLam.p, L, mode, tol, max_sweeps, sig_tol, max_outer,
                          dStack.p, nullptr, dInfo.p, ninfo, 1, (size_t)B));
    launch_mb_symmetrize(st, dStack.p, nLB, p, rule);
    HIPCHK(hipGetLastError());
    launch_edge_stability(st, dStack.p, L, B, p, t, dCnt.p, num);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(num_out, num, L * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(info_out, dInfo.p, nLB * p * ninfo * sizeof(int), hipMemcpyDeviceToHost, st));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, dCnt.p, (size_t)L * pp * sizeof(int), hipMemcpyDeviceToHost, st));
    if (stack_out) HIPCHK(hipMemcpyAsync(stack_out, dStack.p, nLB * pp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}
}  // namespace

extern "C" int ggl_neighborhood_path(int device, int M, int p, const double* S_host, int L, const double* lam, int rule,
                                     double tol, int max_sweeps, double* coef_out, double* resvar_out, int* info_out)
{
    return mb_path_host(device, M, p, S_host, L, lam, rule, tol, max_sweeps, nullptr, 0, GGL_MB_LASSO, 0.0, 1, 2, coef_out,
                        resvar_out, info_out);
}

extern "C" int ggl_neighborhood_path_w(int device, int M, int p, const double* S_host, int L, const double* lam, int rule,
                                       double tol, int max_sweeps, const double* weights, int weights_per_matrix, int mode,
                                       double sig_tol, int max_outer, double* coef_out, double* resvar_out, int* info_out)
{
    return mb_path_host(device, M, p, S_host, L, lam, rule, tol, max_sweeps, weights, weights_per_matrix, mode, sig_tol, max_outer, 3,
                        coef_out, resvar_out, info_out);
}

extern "C" int ggl_neighborhood_stability(ggl_ctx* c, int L, const double* lam, int rule, double tol, int max_sweeps, double t,
                                          long long* num_out, int* counts_out, double* stack_out, int* info_out)
{
    return mb_stability_host(c, L, lam, rule, tol, max_sweeps, t, nullptr, 0, GGL_MB_LASSO, 0.0, 1, 2, num_out, counts_out,
                             stack_out, info_out);
}

extern "C" int ggl_neighborhood_stability_w(ggl_ctx* c, int L, const double* lam, int rule, double tol, int max_sweeps, double t,
                                            const double* weights, int weights_per_matrix, int mode, double sig_tol,
                                            int max_outer, long long* num_out, int* counts_out, double* stack_out, int* info_out)
{
    return mb_stability_host(c, L, lam, rule, tol, max_sweeps, t, weights, weights_per_matrix, mode, sig_tol, max_outer, 3, num_out,
                             counts_out, stack_out, info_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// Refit on the graph (kernels: mb_refit.hip): the relaxed lasso of Meinshausen (2007), the regression-based
// precision estimator of Yuan (2010, JMLR 11) and Zhou, Ruetimann, Xu, Buehlmann (2011, JMLR 12)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// The refit of nslot slots on stream st: dCoef zeroed, every unit through the wave kernel, info read back once, the pending
// units (32 < degree <= MBR_MAX_DEG) listed and served a workgroup each, then the transpose that puts beta^(j) into column j.
// info_host (nslot,p,2) holds the final info on return; the stream has been waited for.
int run_refit(hipStream_t st, const double* dS, const double* dT, const double* dW, double t, int p, size_t nslot, int sdiv,
              int smod, double* dCoef, double* dRes, double* dHeld, int* dInfo, int* info_host)
{
    const size_t pp = (size_t)p * p, nunit = nslot * p;
    HIPCHK(hipMemsetAsync(dCoef, 0, nslot * pp * sizeof(double), st));
    launch_mb_refit(st, dS, dT, dW, t, p, nslot, sdiv, smod, dCoef, dRes, dHeld, dInfo);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(info_host, dInfo, nunit * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<int> list;
    for (size_t u = 0; u < nunit; ++u)
        if (info_host[2 * u + 1] == -1) list.push_back((int)u);
    IntBuf dList;
    if (!list.empty()) {
        HIPCHK(dList.alloc(list.size()));
        HIPCHK(hipMemcpyAsync(dList.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
        launch_mb_refit_listed(st, dS, dT, dW, t, p, dList.p, (int)list.size(), sdiv, smod, dCoef, dRes, dHeld, dInfo);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(info_host, dInfo, nunit * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    launch_mb_symmetrize(st, dCoef, nslot, p, GGL_MB_RAW);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}
}  // namespace

extern "C" void ggl_mb_refit_limits(int out[2])
{
    if (!out) return;
    out[0] = MBR_MAX_DEG;
    out[1] = MB_MAX_P;
}

extern "C" int ggl_neighborhood_refit(int device, int M, int p, const double* S_host, int G, const double* W_host, double t,
                                      const double* T_host, double* coef_out, double* resvar_out, double* heldout_out,
                                      int* info_out)
{
    if (M < 1 || G < 1 || p < 1) return fail(GGL_E_ARG, "bad argument: M = %d, G = %d, p = %d; each must be at least 1", M, G, p);
    if (p > MB_MAX_P) return fail(GGL_E_ARG, "bad argument: p = %d, k_mb_refit serves p <= %d", p, MB_MAX_P);
    ARGCHK(S_host, "S must not be NULL");
    ARGCHK(W_host, "W must not be NULL");
    ARGCHK(coef_out, "coef_out must not be NULL");
    ARGCHK(resvar_out, "resvar_out must not be NULL");
    ARGCHK(info_out, "info_out must not be NULL");
    ARGCHK(!heldout_out || T_host, "heldout_out needs the second stack T");
    RCCHK(check_threshold(t));
    ARGCHK((double)M * G * p < 2147483647.0, "M * G * p must stay below 2^31");
    RCCHK(check_S_host(S_host, M, p, "matrix"));
    HIPCHK(hipSetDevice(device));
    const size_t pp = (size_t)p * p, nslot = (size_t)M * G;
    const bool held = heldout_out != nullptr;
    DevBuf dS, dT, dW, dCoef, dRes, dHeld;
    IntBuf dInfo;
    HIPCHK(dS.alloc((size_t)M * pp));
    if (held) HIPCHK(dT.alloc((size_t)M * pp));
    HIPCHK(dW.alloc(nslot * pp));
    HIPCHK(dCoef.alloc(nslot * pp));
    HIPCHK(dRes.alloc(nslot * p));
    if (held) HIPCHK(dHeld.alloc(nslot * p));
    HIPCHK(dInfo.alloc(nslot * p * 2));
    UP(dS.p, S_host, (size_t)M * pp);
    if (held) UP(dT.p, T_host, (size_t)M * pp);
    UP(dW.p, W_host, nslot * pp);
    std::vector<int> info(nslot * p * 2);
    RCCHK(run_refit(nullptr, dS.p, dT.p, dW.p, t, p, nslot, G, M, dCoef.p, dRes.p, dHeld.p, dInfo.p, info.data()));
    DOWN(coef_out, dCoef.p, nslot * pp);
    DOWN(resvar_out, dRes.p, nslot * p);
    if (held) DOWN(heldout_out, dHeld.p, nslot * p);
    std::memcpy(info_out, info.data(), info.size() * sizeof(int));
    return GGL_OK;
}

namespace {
int mb_cv_host(ggl_ctx* c, const double* X_host, int N, int F, int m, const int* idx_test, int flags, int L, const double* lam,
               int rule, double tol, int max_sweeps, double t, int refit, const double* weights, int weights_per_matrix, int mode,
               double sig_tol, int max_outer, int ninfo, double* resvar_out, double* heldout_out, int* info_out, double* stack_out)
{
    ARGCHK(c && resvar_out && heldout_out && info_out, "ctx, resvar_out, heldout_out and info_out must not be NULL");
    ARGCHK(!c->has_dims, "a ctx with instance dimensions (ggl_set_instance_dims) holds no stack of one dimension");
    RCCHK(check_mb_args(L, lam, rule, GGL_MB_AND, tol, max_sweeps, c->p));
    RCCHK(check_threshold(t));
    RCCHK(heldout_fold_check(c, X_host, N, F, m, idx_test, flags));
    if (c->K != F)
        return fail(GGL_E_ARG, "bad argument: the ctx holds K = %d matrices, the cross-validation has F = %d folds; instance f must "
                    "be the train matrix of fold f", c->K, F);
    const int p = c->p;
    ARGCHK(L <= 65535, "more than 65535 lambdas in one call");
    ARGCHK((double)L * F * p < 2147483647.0, "L * F * p must stay below 2^31");
    RCCHK(check_mbw_args(weights, weights_per_matrix, F, p, mode, sig_tol, max_outer));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    const size_t pp = (size_t)p * p, nLF = (size_t)L * F, nW = weights ? (weights_per_matrix ? (size_t)F : 1) * pp : 0;
    DevBuf dLam, dStack, dCoef, dRes, dHeld, dT, dVar, dW;
    IntBuf dInfo;
    HIPCHK(dLam.alloc(L));
    HIPCHK(dStack.alloc(nLF * pp));
    if (refit) HIPCHK(dCoef.alloc(nLF * pp));
    HIPCHK(dRes.alloc(nLF * p));
    HIPCHK(dHeld.alloc(nLF * p));
    HIPCHK(dT.alloc((size_t)F * pp));
    HIPCHK(dVar.alloc((size_t)F * p));
    if (weights) HIPCHK(dW.alloc(nW));                                  // a plain call has no table
    HIPCHK(dInfo.alloc(nLF * p * ninfo));
    hipStream_t st = c->stream;
    RCCHK(heldout_fold_covariances(c, X_host, N, F, m, idx_test, flags, dT.p, dVar.p));
    HIPCHK(hipMemcpyAsync(dLam.p, lam, L * sizeof(double), hipMemcpyHostToDevice, st));
    if (weights) HIPCHK(hipMemcpyAsync(dW.p, weights, nW * sizeof(double), hipMemcpyHostToDevice, st));
    // slot (fold f, lambda l) is l * F + f, as in ggl_neighborhood_stability; its matrices are S[f], T[f]
    HIPCHK(launch_mb_path(st, c->S, F, p, dW.p, weights_per_matrix ? pp : 0, dLam.p, L, mode, tol, max_sweeps, sig_tol, max_outer,
                          dStack.p, refit ? nullptr : dRes.p, dInfo.p, ninfo, 1, (size_t)F));
    if (!refit) {
        launch_mb_heldout(st, dT.p, dStack.p, p, nLF, 1, F, dHeld.p);       // the lasso's own beta, still in rows
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(info_out, dInfo.p, nLF * p * ninfo * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    launch_mb_symmetrize(st, dStack.p, nLF, p, rule);
    HIPCHK(hipGetLastError());
    // (the refit's info is 2 ints per node whatever ninfo: dInfo is large enough for either)
    if (refit) RCCHK(run_refit(st, c->S, dT.p, dStack.p, t, p, nLF, 1, F, dCoef.p, dRes.p, dHeld.p, dInfo.p, info_out));
    HIPCHK(hipMemcpyAsync(resvar_out, dRes.p, nLF * p * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(heldout_out, dHeld.p, nLF * p * sizeof(double), hipMemcpyDeviceToHost, st));
    if (stack_out) HIPCHK(hipMemcpyAsync(stack_out, dStack.p, nLF * pp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}
}  // namespace

extern "C" int ggl_neighborhood_cv(ggl_ctx* c, const double* X_host, int N, int F, int m, const int* idx_test, int flags, int L,
                                   const double* lam, int rule, double tol, int max_sweeps, double t, int refit,
                                   double* resvar_out, double* heldout_out, int* info_out, double* stack_out)
{
    return mb_cv_host(c, X_host, N, F, m, idx_test, flags, L, lam, rule, tol, max_sweeps, t, refit, nullptr, 0, GGL_MB_LASSO, 0.0, 1,
                      2, resvar_out, heldout_out, info_out, stack_out);
}

extern "C" int ggl_neighborhood_cv_w(ggl_ctx* c, const double* X_host, int N, int F, int m, const int* idx_test, int flags, int L,
                                     const double* lam, int rule, double tol, int max_sweeps, double t, int refit,
                                     const double* weights, int weights_per_matrix, int mode, double sig_tol, int max_outer,
                                     double* resvar_out, double* heldout_out, int* info_out, double* stack_out)
{
    return mb_cv_host(c, X_host, N, F, m, idx_test, flags, L, lam, rule, tol, max_sweeps, t, refit, weights, weights_per_matrix, mode,
                      sig_tol, max_outer, 3, resvar_out, heldout_out, info_out, stack_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// Joint neighbourhood selection of K instances under the GGL penalty (kernel: neighborhood_joint.hip): the group
// lasso across the instances of Chiquet, Grandvalet, Ambroise (2011) with the penalty of Danaher, Wang, Witten (2014), the
// sparse-group block update of Simon, Friedman, Hastie, Tibshirani (2013).  Everything behind the path -- the rule per
// instance, the refit on the symmetrised stack -- is the code of the entries above.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t MBJ_CHUNK_BYTES = (size_t)2 << 30;   // the coefficient stacks of a chunk of chains take at most this
std::atomic<long long> mbj_chunk_bytes{0};            // ggl_mb_joint_chunk_budget: 0 = MBJ_CHUNK_BYTES

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// what ggl_neighborhood_joint_path and ggl_neighborhood_joint_last share; last_only: coef_out and refit_coef_out are (C,K,p,p)
// and receive the LAST pair of every chain
int joint_path_impl(int device, int K, int p, const double* S_host, const double* omega, int C, int L, const double* lam1,
                    const double* lam2, int rule, double tol, int max_sweeps, int refit, double t, double* coef_out,
                    double* resvar_out, int* info_out, double* refit_coef_out, double* refit_resvar_out, int* refit_info_out,
                    bool last_only, bool fused);
}  // namespace

extern "C" void ggl_mb_joint_limits(int out[2])
{
    if (!out) return;
    out[0] = MBJ_MAX_K;
    out[1] = MBJ_MAX_P;
}

extern "C" void ggl_mb_joint_chunk_budget(long long bytes) { mbj_chunk_bytes.store(bytes > 0 ? bytes : 0); }

extern "C" int ggl_neighborhood_joint_path(int device, int K, int p, const double* S_host, const double* omega, int C, int L,
                                           const double* lam1, const double* lam2, int rule, double tol, int max_sweeps, int refit,
                                           double t, double* coef_out, double* resvar_out, int* info_out, double* refit_coef_out,
                                           double* refit_resvar_out, int* refit_info_out)
{
    return joint_path_impl(device, K, p, S_host, omega, C, L, lam1, lam2, rule, tol, max_sweeps, refit, t, coef_out, resvar_out,
                           info_out, refit_coef_out, refit_resvar_out, refit_info_out, false, false);
}

extern "C" int ggl_neighborhood_joint_last(int device, int K, int p, const double* S_host, const double* omega, int C, int L,
                                           const double* lam1, const double* lam2, int rule, double tol, int max_sweeps, int refit,
                                           double t, double* coef_out, double* resvar_out, int* info_out, double* refit_coef_out,
                                           double* refit_resvar_out, int* refit_info_out)
{
    return joint_path_impl(device, K, p, S_host, omega, C, L, lam1, lam2, rule, tol, max_sweeps, refit, t, coef_out, resvar_out,
                           info_out, refit_coef_out, refit_resvar_out, refit_info_out, true, false);
}

// The path kernel alone, timed by HIP events on the device for tools/bench_neighborhood_joint.py (the convention of
// ggl_dev_chol_bench) and, with fused, k_mb_fused_path for tools/bench_neighborhood_fused.py: all C chains in one launch,
// iters launches behind one warm-up, ms_out[iters].  S_host is not checked.
static int mb_joint_bench_impl(int K, int p, const double* S_host, int C, int L, const double* lam1, const double* lam2, double tol,
                               int max_sweeps, int iters, double* ms_out, bool fused)
{
    ARGCHK(C >= 1 && L >= 1 && iters >= 1 && S_host && lam1 && lam2 && ms_out, "C, L, iters >= 1 and no NULL buffer");
    ARGCHK(fused ? mb_fused_supported(K, p) : mb_joint_supported(K, p), "K, p outside ggl_mb_joint_limits / ggl_mb_fused_limits");
    ARGCHK((double)C * L * K * p < 2147483647.0, "C * L * K * p must stay below 2^31");
    const size_t pp = (size_t)p * p, nCL = (size_t)C * L;
    DevBuf dS, dL1, dL2, dCoef, dG;
    IntBuf dInfo;
    HIPCHK(dS.alloc((size_t)K * pp));
    HIPCHK(dL1.alloc(nCL));
    HIPCHK(dL2.alloc(nCL));
    HIPCHK(dCoef.alloc(nCL * K * pp));
    HIPCHK(dInfo.alloc(nCL * p * 3));
    HIPCHK(dG.alloc((size_t)C * p * (fused ? mb_fused_workspace(K, p) : mb_joint_workspace(K, p))));
    UP(dS.p, S_host, (size_t)K * pp);
    UP(dL1.p, lam1, nCL);
    UP(dL2.p, lam2, nCL);
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    for (int it = -1; it < iters; ++it) {
        HIPCHK(hipEventRecord(ev.a, nullptr));
        (fused ? launch_mb_fused_path : launch_mb_joint_path)(nullptr, dS.p, K, p, nullptr, dL1.p, dL2.p, C, L, tol, max_sweeps,
                                                              dCoef.p, nullptr, dInfo.p, dG.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev.b, nullptr));
        HIPCHK(hipEventSynchronize(ev.b));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
        if (it >= 0) ms_out[it] = ms;
    }
    return GGL_OK;
}

extern "C" int ggl_dev_mb_joint_bench(int K, int p, const double* S_host, int C, int L, const double* lam1, const double* lam2,
                                      double tol, int max_sweeps, int iters, double* ms_out)
{
    return mb_joint_bench_impl(K, p, S_host, C, L, lam1, lam2, tol, max_sweeps, iters, ms_out, false);
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused joint neighbourhood selection of K ordered instances (kernel: neighborhood_fused.hip): lam2 weighs the
// differences between consecutive instances.  The host work is that of the joint route, refusals and chunking included;
// lam2 > 0 with K = 1 is accepted and inert.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" void ggl_mb_fused_limits(int out[2])
{
    if (!out) return;
    out[0] = MBF_MAX_K;
    out[1] = MBF_MAX_P;
}

extern "C" int ggl_neighborhood_fused_path(int device, int K, int p, const double* S_host, const double* omega, int C, int L,
                                           const double* lam1, const double* lam2, int rule, double tol, int max_sweeps, int refit,
                                           double t, double* coef_out, double* resvar_out, int* info_out, double* refit_coef_out,
                                           double* refit_resvar_out, int* refit_info_out)
{
    return joint_path_impl(device, K, p, S_host, omega, C, L, lam1, lam2, rule, tol, max_sweeps, refit, t, coef_out, resvar_out,
                           info_out, refit_coef_out, refit_resvar_out, refit_info_out, false, true);
}

extern "C" int ggl_neighborhood_fused_last(int device, int K, int p, const double* S_host, const double* omega, int C, int L,
                                           const double* lam1, const double* lam2, int rule, double tol, int max_sweeps, int refit,
                                           double t, double* coef_out, double* resvar_out, int* info_out, double* refit_coef_out,
                                           double* refit_resvar_out, int* refit_info_out)
{
    return joint_path_impl(device, K, p, S_host, omega, C, L, lam1, lam2, rule, tol, max_sweeps, refit, t, coef_out, resvar_out,
                           info_out, refit_coef_out, refit_resvar_out, refit_info_out, true, true);
}

extern "C" int ggl_dev_mb_fused_bench(int K, int p, const double* S_host, int C, int L, const double* lam1, const double* lam2,
                                      double tol, int max_sweeps, int iters, double* ms_out)
{
    return mb_joint_bench_impl(K, p, S_host, C, L, lam1, lam2, tol, max_sweeps, iters, ms_out, true);
}

namespace {
int joint_path_impl(int device, int K, int p, const double* S_host, const double* omega, int C, int L, const double* lam1,
                    const double* lam2, int rule, double tol, int max_sweeps, int refit, double t, double* coef_out,
                    double* resvar_out, int* info_out, double* refit_coef_out, double* refit_resvar_out, int* refit_info_out,
                    bool last_only, bool fused)
{
    const char* kernel = fused ? "k_mb_fused_path" : "k_mb_joint_path";
    const int maxK = fused ? MBF_MAX_K : MBJ_MAX_K, maxP = fused ? MBF_MAX_P : MBJ_MAX_P;
    if (K < 1 || p < 1 || C < 1 || L < 1)
        return fail(GGL_E_ARG, "bad argument: K = %d, p = %d, C = %d, L = %d; each must be at least 1", K, p, C, L);
    if (K > maxK) return fail(GGL_E_ARG, "bad argument: K = %d, %s serves K <= %d", K, kernel, maxK);
    if (p > maxP) return fail(GGL_E_ARG, "bad argument: p = %d, %s serves p <= %d", p, kernel, maxP);
    ARGCHK(S_host, "S must not be NULL");
    ARGCHK(lam1 && lam2, "lam1 and lam2 must not be NULL");
    ARGCHK(info_out, "info_out must not be NULL");
    for (int c = 0; c < C; ++c)
        for (int l = 0; l < L; ++l) {
            const double a = lam1[(size_t)c * L + l], b = lam2[(size_t)c * L + l];
            if (!(a >= 0.0) || !std::isfinite(a))
                return fail(GGL_E_ARG, "bad argument: lam1 of (chain %d, index %d) = %g; a penalty must be non-negative and finite", c, l, a);
            if (!(b >= 0.0) || !std::isfinite(b))
                return fail(GGL_E_ARG, "bad argument: lam2 of (chain %d, index %d) = %g; a penalty must be non-negative and finite", c, l, b);
            if (!(a + b > 0.0))
                return fail(GGL_E_ARG, "bad argument: lam1 + lam2 of (chain %d, index %d) = %g; one of the two must be positive", c, l, a + b);
        }
    if (omega)
        for (int k = 0; k < K; ++k)
            if (!(omega[k] > 0.0) || !std::isfinite(omega[k]))
                return fail(GGL_E_ARG, "bad argument: omega[%d] = %g; an instance weight must be positive and finite", k, omega[k]);
    ARGCHK(tol >= 0.0 && std::isfinite(tol), "tol must be non-negative and finite");
    ARGCHK(max_sweeps >= 1, "max_sweeps >= 1");
    if (rule < GGL_MB_RAW || rule > GGL_MB_OR)
        return fail(GGL_E_ARG, "bad argument: rule = %d (GGL_MB_RAW 0, GGL_MB_AND 1, GGL_MB_OR 2)", rule);
    if (refit) {
        if (rule == GGL_MB_RAW)
            return fail(GGL_E_ARG, "bad argument: rule = GGL_MB_RAW with refit; the refit needs a graph (GGL_MB_AND 1, GGL_MB_OR 2)");
        RCCHK(check_threshold(t));
    }
    const size_t pp = (size_t)p * p;
    for (int k = 0; k < K; ++k) {
        const double* a = S_host + (size_t)k * pp;
        RCCHK(check_S_host(S_host, k + 1, p, "instance", k));               // instance k alone: its symmetry is tested next
        for (int i = 0; i < p; ++i)
            for (int q = i + 1; q < p; ++q)
                if (std::memcmp(&a[(size_t)i * p + q], &a[(size_t)q * p + i], sizeof(double)) != 0)
                    return fail(GGL_E_ARG, "bad argument: S of instance %d is not bitwise symmetric: the entries (%d, %d) = %.17g and "
                                "(%d, %d) = %.17g differ", k, i, q, a[(size_t)i * p + q], q, i, a[(size_t)q * p + i]);
    }
    // chunks of chains: a chain's bits do not depend on the chains beside it, so the outputs do not depend on the chunking
    const size_t gws_per_unit = fused ? mb_fused_workspace(K, p) : mb_joint_workspace(K, p);
    const size_t per_chain = ((size_t)L * K * pp * (refit ? 2 : 1) + (size_t)p * gws_per_unit) * sizeof(double);
    const long long forced = mbj_chunk_bytes.load();
    const size_t budget = forced > 0 ? (size_t)forced : MBJ_CHUNK_BYTES;
    int Cc = (int)std::min<size_t>((size_t)C, std::max<size_t>(1, budget / per_chain));
    ARGCHK((double)L * K * p < 2147483647.0, "L * K * p must stay below 2^31");
    while (Cc > 1 && (double)Cc * L * K * p >= 2147483647.0) --Cc;

    HIPCHK(hipSetDevice(device));
    const size_t nCL = (size_t)Cc * L, nslot = nCL * K;
    DevBuf dS, dOm, dL1, dL2, dCoef, dRes, dRCoef, dRRes, dG;
    IntBuf dInfo, dRInfo;
    HIPCHK(dS.alloc((size_t)K * pp));
    if (omega) HIPCHK(dOm.alloc(K));
    HIPCHK(dL1.alloc((size_t)C * L));
    HIPCHK(dL2.alloc((size_t)C * L));
    HIPCHK(dCoef.alloc(nslot * pp));
    HIPCHK(dG.alloc((size_t)Cc * p * gws_per_unit));                  // empty where the gradients fit the registers
    if (resvar_out) HIPCHK(dRes.alloc(nslot * p));
    HIPCHK(dInfo.alloc(nCL * p * 3));
    std::vector<int> rinfo;
    if (refit) {
        HIPCHK(dRCoef.alloc(nslot * pp));
        HIPCHK(dRRes.alloc(nslot * p));
        HIPCHK(dRInfo.alloc(nslot * p * 2));
        if (!refit_info_out) rinfo.resize(nslot * p * 2);
    }
    UP(dS.p, S_host, (size_t)K * pp);
    if (omega) UP(dOm.p, omega, K);
    UP(dL1.p, lam1, (size_t)C * L);
    UP(dL2.p, lam2, (size_t)C * L);
    // a (cc,L,K,p,p) device stack to the host: whole, or with last_only the last pair of every chain to (cc,K,p,p)
    auto down_stack = [&](double* host, const double* dev, int c0, int cc) -> int {
        if (!last_only) {
            DOWN(host + (size_t)c0 * L * K * pp, dev, (size_t)cc * L * K * pp);
            return GGL_OK;
        }
        for (int c = 0; c < cc; ++c)
            DOWN(host + (size_t)(c0 + c) * K * pp, dev + ((size_t)c * L + (L - 1)) * K * pp, (size_t)K * pp);
        return GGL_OK;
    };
    for (int c0 = 0; c0 < C; c0 += Cc) {
        const int cc = std::min(Cc, C - c0);
        const size_t nl = (size_t)cc * L, ns = nl * K, o = (size_t)c0 * L;
        (fused ? launch_mb_fused_path : launch_mb_joint_path)(nullptr, dS.p, K, p, omega ? dOm.p : nullptr, dL1.p + o, dL2.p + o, cc,
                                                              L, tol, max_sweeps, dCoef.p, resvar_out ? dRes.p : nullptr,
                                                              dInfo.p, dG.p);
        HIPCHK(hipGetLastError());
        launch_mb_symmetrize(nullptr, dCoef.p, ns, p, rule);
        HIPCHK(hipGetLastError());
        if (refit) {
            int* ih = refit_info_out ? refit_info_out + o * K * p * 2 : rinfo.data();
            RCCHK(run_refit(nullptr, dS.p, nullptr, dCoef.p, t, p, ns, 1, K, dRCoef.p, dRRes.p, nullptr, dRInfo.p, ih));
            if (refit_coef_out) RCCHK(down_stack(refit_coef_out, dRCoef.p, c0, cc));
            if (refit_resvar_out) DOWN(refit_resvar_out + o * K * p, dRRes.p, ns * p);
        }
        if (coef_out) RCCHK(down_stack(coef_out, dCoef.p, c0, cc));
        if (resvar_out) DOWN(resvar_out + o * K * p, dRes.p, ns * p);
        HIPCHK(hipMemcpy(info_out + o * p * 3, dInfo.p, nl * p * 3 * sizeof(int), hipMemcpyDeviceToHost));
    }
    return GGL_OK;
}
}  // namespace
