// C ABI: Meinshausen-Buhlmann neighbourhood selection (kernels: neighborhood.hip).  ggl_neighborhood_path is the
// stateless operator, host buffers in and out; ggl_neighborhood_stability runs the same path on the B matrices a ctx holds
// (the StARS route: ggl_set_S_from_subsets and its siblings wrote them), keeps the symmetrised (L,B,p,p) stack on the device
// and reduces it with the kernel behind ggl_edge_stability.
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
}  // namespace

extern "C" int ggl_neighborhood_path(int device, int M, int p, const double* S_host, int L, const double* lam, int rule,
                                     double tol, int max_sweeps, double* coef_out, double* resvar_out, int* info_out)
{
    ARGCHK(M >= 1, "M >= 1");
    RCCHK(check_mb_args(L, lam, rule, GGL_MB_RAW, tol, max_sweeps, p));
    ARGCHK(S_host && coef_out && info_out, "S, coef_out and info_out must not be NULL");
    ARGCHK((double)M * p < 2147483647.0, "M * p must stay below 2^31");
    const size_t pp = (size_t)p * p;
    for (int m = 0; m < M; ++m) {
        const double* a = S_host + (size_t)m * pp;
        for (size_t e = 0; e < pp; ++e)
            if (!std::isfinite(a[e]))
                return fail(GGL_E_ARG, "bad argument: S of matrix %d: the entry (%d, %d) is not finite", m, (int)(e / p), (int)(e % p));
        for (int i = 0; i < p; ++i)
            if (!(a[(size_t)i * p + i] > 0.0))
                return fail(GGL_E_ARG, "bad argument: S of matrix %d, variable %d: the diagonal entry is %g; it must be positive", m,
                            i, a[(size_t)i * p + i]);
    }
    HIPCHK(hipSetDevice(device));
    const size_t nML = (size_t)M * L;
    DevBuf dS, dLam, dCoef, dRes;
    IntBuf dInfo;
    HIPCHK(dS.alloc((size_t)M * pp));
    HIPCHK(dLam.alloc(L));
    HIPCHK(dCoef.alloc(nML * pp));
    if (resvar_out) HIPCHK(dRes.alloc(nML * p));
    HIPCHK(dInfo.alloc(nML * p * 2));
    UP(dS.p, S_host, (size_t)M * pp);
    UP(dLam.p, lam, L);
    launch_mb_path(nullptr, dS.p, M, p, dLam.p, L, tol, max_sweeps, dCoef.p, dRes.p, dInfo.p, (size_t)L, 1);
    HIPCHK(hipGetLastError());
    launch_mb_symmetrize(nullptr, dCoef.p, nML, p, rule);
    HIPCHK(hipGetLastError());
    DOWN(coef_out, dCoef.p, nML * pp);
    if (resvar_out) DOWN(resvar_out, dRes.p, nML * p);
    HIPCHK(hipMemcpy(info_out, dInfo.p, nML * p * 2 * sizeof(int), hipMemcpyDeviceToHost));
    return GGL_OK;
}

extern "C" int ggl_neighborhood_stability(ggl_ctx* c, int L, const double* lam, int rule, double tol, int max_sweeps, double t,
                                          long long* num_out, int* counts_out, double* stack_out, int* info_out)
{
    ARGCHK(c && num_out && info_out, "ctx, num_out and info_out must not be NULL");
    ARGCHK(!c->has_dims, "a ctx with instance dimensions (ggl_set_instance_dims) holds no stack of one dimension");
    RCCHK(check_mb_args(L, lam, rule, GGL_MB_AND, tol, max_sweeps, c->p));
    if (!(t >= 0.0) || !(t <= 1.79769313486231570815e308))
        return fail(GGL_E_ARG, "bad argument: the edge threshold t = %g must be finite and not negative", t);
    const int B = c->K, p = c->p;
    ARGCHK(L <= 65535, "more than 65535 lambdas in one call");
    ARGCHK((double)B * p < 2147483647.0, "K * p must stay below 2^31");
    ARGCHK((double)p * (double)p * (double)B * (double)B < 7e19, "p * B too large for exact 64-bit sums");
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    const size_t pp = (size_t)p * p, nLB = (size_t)L * B;
    DevBuf dLam, dStack, dNum;
    IntBuf dInfo, dCnt;
    HIPCHK(dLam.alloc(L));
    HIPCHK(dStack.alloc(nLB * pp));
    HIPCHK(dNum.alloc(L));
    HIPCHK(dInfo.alloc(nLB * p * 2));
    if (counts_out) HIPCHK(dCnt.alloc((size_t)L * pp));
    hipStream_t st = c->stream;
    unsigned long long* num = reinterpret_cast<unsigned long long*>(dNum.p);
    HIPCHK(hipMemcpyAsync(dLam.p, lam, L * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(num, 0, L * sizeof(unsigned long long), st));
    // slot (subsample r, lambda l) of the stack is l * B + r: the layout k_edge_stability reads
    launch_mb_path(st, c->S, B, p, dLam.p, L, tol, max_sweeps, dStack.p, nullptr, dInfo.p, 1, (size_t)B);
    HIPCHK(hipGetLastError());
    launch_mb_symmetrize(st, dStack.p, nLB, p, rule);
    HIPCHK(hipGetLastError());
    launch_edge_stability(st, dStack.p, L, B, p, t, dCnt.p, num);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(num_out, num, L * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(info_out, dInfo.p, nLB * p * 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, dCnt.p, (size_t)L * pp * sizeof(int), hipMemcpyDeviceToHost, st));
    if (stack_out) HIPCHK(hipMemcpyAsync(stack_out, dStack.p, nLB * pp * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}
