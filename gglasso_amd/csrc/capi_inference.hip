// C ABI: the output side -- inference on a fitted precision matrix.  The debiased graphical lasso and its standard errors
// (kernels: launch_gemm_right of gemm_sym.hip, then debias.hip) as a stateless operator, host buffers in, host
// buffers out.  The tests built on T and SE (z-scores, p-values, multiplicity adjustment) are O(p^2) host work on what comes
// back anyway (gglasso_amd/utils.py).  And the batched Cholesky behind Gaussian predictive scores (cholesky.hip).
#include "capi_internal.hpp"

namespace {
constexpr int DEBIAS_FLAGS = GGL_DEBIAS_TILE32 | GGL_DEBIAS_TILE64;

// the first non-finite entry of a (K,p,p) stack, the first non-positive diagonal entry of Theta, the first bad n: found on
// the host, before anything goes up
int check_debias_inputs(int K, int p, const double* Theta, const double* S, const double* n)
{
    const size_t pp = (size_t)p * p;
    for (int k = 0; k < K; ++k)
        if (!(n[k] > 0.0) || !std::isfinite(n[k]))
            return fail(GGL_E_ARG, "bad argument: n of instance %d is %g; the number of observations must be positive and finite", k,
                        n[k]);
    const double* stacks[2] = {Theta, S};
    const char* names[2] = {"Theta", "S"};
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < K; ++k) {
            const double* a = stacks[s] + (size_t)k * pp;
            for (size_t e = 0; e < pp; ++e)
                if (!std::isfinite(a[e]))
                    return fail(GGL_E_ARG, "bad argument: %s of instance %d, variable %d: the entry (%d, %d) is not finite", names[s],
                                k, (int)(e / p), (int)(e / p), (int)(e % p));
        }
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < p; ++i) {
            const double d = Theta[(size_t)k * pp + (size_t)i * p + i];
            if (!(d > 0.0))
                return fail(GGL_E_ARG, "bad argument: Theta of instance %d, variable %d: the diagonal entry is %g; a precision matrix "
                            "has a positive diagonal", k, i, d);
        }
    return GGL_OK;
}

int debias_tile(int flags) { return (flags & GGL_DEBIAS_TILE64) ? 64 : ((flags & GGL_DEBIAS_TILE32) ? 32 : 0); }
}  // namespace

extern "C" int ggl_debias(int device, int K, int p, const double* Theta_host, const double* S_host, const double* n, int flags,
                          double* T_out, double* SE_out)
{
    ARGCHK(K >= 1 && p >= 1, "K >= 1, p >= 1");
    ARGCHK(Theta_host && S_host && n && T_out && SE_out, "Theta, S, n, T_out and SE_out must not be NULL");
    ARGCHK((flags & ~DEBIAS_FLAGS) == 0, "flags: unknown bits (GGL_DEBIAS_TILE32 | GGL_DEBIAS_TILE64)");
    ARGCHK(flags != DEBIAS_FLAGS, "flags: GGL_DEBIAS_TILE32 and GGL_DEBIAS_TILE64 exclude each other");
    RCCHK(check_debias_inputs(K, p, Theta_host, S_host, n));
    HIPCHK(hipSetDevice(device));
    const size_t np = (size_t)K * p * p;
    const std::vector<double> ones(K, 1.0);
    DevBuf dTheta, dS, dM, dT, dSE, dN, dOne;
    HIPCHK(dTheta.alloc(np));
    HIPCHK(dS.alloc(np));
    HIPCHK(dM.alloc(np));
    HIPCHK(dT.alloc(np));
    HIPCHK(dSE.alloc(np));
    HIPCHK(dN.alloc(K));
    HIPCHK(dOne.alloc(K));
    UP(dTheta.p, Theta_host, np);
    UP(dS.p, S_host, np);
    UP(dN.p, n, K);
    UP(dOne.p, ones.data(), K);
    launch_gemm_right(nullptr, dTheta.p, dS.p, dM.p, dOne.p, K, K, p, 0);
    HIPCHK(hipGetLastError());
    launch_debias(nullptr, dM.p, dTheta.p, dN.p, dT.p, dSE.p, K, p, debias_tile(flags));
    HIPCHK(hipGetLastError());
    DOWN(T_out, dT.p, np);
    DOWN(SE_out, dSE.p, np);
    return GGL_OK;
}

// Average milliseconds of `iters` launches on random device data (HIP events): ms_out[0] the full product M = A T
// (launch_gemm_right, the only route to M Theta without k_debias), ms_out[1] k_debias with its epilogues.  tile: 0, 32, 64.
extern "C" int ggl_dev_debias_bench(int K, int p, int tile, int iters, double* ms_out)
{
    ARGCHK(K >= 1 && p >= 1 && iters >= 1 && ms_out, "arguments");
    ARGCHK(tile == 0 || tile == 32 || tile == 64, "tile: 0, 32 or 64");
    const size_t np = (size_t)K * p * p;
    std::vector<double> h(np), ones(K, 1.0), nobs(K, 1000.0);
    unsigned long long s = 88172645463325252ull;
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < p; ++i)
            for (int j = i; j < p; ++j) {
                s ^= s << 13; s ^= s >> 7; s ^= s << 17;
                const double v = i == j ? 1.0 : ((double)(s >> 11) / 9007199254740992.0 - 0.5) / p;
                h[(size_t)k * p * p + (size_t)i * p + j] = h[(size_t)k * p * p + (size_t)j * p + i] = v;
            }
    DevBuf dA, dM, dT, dSE, dN, dOne;
    HIPCHK(dA.alloc(np));
    HIPCHK(dM.alloc(np));
    HIPCHK(dT.alloc(np));
    HIPCHK(dSE.alloc(np));
    HIPCHK(dN.alloc(K));
    HIPCHK(dOne.alloc(K));
    UP(dA.p, h.data(), np);
    UP(dN.p, nobs.data(), K);
    UP(dOne.p, ones.data(), K);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int route = 0; route < 2; ++route) {
        auto launch = [&] {
            if (route == 0) launch_gemm_right(nullptr, dA.p, dA.p, dM.p, dOne.p, K, K, p, 0);
            else launch_debias(nullptr, dM.p, dA.p, dN.p, dT.p, dSE.p, K, p, tile);
        };
        for (int i = 0; i < 3; ++i) launch();
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) launch();
        HIPCHK(hipEventRecord(e1, nullptr));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        ms_out[route] = ms / iters;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    return GGL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched Cholesky with the outputs of a Gaussian predictive score (cholesky.hip) as a stateless operator.  The
// bandwidth search itself (ggl_weighted_predictive_scores) stands beside the weighted covariance in capi_data.hip.
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int ggl_cholesky_predict(int device, int K, int p, const double* S_host, const double* d_host, double ridge,
                                    double* out)
{
    ARGCHK(K >= 1 && p >= 1, "K >= 1, p >= 1");
    ARGCHK(S_host && out, "S and out must not be NULL");
    ARGCHK(ridge >= 0.0 && std::isfinite(ridge), "ridge must be non-negative and finite");
    HIPCHK(hipSetDevice(device));
    const size_t np = (size_t)K * p * p;
    DevBuf dS, dD, dOut;
    HIPCHK(dS.alloc(np));
    HIPCHK(dOut.alloc((size_t)K * 4));
    UP(dS.p, S_host, np);
    if (d_host) {
        HIPCHK(dD.alloc((size_t)K * p));
        UP(dD.p, d_host, (size_t)K * p);
    }
    launch_chol_predict(nullptr, dS.p, d_host ? dD.p : nullptr, ridge, dOut.p, K, p);
    HIPCHK(hipGetLastError());
    DOWN(out, dOut.p, (size_t)K * 4);
    return GGL_OK;
}

// K copies of one random SPD matrix (unit diagonal plus p, off-diagonal entries in (-0.5, 0.5): diagonally dominant) with a
// right-hand side; every timed launch is preceded by the device copy that restores the stack the kernel overwrites, and
// ms_out[2] is that copy alone
extern "C" int ggl_dev_chol_bench(int K, int p, int iters, double* ms_out)
{
    ARGCHK(K >= 1 && p >= 1 && iters >= 1 && ms_out, "arguments");
    const size_t pp = (size_t)p * p, np = (size_t)K * pp;
    std::vector<double> h(pp), hd(p);
    unsigned long long s = 88172645463325252ull;
    for (int i = 0; i < p; ++i) {
        for (int j = i; j < p; ++j) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            const double v = i == j ? 1.0 + p : (double)(s >> 11) / 9007199254740992.0 - 0.5;
            h[(size_t)i * p + j] = h[(size_t)j * p + i] = v;
        }
        hd[i] = (double)((s >> 20) & 1023) / 1024.0 - 0.5;
    }
    DevBuf dS0, dD0, dS, dD, dOut;
    HIPCHK(dS0.alloc(np));
    HIPCHK(dD0.alloc((size_t)K * p));
    HIPCHK(dS.alloc(np));
    HIPCHK(dD.alloc((size_t)K * p));
    HIPCHK(dOut.alloc((size_t)K * 4));
    for (int k = 0; k < K; ++k) {
        UP(dS0.p + (size_t)k * pp, h.data(), pp);
        UP(dD0.p + (size_t)k * p, hd.data(), p);
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int route = 0; route < 3; ++route) {
        auto launch = [&]() -> hipError_t {
            hipError_t e = hipMemcpyAsync(dS.p, dS0.p, np * sizeof(double), hipMemcpyDeviceToDevice, nullptr);
            if (e != hipSuccess) return e;
            e = hipMemcpyAsync(dD.p, dD0.p, (size_t)K * p * sizeof(double), hipMemcpyDeviceToDevice, nullptr);
            if (e != hipSuccess) return e;
            if (route < 2) launch_chol_predict(nullptr, dS.p, dD.p, 0.0, dOut.p, K, p, route == 0);
            return hipSuccess;
        };
        for (int i = 0; i < 3; ++i) HIPCHK(launch());
        HIPCHK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i) HIPCHK(launch());
        HIPCHK(hipEventRecord(e1, nullptr));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        ms_out[route] = ms / iters;
    }
    ms_out[0] -= ms_out[2];
    ms_out[1] -= ms_out[2];
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    return GGL_OK;
}
