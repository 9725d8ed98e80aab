// C ABI: nearest-correlation projection of an indefinite S (kernels: nearcorr.hip) -- Higham's alternating
// projections with Dykstra's correction around the L-step's (C - mu I)_+ (rank_step, capi_lstep.hip), stateless and in place on
// the S of a ctx.
#include "capi_internal.hpp"

namespace {
template <class T> struct DevArr {
    T* p = nullptr;
    ~DevArr() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)); }
};
struct PinArr {
    void* p = nullptr;
    ~PinArr() { if (p) (void)hipHostFree(p); }
};
struct ScratchCtx {
    ggl_ctx* c = nullptr;
    ~ScratchCtx() { if (c) ggl_ctx_destroy(c); }
};

int check_nc_args(int B, double eps, double tol, int max_iter, const int* iters, const double* info)
{
    // (B is the y extent of the kernels' grids)
    if (B > 65535) return fail(GGL_E_ARG, "bad argument: B = %d matrices, one call takes at most 65535", B);
    if (!(eps >= 0.0 && eps <= 0.5)) return fail(GGL_E_ARG, "bad argument: eps = %g, the eigenvalue floor lies in [0, 0.5]", eps);
    if (!(tol >= 1e-14 && tol <= 1e-2)) return fail(GGL_E_ARG, "bad argument: tol = %g, the tolerance lies in [1e-14, 1e-2]", tol);
    if (max_iter < 1) return fail(GGL_E_ARG, "bad argument: max_iter = %d, at least one iteration is needed", max_iter);
    ARGCHK(iters && info, "iters (B) and info (B,4) must not be NULL");
    return GGL_OK;
}

// The B = s->K matrices at raw (device) are projected into dst (device; may be raw) with the stacks of the scratch ctx s:
// A0 = s->S, Y = s->Theta, dS = s->X, R = s->W (what rank_step reads), X = s->L (what it writes).  diag(A), the error word and
// the flags live in buffers of the call's own: rank_step's eigendecomposition fallback uses the ctx's small scratch (scale, E,
// info) for itself.
// Nothing is written to dst unless every matrix passed the input check.  Waits for s->stream.
int nc_project(ggl_ctx* s, const double* raw, double* dst, double eps, double tol, int max_iter, int* iters, double* info,
               const char* what)
{
    const int B = s->K, p = s->p;
    ARGCHK((size_t)B * p < (size_t)GGL_DIAG_OK, "B * p too large");
    DevArr<int> dErr;
    DevArr<double> dDiag;
    HIPCHK(dErr.alloc(1));
    HIPCHK(dDiag.alloc((size_t)B * p));
    HIPCHK(hipMemsetAsync(dErr.p, 0x7f, sizeof(int), s->stream));
    // device-visible host words: frozen[B] | pass[B] flags, nu[B]
    PinArr pin;
    HIPCHK(hipHostMalloc(&pin.p, (size_t)B * (2 * sizeof(int) + sizeof(double)) + 16));
    double* nu = (double*)pin.p;
    int* frozen = (int*)(nu + B);
    int* pass = frozen + B;
    for (int b = 0; b < B; ++b) { nu[b] = 0.0; frozen[b] = 0; pass[b] = 0; }
    double *A0 = s->S, *Y = s->Theta, *dS = s->X;
    launch_nc_begin(s->stream, raw, A0, Y, dS, s->W, dDiag.p, dErr.p, B, p);
    HIPCHK(hipGetLastError());
    int err = GGL_DIAG_OK;
    HIPCHK(hipMemcpyAsync(&err, dErr.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (err != GGL_DIAG_OK)
        return fail(GGL_E_ARG, "bad argument: %s of instance %d, variable %d: its row holds a non-finite entry or its diagonal entry "
                    "is not positive; the projection needs a finite matrix with a positive diagonal", what, err / p, err % p);
    const int nblk = nc_update_blocks(p), nfin = nc_finish_blocks(p);
    int rc = ensure_partials(s, (size_t)B * std::max(3 * nblk, nfin));
    if (rc) return rc;
    std::vector<double> delta(B, 0.0), res(B, 0.0);
    int nfrozen = 0;
    s->info_dirty = false;          // (a fresh ctx: no eigensolver has written `info` yet; rank_step says when one has)
    for (int it = 1; it <= max_iter && nfrozen < B; ++it) {
        rc = upload_par(s, 2, nullptr, eps, 1.0);
        if (!rc) rc = rank_step(s);
        if (rc) return rc;
        // (rank_step swaps W and Ckeep on its sign-iteration route: s->W is taken here, behind it)
        launch_nc_update(s->stream, s->L, Y, dS, s->W, s->partials, frozen, dErr.p, eps, B, p);
        launch_nc_reduce(s->stream, s->partials, s->norms_h, dErr.p, B, nblk, 3);
        HIPCHK(hipGetLastError());
        const bool eig_ran = s->info_dirty;
        if (eig_ran) HIPCHK(hipMemcpyAsync(s->info_h, s->info, B * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        // the one wait of the iteration that is ours: rank_step's own lies in front of the update, so it cannot carry these
        // sums, and reading them behind the NEXT rank_step instead would cost a whole rank_step once everything has stopped
        HIPCHK(hipStreamSynchronize(s->stream));
        if (eig_ran) {
            rc = check_info(s, "nearest correlation");
            if (rc) return rc;
            s->info_dirty = false;
        }
        for (int b = 0; b < B; ++b) {
            if (frozen[b]) continue;
            const double* sm = s->norms_h + (size_t)b * 8;
            if (!std::isfinite(sm[0]) || !std::isfinite(sm[1]) || !(sm[2] > 0.0) || !std::isfinite(sm[2]))
                return fail(GGL_E_SOLVER, "nearest correlation: non-finite iterate of instance %d in iteration %d", b, it);
            const double ny = std::sqrt(sm[2]);
            delta[b] = std::sqrt(sm[1]);
            res[b] = std::max(std::sqrt(sm[0]) / ny, delta[b] / ny);
            if (res[b] <= tol) {
                frozen[b] = 1;
                pass[b] = it == 1;          // the input needed no projection: it is returned bit for bit
                iters[b] = it;
                nfrozen += 1;
            }
        }
    }
    for (int b = 0; b < B; ++b) {
        if (!frozen[b]) iters[b] = -max_iter;
        nu[b] = pass[b] ? 0.0 : delta[b] / (1.0 - eps + delta[b]);
    }
    launch_nc_finish(s->stream, Y, raw, dst, dDiag.p, nu, pass, s->partials, dErr.p, B, p);
    launch_nc_reduce(s->stream, s->partials, s->norms_h, dErr.p, B, nfin, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    for (int b = 0; b < B; ++b) {
        info[4 * (size_t)b + 0] = res[b];
        info[4 * (size_t)b + 1] = std::sqrt(s->norms_h[(size_t)b * 8]);
        info[4 * (size_t)b + 2] = nu[b];
        info[4 * (size_t)b + 3] = (double)s->rank_fallbacks;
    }
    return GGL_OK;
}
}  // namespace

extern "C" int ggl_nearest_correlation(int B, int p, const double* A, double* out, double eps, double tol, int max_iter, int* iters,
                                       double* info)
{
    ARGCHK(B >= 1 && p >= 1, "B >= 1, p >= 1");
    ARGCHK(A && out, "A and out must not be NULL");
    int rc = check_nc_args(B, eps, tol, max_iter, iters, info);
    if (rc) return rc;
    ScratchCtx s;
    rc = ggl_ctx_create(0, B, p, GGL_EIG_AUTO, nullptr, &s.c);
    if (rc) return rc;
    ggl_ctx* c = s.c;
    HIPCHK(hipMemcpyAsync(c->Om[0], A, c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rc = nc_project(c, c->Om[0], c->Om[1], eps, tol, max_iter, iters, info, "A");
    if (rc) return rc;
    DOWN(out, c->Om[1], c->n);
    return GGL_OK;
}

extern "C" int ggl_project_S(ggl_ctx* c, int period, double eps, double tol, int max_iter, int* iters, double* info)
{
    ARGCHK(c, "ctx");
    ARGCHK(!c->has_dims, "a ctx with instance dimensions (ggl_set_instance_dims) is not projected");
    if (period < 0 || period > c->K || (period > 0 && c->K % period != 0))
        return fail(GGL_E_ARG, "bad argument: period = %d, 0 (all K = %d matrices) or a divisor of K", period, c->K);
    int rc = check_nc_args(period > 0 ? period : c->K, eps, tol, max_iter, iters, info);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    const int B = period > 0 ? period : c->K;
    {
        ScratchCtx s;
        rc = ggl_ctx_create(c->device, B, c->p, GGL_EIG_AUTO, nullptr, &s.c);
        if (rc) return rc;
        rc = nc_project(s.c, c->S, c->S, eps, tol, max_iter, iters, info, "S");
        if (rc) return rc;          // (a refused call: S as it was)
    }
    // what earlier iterations carried is forgotten, as in ggl_set_S; the variances of a correlation S stay (the diagonal is kept)
    s_replaced_begin(c);
    rc = replicate_instances(c, c->S, B);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return s_replaced_end(c);
}
