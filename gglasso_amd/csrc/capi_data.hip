// C ABI: the input side -- everything that makes an S from data, as stateless operators (host buffers in, host buffers out)
// and straight into the S of a ctx: sample covariance of K instances or of column subsets of one array and scaling by a
// diagonal (kernels: covariance.hip), pairwise-complete covariance of data with NaN (covariance_missing.hip), weighted
// covariance (covariance_weighted.hip), Kendall's tau and the latent correlation of mixed data (kendall.hip, bridge.hip), and
// the held-out scores of a cross-validation (stars.hip).  The idioms the routes share stand once, in the namespace below.
#include "capi_internal.hpp"

namespace {
template <class T> struct DevArr {
    T* p = nullptr;
    ~DevArr() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T) + STACK_SLACK); }
};

constexpr int COV_FLAGS = GGL_COV_CENTER | GGL_COV_SCALE | GGL_COV_TILE32 | GGL_COV_TILE64;
constexpr int WCOV_FLAGS = COV_FLAGS | GGL_COV_FULL_RANGE;

int check_cov_flags(int flags, int allowed)
{
    ARGCHK((flags & ~allowed) == 0,
           (allowed & GGL_COV_FULL_RANGE)
               ? "flags: unknown bits (GGL_COV_CENTER | GGL_COV_SCALE | GGL_COV_TILE32 | GGL_COV_TILE64 | GGL_COV_FULL_RANGE)"
               : "flags: unknown bits (GGL_COV_CENTER | GGL_COV_SCALE | GGL_COV_TILE32 | GGL_COV_TILE64)");
    ARGCHK(!((flags & GGL_COV_TILE32) && (flags & GGL_COV_TILE64)), "flags: GGL_COV_TILE32 and GGL_COV_TILE64 exclude each other");
    return GGL_OK;
}

// the tile argument of the Gram launchers: 0 by size, 32, 64
int cov_tile(int flags) { return (flags & GGL_COV_TILE64) ? 64 : ((flags & GGL_COV_TILE32) ? 32 : 0); }

// idx (rows, cols): every entry in [0, N).  what: "subset" or "fold", for the message
int check_index_table(const int* idx, int rows, int cols, int N, const char* what)
{
    for (int r = 0; r < rows; ++r)
        for (int q = 0; q < cols; ++q) {
            const int n = idx[(size_t)r * cols + q];
            if (n < 0 || n >= N)
                return fail(GGL_E_ARG, "bad argument: %s %d, position %d holds the index %d, outside [0, %d)", what, r, q, n, N);
        }
    return GGL_OK;
}

// what every route into a ctx's S asks of the ctx first, and of a period B
int check_ctx_takes_S(const ggl_ctx* c)
{
    ARGCHK(c, "ctx");
    ARGCHK(!c->has_dims, "a ctx with instance dimensions (ggl_set_instance_dims) takes its S from ggl_set_S");
    return GGL_OK;
}

int check_divides_K(const ggl_ctx* c, int B)
{
    if (c->K % B != 0) return fail(GGL_E_ARG, "bad argument: B = %d subsets do not divide the K = %d instances of the ctx", B, c->K);
    return GGL_OK;
}

// an error word a kernel left on the device, once the stream has run dry: the 32-bit word (GGL_DIAG_OK: none) and the 64-bit
// word (every bit set: none)
int read_err_word(hipStream_t st, const int* err_d, int* err)
{
    *err = GGL_DIAG_OK;
    HIPCHK(hipMemcpyAsync(err, err_d, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}

int read_err_word64(hipStream_t st, const unsigned long long* err_d, unsigned long long* err)
{
    *err = ~0ull;
    HIPCHK(hipMemcpyAsync(err, err_d, sizeof(*err), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}

int check_data_args(int K, int p, const int* N, const double* const* X_host, int flags)
{
    ARGCHK(K >= 1 && p >= 1, "K >= 1, p >= 1");
    ARGCHK(N && X_host, "N, X");
    RCCHK(check_cov_flags(flags, COV_FLAGS));
    ARGCHK((size_t)K * p < (size_t)GGL_DIAG_OK, "K * p too large");
    for (int k = 0; k < K; ++k) {
        if (!X_host[k]) return fail(GGL_E_ARG, "bad argument: X[%d] is NULL", k);
        if (N[k] < 1) return fail(GGL_E_ARG, "bad argument: N[%d] = %d, every instance needs at least one sample", k, N[k]);
    }
    return GGL_OK;
}

// the error word of launch_scale_by_diag -> GGL_E_ARG naming instance and variable.  dvals: the (K,p) diagonal on the device
// as far as it was written (null: d_host holds the caller's), Xdiag: the stack the diagonal was taken from
int diag_error(hipStream_t st, const int* err_d, int p, const double* d_host, const double* Xdiag, const char* what)
{
    int err;
    RCCHK(read_err_word(st, err_d, &err));
    if (err == GGL_DIAG_OK) return GGL_OK;
    const int k = err / p, i = err % p;
    double v = 0.0;
    if (d_host) v = d_host[err];
    else HIPCHK(hipMemcpy(&v, Xdiag + (size_t)k * p * p + (size_t)i * p + i, sizeof(double), hipMemcpyDeviceToHost));
    return fail(GGL_E_ARG, "bad argument: %s of instance %d, variable %d is %g; scaling by the diagonal needs positive finite values",
                what, k, i, v);
}

// GGL_COV_SCALE: S_dev (K,p,p) is divided by its own diagonal in place, var_dev (K,p) gets the diagonal; a variance that is not
// positive and finite is refused naming `what`
int scale_in_place(hipStream_t st, int K, int p, double* S_dev, double* var_dev, const char* what)
{
    DevArr<double> dSd;
    DevArr<int> dErr;
    HIPCHK(dSd.alloc((size_t)K * p));
    HIPCHK(dErr.alloc(1));
    HIPCHK(hipMemsetAsync(dErr.p, 0x7f, sizeof(int), st));
    launch_scale_by_diag(st, S_dev, nullptr, S_dev, var_dev, dSd.p, dErr.p, K, p);
    HIPCHK(hipGetLastError());
    return diag_error(st, dErr.p, p, nullptr, S_dev, what);
}

// The data on the device as the Gram kernels read them: one arena of sum_k p N_k doubles, instance k the packed row-major
// (p, N_k) array at off[k], and the two tables.  Filled on a stream; the host tables live as long as the arena, which a
// caller frees only behind a wait for that stream (the *_of_arena functions end with one).
struct Arena {
    int K = 0;
    DevArr<double> X, src;
    DevArr<long long> off;
    DevArr<int> N, idx;
    std::vector<long long> off_h;
    std::vector<int> N_h;

    int tables(hipStream_t st, int K_, int p, const int* Nk)
    {
        K = K_;
        off_h.resize(K);
        N_h.assign(Nk, Nk + K);
        size_t total = 0;
        for (int k = 0; k < K; ++k) { off_h[k] = (long long)total; total += (size_t)p * N_h[k]; }
        HIPCHK(X.alloc(total));
        HIPCHK(off.alloc(K));
        HIPCHK(N.alloc(K));
        HIPCHK(hipMemcpyAsync(off.p, off_h.data(), K * sizeof(long long), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(N.p, N_h.data(), K * sizeof(int), hipMemcpyHostToDevice, st));
        return GGL_OK;
    }
    // K instances from the host, each going up once (NaNs travel as they are)
    int from_instances(hipStream_t st, int K_, int p, const int* Nk, const double* const* X_host)
    {
        RCCHK(tables(st, K_, p, Nk));
        for (int k = 0; k < K; ++k)
            HIPCHK(hipMemcpyAsync(X.p + off_h[k], X_host[k], (size_t)p * N_h[k] * sizeof(double), hipMemcpyHostToDevice, st));
        return GGL_OK;
    }
    // B column subsets idx (B,b) of one (p,N) array: X goes up once, the columns are gathered on the device (k_gather_cols,
    // stars.hip, moves bytes: NaNs travel)
    int from_subsets(hipStream_t st, int p, int Ncols, const double* X_host, int B, int b, const int* idx_host)
    {
        const std::vector<int> Nb(B, b);
        RCCHK(tables(st, B, p, Nb.data()));
        HIPCHK(src.alloc((size_t)p * Ncols));
        HIPCHK(idx.alloc((size_t)B * b));
        HIPCHK(hipMemcpyAsync(src.p, X_host, (size_t)p * Ncols * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(idx.p, idx_host, (size_t)B * b * sizeof(int), hipMemcpyHostToDevice, st));
        launch_gather_cols(st, src.p, idx.p, X.p, p, Ncols, B, b);
        HIPCHK(hipGetLastError());
        return GGL_OK;
    }
};

// S_dev (K,p,p) from the arena on stream st; with GGL_COV_SCALE the correlations, and the variances in var_dev (K,p).  Waits
// for the stream: the caller may free the arena on return.
int covariance_of_arena(hipStream_t st, const Arena& a, int p, int flags, double* S_dev, double* var_dev)
{
    DevArr<double> dMean;
    const bool center = (flags & GGL_COV_CENTER) != 0;
    if (center) {
        HIPCHK(dMean.alloc((size_t)a.K * p));
        launch_row_means(st, a.X.p, a.off.p, a.N.p, dMean.p, a.K, p);
        HIPCHK(hipGetLastError());
    }
    launch_gram_nt(st, a.X.p, a.off.p, a.N.p, center ? dMean.p : nullptr, S_dev, a.K, p, cov_tile(flags));
    HIPCHK(hipGetLastError());
    if (flags & GGL_COV_SCALE) RCCHK(scale_in_place(st, a.K, p, S_dev, var_dev, "the variance"));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}

// ... from the host data of K instances
int covariance_to_device(hipStream_t st, int K, int p, const int* N, const double* const* X_host, int flags, double* S_dev,
                         double* var_dev)
{
    Arena a;
    RCCHK(a.from_instances(st, K, p, N, X_host));
    return covariance_of_arena(st, a, p, flags, S_dev, var_dev);
}

// The device results of a stateless covariance call and their way to the caller.  begin: the two checks of the output
// arguments every such call makes behind its own, the device, the buffers; down: the last step of a call that was not refused.
struct CovOut {
    DevBuf S, var, wsum;
    DevArr<int> cnt;
    size_t K = 0, p = 0;
    int begin(int device, int K_, int p_, int flags, const double* S_out, const double* scale_out, bool counts, bool sums)
    {
        ARGCHK(S_out, "S_out");
        ARGCHK(!(flags & GGL_COV_SCALE) || scale_out, "GGL_COV_SCALE needs scale_out");
        HIPCHK(hipSetDevice(device));
        K = K_;
        p = p_;
        HIPCHK(S.alloc(K * p * p));
        HIPCHK(var.alloc(K * p));
        if (sums) HIPCHK(wsum.alloc(K));
        if (counts) HIPCHK(cnt.alloc(K * p * p));
        return GGL_OK;
    }
    int down(int flags, double* S_out, double* scale_out, int* counts_out = nullptr, double* wsum_out = nullptr)
    {
        DOWN(S_out, S.p, K * p * p);
        if (flags & GGL_COV_SCALE) DOWN(scale_out, var.p, K * p);
        if (wsum_out) DOWN(wsum_out, wsum.p, K);
        if (counts_out) HIPCHK(hipMemcpy(counts_out, cnt.p, K * p * p * sizeof(int), hipMemcpyDeviceToHost));
        return GGL_OK;
    }
};
}  // namespace

extern "C" int ggl_covariance(int device, int K, int p, const int* N, const double* const* X_host, int flags, double* S_out,
                              double* scale_out)
{
    RCCHK(check_data_args(K, p, N, X_host, flags));
    CovOut d;
    RCCHK(d.begin(device, K, p, flags, S_out, scale_out, false, false));
    RCCHK(covariance_to_device(nullptr, K, p, N, X_host, flags, d.S.p, d.var.p));
    return d.down(flags, S_out, scale_out);
}

extern "C" int ggl_scale_by_diagonal(int device, int K, int p, const double* X_host, const double* d_in, double* Y_out,
                                     double* d_out)
{
    ARGCHK(K >= 1 && p >= 1, "K >= 1, p >= 1");
    ARGCHK(X_host && Y_out, "X, Y_out");
    ARGCHK((size_t)K * p < (size_t)GGL_DIAG_OK, "K * p too large");
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)K * p * p, kp = (size_t)K * p;
    DevBuf dX, dY, dD, dDo, dSd;
    DevArr<int> dErr;
    HIPCHK(dX.alloc(n));
    HIPCHK(dY.alloc(n));
    HIPCHK(dDo.alloc(kp));
    HIPCHK(dSd.alloc(kp));
    HIPCHK(dErr.alloc(1));
    UP(dX.p, X_host, n);
    if (d_in) { HIPCHK(dD.alloc(kp)); UP(dD.p, d_in, kp); }
    HIPCHK(hipMemset(dErr.p, 0x7f, sizeof(int)));
    launch_scale_by_diag(nullptr, dX.p, d_in ? dD.p : nullptr, dY.p, dDo.p, dSd.p, dErr.p, K, p);
    HIPCHK(hipGetLastError());
    RCCHK(diag_error(nullptr, dErr.p, p, d_in, dX.p, d_in ? "d" : "the diagonal"));
    DOWN(Y_out, dY.p, n);
    if (d_out) DOWN(d_out, dDo.p, kp);
    return GGL_OK;
}

extern "C" int ggl_set_S_from_data(ggl_ctx* c, const double* const* X_host, const int* N, int flags)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_data_args(c->K, c->p, N, X_host, flags));
    // S is overwritten from here on, also where a later step fails: nothing built for the old S may survive
    s_replaced_begin(c);
    c->cov_scale.clear();
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    const size_t kp = (size_t)c->K * c->p;
    DevBuf dVar;
    HIPCHK(dVar.alloc(kp));
    RCCHK(covariance_to_device(c->stream, c->K, c->p, N, X_host, flags, c->S, dVar.p));
    if (flags & GGL_COV_SCALE) {
        c->cov_scale.resize(kp);
        HIPCHK(hipMemcpyAsync(c->cov_scale.data(), dVar.p, kp * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return s_replaced_end(c);
}

extern "C" int ggl_get_S(ggl_ctx* c, double* S_out, double* scale_out)
{
    ARGCHK(c && S_out, "ctx, S_out");
    ARGCHK(!scale_out || !c->cov_scale.empty(), "scale_out: the S of this ctx was not computed from data with GGL_COV_SCALE");
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    RCCHK(download_stacks(c, {{S_out, c->S, c->n * sizeof(double)}}));
    if (scale_out) std::memcpy(scale_out, c->cov_scale.data(), c->cov_scale.size() * sizeof(double));
    return GGL_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// covariances of B column subsets of one X (the subsamples of StARS stability selection): the arena of the subsets is what
// the kernels above read as a K = B call
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// everything but the range of the indices
int check_subset_sizes(int p, int N, const double* X_host, int B, int b, const int* idx, int flags)
{
    ARGCHK(p >= 1 && N >= 1, "p >= 1, N >= 1");
    ARGCHK(X_host && idx, "X, idx");
    RCCHK(check_cov_flags(flags, COV_FLAGS));
    if (B < 1 || B > 65535) return fail(GGL_E_ARG, "bad argument: B = %d subsets, 1 .. 65535 are possible", B);
    if (b < 1) return fail(GGL_E_ARG, "bad argument: b = %d, every subset needs at least one sample", b);
    ARGCHK((size_t)B * p < (size_t)GGL_DIAG_OK, "B * p too large");
    return GGL_OK;
}

int check_subset_args(int p, int N, const double* X_host, int B, int b, const int* idx, int flags)
{
    RCCHK(check_subset_sizes(p, N, X_host, B, b, idx, flags));
    return check_index_table(idx, B, b, N, "subset");
}

// S_dev (B,p,p) and var_dev (B,p) of the subsets on stream st; the arguments have been checked
int subsets_to_device(hipStream_t st, int p, int N, const double* X_host, int B, int b, const int* idx, int flags,
                      double* S_dev, double* var_dev)
{
    Arena a;
    RCCHK(a.from_subsets(st, p, N, X_host, B, b, idx));
    return covariance_of_arena(st, a, p, flags, S_dev, var_dev);
}

// The B complete matrices dS (B,p,p) become the S of the ctx, instance k = subset k % B (the layout of ggl_set_S_ex with period
// B), replicated device to device; with GGL_COV_SCALE in flags dVar (B,p, device) holds the variances that go with them.  What
// earlier iterations carried is forgotten, as in ggl_set_S.
int install_subset_S(ggl_ctx* c, const double* dS, int B, const double* dVar = nullptr, int flags = 0)
{
    std::vector<double> var;
    if (flags & GGL_COV_SCALE) {
        var.resize((size_t)B * c->p);
        HIPCHK(hipMemcpyAsync(var.data(), dVar, var.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    s_replaced_begin(c);
    c->cov_scale.clear();
    HIPCHK(hipMemcpyAsync(c->S, dS, (size_t)B * c->p * c->p * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    RCCHK(replicate_instances(c, c->S, B));
    if (!var.empty()) {
        c->cov_scale.resize((size_t)c->K * c->p);
        for (int k = 0; k < c->K; ++k)
            std::memcpy(c->cov_scale.data() + (size_t)k * c->p, var.data() + (size_t)(k % B) * c->p, c->p * sizeof(double));
    }
    HIPCHK(hipStreamSynchronize(c->stream));      // (the caller frees dS on return)
    return s_replaced_end(c);
}
}  // namespace

extern "C" int ggl_covariance_subsets(int device, int p, int N, const double* X_host, int B, int b, const int* idx, int flags,
                                      double* S_out, double* scale_out)
{
    RCCHK(check_subset_args(p, N, X_host, B, b, idx, flags));
    CovOut d;
    RCCHK(d.begin(device, B, p, flags, S_out, scale_out, false, false));
    RCCHK(subsets_to_device(nullptr, p, N, X_host, B, b, idx, flags, d.S.p, d.var.p));
    return d.down(flags, S_out, scale_out);
}

extern "C" int ggl_set_S_from_subsets(ggl_ctx* c, const double* X_host, int N, int B, int b, const int* idx, int flags)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_subset_args(c->p, N, X_host, B, b, idx, flags));
    RCCHK(check_divides_K(c, B));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    // The B matrices are built beside the ctx's S, which is overwritten only once they are complete: a call that is refused
    // (here or by the variance check of GGL_COV_SCALE) leaves S, and what was built for it, as it was.
    DevBuf dS, dVar;
    HIPCHK(dS.alloc((size_t)B * c->p * c->p));
    HIPCHK(dVar.alloc((size_t)B * c->p));
    RCCHK(subsets_to_device(c->stream, c->p, N, X_host, B, b, idx, flags, dS.p, dVar.p));
    return install_subset_S(c, dS.p, B, dVar.p, flags);
}

// K-fold cross-validation: the held-out score <S_test[k % F], Theta_k> of every snapshot of a ctx of K = L * F instances
// (k_heldout_dot, stars.hip) beside the three numbers of ggl_selection_stats, whose route it takes.  The test covariances
// are built as above, beside the ctx: its S is neither read nor written.
extern "C" int ggl_heldout_scores(ggl_ctx* c, const double* X_host, int N, int F, int m, const int* idx_test, int flags,
                                  double* out)
{
    ARGCHK(c, "ctx");
    ARGCHK(X_host, "X");
    ARGCHK(idx_test, "idx_test");
    ARGCHK(out, "out");
    ARGCHK(!c->has_dims, "a ctx with instance dimensions (ggl_set_instance_dims) has no held-out scores");
    if ((flags & ~GGL_COV_CENTER) != 0)
        return fail(GGL_E_ARG, "bad argument: flags = %d, held-out scores take GGL_COV_CENTER or 0 (no GGL_COV_SCALE: the folds share one scale)", flags);
    if (F < 1 || F > 65535 || c->K % F != 0)
        return fail(GGL_E_ARG, "bad argument: F = %d folds do not divide the K = %d instances of the ctx", F, c->K);
    if (m < 1) return fail(GGL_E_ARG, "bad argument: m = %d, every test fold needs at least one observation", m);
    ARGCHK(N >= 1, "N >= 1");
    RCCHK(check_index_table(idx_test, F, m, N, "fold"));
    ARGCHK(c->snapT, "no snapshot taken (ggl_snapshot_k)");
    ARGCHK((size_t)c->K * heldout_blocks(c->p) < ((size_t)1 << 31), "K * p * p too large for one launch");
    RCCHK(check_subset_sizes(c->p, N, X_host, F, m, idx_test, flags));      // (the sizes the covariance route takes)
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    DevBuf dS, dVar;
    HIPCHK(dS.alloc((size_t)F * c->p * c->p));
    HIPCHK(dVar.alloc((size_t)F * c->p));
    RCCHK(subsets_to_device(c->stream, c->p, N, X_host, F, m, idx_test, flags, dS.p, dVar.p));
    // (waits for the stream before it returns: dS is freed behind it)
    return selection_stats_impl(c, out, dS.p, F);
}

// The test-fold side of ggl_heldout_scores for a caller in another file (ggl_neighborhood_cv): the same refusals about the
// folds, then the same route to the F test covariances, so the same bits.  dS (F,p,p) and dVar (F,p) are the caller's.
int heldout_fold_check(ggl_ctx* c, const double* X_host, int N, int F, int m, const int* idx_test, int flags)
{
    ARGCHK(X_host, "X");
    ARGCHK(idx_test, "idx_test");
    if ((flags & ~GGL_COV_CENTER) != 0)
        return fail(GGL_E_ARG, "bad argument: flags = %d, held-out scores take GGL_COV_CENTER or 0 (no GGL_COV_SCALE: the folds share one scale)", flags);
    if (F < 1 || F > 65535 || c->K % F != 0)
        return fail(GGL_E_ARG, "bad argument: F = %d folds do not divide the K = %d instances of the ctx", F, c->K);
    if (m < 1) return fail(GGL_E_ARG, "bad argument: m = %d, every test fold needs at least one observation", m);
    ARGCHK(N >= 1, "N >= 1");
    RCCHK(check_index_table(idx_test, F, m, N, "fold"));
    return check_subset_sizes(c->p, N, X_host, F, m, idx_test, flags);
}

int heldout_fold_covariances(ggl_ctx* c, const double* X_host, int N, int F, int m, const int* idx_test, int flags, double* dS,
                             double* dVar)
{
    return subsets_to_device(c->stream, c->p, N, X_host, F, m, idx_test, flags, dS, dVar);
}

// ---------------------------------------------------------------------------------------------------------------------
// Kendall's tau-b and the skeptic matrix sin(pi/2 tau) from dense ranks (kernels: kendall.hip): the ranks go up once, the
// columns of the B subsets are gathered on the device, the counts G = Z Z^T are exact 64-bit integers
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_kendall_args(int p, int N, const int* ranks_host, int B, int b, const int* idx)
{
    ARGCHK(p >= 1 && N >= 1, "p >= 1, N >= 1");
    ARGCHK(ranks_host, "ranks");
    if (B < 1 || B > 65535) return fail(GGL_E_ARG, "bad argument: B = %d subsets, 1 .. 65535 are possible", B);
    if (!idx && (B != 1 || b != N))
        return fail(GGL_E_ARG, "bad argument: idx = NULL takes all N = %d samples as one subset: B = 1, b = N (B = %d, b = %d)", N, B, b);
    if (b < 2) return fail(GGL_E_ARG, "bad argument: b = %d, a subset needs at least two samples to form a pair", b);
    ARGCHK((size_t)B * p < (size_t)GGL_DIAG_OK, "B * p too large");
    ARGCHK(kendall_counts_fit(p, b, B), "p and b are beyond what one launch takes (p * b < 2^31, p <= 23104, b below about one million)");
    if (idx) {
        RCCHK(check_index_table(idx, B, b, N, "subset"));
    }
    // dense ranks lie in [0, N): their differences then fit 32 bits
    for (size_t e = 0; e < (size_t)p * N; ++e)
        if (ranks_host[e] < 0 || ranks_host[e] >= N)
            return fail(GGL_E_ARG, "bad argument: variable %d, sample %d holds the rank %d, outside [0, %d)", (int)(e / N), (int)(e % N),
                        ranks_host[e], N);
    return GGL_OK;
}

// G_dev (B,p,p) int64 on stream st, and with S_dev the skeptic matrices (B,p,p) -- GGL_E_ARG naming subset and variable where
// a variable is constant over a subset, S_dev is not written then.  The arguments have been checked.  Waits for the stream.
int kendall_to_device(hipStream_t st, int p, int N, const int* ranks_host, int B, int b, const int* idx, long long* G_dev,
                      double* S_dev, DevArr<int>* keep = nullptr)
{
    DevArr<int> dR, dA, dIdx, dErr;
    HIPCHK(dR.alloc((size_t)p * N));
    HIPCHK(hipMemcpyAsync(dR.p, ranks_host, (size_t)p * N * sizeof(int), hipMemcpyHostToDevice, st));
    const int* Rg = dR.p;
    if (idx) {
        HIPCHK(dA.alloc((size_t)B * p * b));
        HIPCHK(dIdx.alloc((size_t)B * b));
        HIPCHK(hipMemcpyAsync(dIdx.p, idx, (size_t)B * b * sizeof(int), hipMemcpyHostToDevice, st));
        launch_gather_ranks(st, dR.p, dIdx.p, dA.p, p, N, B, b);
        HIPCHK(hipGetLastError());
        Rg = dA.p;
    }
    launch_kendall_counts(st, Rg, G_dev, B, p, b);
    HIPCHK(hipGetLastError());
    // keep: the caller goes on with the B packed (p,b) rank arrays the counts were taken from (the mixed route), and owns them
    if (keep) std::swap(keep->p, idx ? dA.p : dR.p);
    if (S_dev) {
        HIPCHK(dErr.alloc(1));
        HIPCHK(hipMemsetAsync(dErr.p, 0x7f, sizeof(int), st));
        launch_kendall_skeptic(st, G_dev, S_dev, dErr.p, B, p);
        HIPCHK(hipGetLastError());
        int err;
        RCCHK(read_err_word(st, dErr.p, &err));
        if (err != GGL_DIAG_OK)
            return fail(GGL_E_ARG, "bad argument: variable %d is constant over subset %d (no untied pair of samples); the rank "
                        "correlation needs every variable to vary", err % p, err / p);
    }
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}

int kendall_call(int device, int p, int N, const int* ranks_host, int B, int b, const int* idx, double* S_out, long long* G_out)
{
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)B * p * p;
    DevArr<long long> dG;
    DevBuf dS;
    HIPCHK(dG.alloc(n));
    if (S_out) HIPCHK(dS.alloc(n));
    RCCHK(kendall_to_device(nullptr, p, N, ranks_host, B, b, idx, dG.p, S_out ? dS.p : nullptr));
    if (G_out) HIPCHK(hipMemcpy(G_out, dG.p, n * sizeof(long long), hipMemcpyDeviceToHost));
    if (S_out) DOWN(S_out, dS.p, n);
    return GGL_OK;
}
}  // namespace

extern "C" int ggl_kendall_counts(int device, int p, int N, const int* ranks_host, int B, int b, const int* idx, long long* G_out)
{
    RCCHK(check_kendall_args(p, N, ranks_host, B, b, idx));
    ARGCHK(G_out, "G_out");
    return kendall_call(device, p, N, ranks_host, B, b, idx, nullptr, G_out);
}

extern "C" int ggl_kendall_skeptic(int device, int p, int N, const int* ranks_host, int B, int b, const int* idx, double* S_out,
                                   long long* G_out)
{
    RCCHK(check_kendall_args(p, N, ranks_host, B, b, idx));
    ARGCHK(S_out, "S_out");
    return kendall_call(device, p, N, ranks_host, B, b, idx, S_out, G_out);
}

extern "C" int ggl_set_S_from_kendall(ggl_ctx* c, const int* ranks_host, int N, int B, int b, const int* idx)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_kendall_args(c->p, N, ranks_host, B, b, idx));
    RCCHK(check_divides_K(c, B));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    // as ggl_set_S_from_subsets: the B matrices are built beside the ctx's S; a refused call (a constant variable) leaves S alone
    const size_t n = (size_t)B * c->p * c->p;
    DevArr<long long> dG;
    DevBuf dS;
    HIPCHK(dG.alloc(n));
    HIPCHK(dS.alloc(n));
    RCCHK(kendall_to_device(c->stream, c->p, N, ranks_host, B, b, idx, dG.p, dS.p));
    return install_subset_S(c, dS.p, B);
}

// ---------------------------------------------------------------------------------------------------------------------
// Latent correlation of mixed binary / continuous data (kernels: bridge.hip): the counts of the route above, the zero counts
// of the binary variables from the same gathered ranks, and one root of the bridge function per pair of variables
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_mixed_args(int p, int N, const int* ranks_host, const int* types, int B, int b, const int* idx, double clip)
{
    RCCHK(check_kendall_args(p, N, ranks_host, B, b, idx));
    ARGCHK(types, "types");
    if (!(clip > 0.0 && clip < 1.0)) return fail(GGL_E_ARG, "bad argument: clip = %g, outside (0, 1)", clip);
    for (int i = 0; i < p; ++i) {
        if (types[i] != 0 && types[i] != 1)
            return fail(GGL_E_ARG, "bad argument: types[%d] = %d, a variable is continuous (0) or binary (1)", i, types[i]);
        int top = 0;
        for (int n = 0; n < N; ++n) top = std::max(top, ranks_host[(size_t)i * N + n]);
        if (top == 0)
            return fail(GGL_E_ARG, "bad argument: variable %d is constant (every rank is 0); the rank correlation needs every "
                        "variable to vary", i);
        if (types[i] == 1 && top > 1)
            return fail(GGL_E_ARG, "bad argument: variable %d is marked binary and holds the rank %d; a binary variable has the "
                        "dense ranks 0 and 1", i, top);
    }
    return GGL_OK;
}

// S_dev (B,p,p), G_dev (B,p,p), n0_dev (B,p), clip_dev (B) on stream st -- GGL_E_ARG naming subset and variable where a variable
// takes one value over a subset; S_dev is not written then.  The arguments have been checked.  Waits for the stream.
int mixed_to_device(hipStream_t st, int p, int N, const int* ranks_host, const int* types, int B, int b, const int* idx,
                    double clip, double* S_dev, long long* G_dev, int* n0_dev, int* clip_dev)
{
    DevArr<int> dRg, dT, dErr;
    HIPCHK(dT.alloc(p));
    HIPCHK(dErr.alloc(1));
    HIPCHK(hipMemcpyAsync(dT.p, types, (size_t)p * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dErr.p, 0x7f, sizeof(int), st));
    RCCHK(kendall_to_device(st, p, N, ranks_host, B, b, idx, G_dev, nullptr, &dRg));
    launch_bridge_zero_counts(st, dRg.p, n0_dev, dErr.p, B, p, b);
    HIPCHK(hipGetLastError());
    launch_bridge_invert(st, G_dev, n0_dev, dT.p, S_dev, clip_dev, dErr.p, B, p, b, clip);
    HIPCHK(hipGetLastError());
    int err;
    RCCHK(read_err_word(st, dErr.p, &err));
    if (err != GGL_DIAG_OK)
        return fail(GGL_E_ARG, "bad argument: variable %d is constant over subset %d (%s); the latent correlation needs every "
                    "variable to vary", err % p, err / p, types[err % p] ? "a binary variable with one of its two values only"
                    : "no untied pair of samples");
    return GGL_OK;
}

struct MixedBufs {
    DevBuf S;
    DevArr<long long> G;
    DevArr<int> n0, clipped;
    int alloc(int B, int p)
    {
        const size_t n = (size_t)B * p * p;
        HIPCHK(S.alloc(n));
        HIPCHK(G.alloc(n));
        HIPCHK(n0.alloc((size_t)B * p));
        HIPCHK(clipped.alloc(B));
        return GGL_OK;
    }
};
}  // namespace

extern "C" int ggl_mixed_correlation(int device, int p, int N, const int* ranks_host, const int* types, int B, int b,
                                     const int* idx, double clip, double* S_out, long long* G_out, int* n0_out, int* clipped_out)
{
    RCCHK(check_mixed_args(p, N, ranks_host, types, B, b, idx, clip));
    ARGCHK(S_out, "S_out");
    HIPCHK(hipSetDevice(device));
    MixedBufs d;
    RCCHK(d.alloc(B, p));
    RCCHK(mixed_to_device(nullptr, p, N, ranks_host, types, B, b, idx, clip, d.S.p, d.G.p, d.n0.p, d.clipped.p));
    const size_t n = (size_t)B * p * p;
    DOWN(S_out, d.S.p, n);
    if (G_out) HIPCHK(hipMemcpy(G_out, d.G.p, n * sizeof(long long), hipMemcpyDeviceToHost));
    if (n0_out) HIPCHK(hipMemcpy(n0_out, d.n0.p, (size_t)B * p * sizeof(int), hipMemcpyDeviceToHost));
    if (clipped_out) HIPCHK(hipMemcpy(clipped_out, d.clipped.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    return GGL_OK;
}

extern "C" int ggl_set_S_from_mixed(ggl_ctx* c, const int* ranks_host, const int* types, int N, int B, int b, const int* idx,
                                    double clip)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_mixed_args(c->p, N, ranks_host, types, B, b, idx, clip));
    RCCHK(check_divides_K(c, B));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    // as ggl_set_S_from_kendall: the B matrices are built beside the ctx's S; a refused call leaves S alone
    MixedBufs d;
    RCCHK(d.alloc(B, c->p));
    RCCHK(mixed_to_device(c->stream, c->p, N, ranks_host, types, B, b, idx, clip, d.S.p, d.G.p, d.n0.p, d.clipped.p));
    return install_subset_S(c, d.S.p, B);
}

// ---------------------------------------------------------------------------------------------------------------------
// Pairwise-complete covariance of data with missing values, NaN (kernels: covariance_missing.hip).  Every route builds S
// and the pair counts in buffers of its own; the caller's S_out, or the S of a ctx, is written only after the row check, the
// pair-count check and (GGL_COV_SCALE) the variance check have passed: a refused call leaves both as they were.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_min_pairs(int min_pairs, size_t K, size_t p)
{
    if (min_pairs < 1)
        return fail(GGL_E_ARG, "bad argument: min_pairs = %d, every pair of variables needs at least one shared sample (min_pairs >= 1)",
                    min_pairs);
    ARGCHK(K * p * p < ((size_t)1 << 38), "K * p * p too large");
    return GGL_OK;
}

// S_dev, cnt_dev (K,p,p) from the arena on stream st; with GGL_COV_SCALE S is divided by its own diagonal -- the variance of
// each variable over all its observed entries -- and var_dev (K,p) gets it.  what: "instance" or "subset", for the messages.
// Waits for the stream.
int pairwise_of_arena(hipStream_t st, const Arena& a, int p, int flags, int min_pairs, double* S_dev, int* cnt_dev,
                      double* var_dev, const char* what)
{
    DevArr<double> dShift;
    DevArr<int> dRowCnt, dErr;
    DevArr<unsigned long long> dPairErr;
    const int K = a.K;
    const size_t kp = (size_t)K * p, pp = (size_t)p * p;
    HIPCHK(dShift.alloc(kp));
    HIPCHK(dRowCnt.alloc(kp));
    HIPCHK(dErr.alloc(1));
    HIPCHK(dPairErr.alloc(1));
    HIPCHK(hipMemsetAsync(dErr.p, 0x7f, sizeof(int), st));
    launch_row_stats_masked(st, a.X.p, a.off.p, a.N.p, dShift.p, dRowCnt.p, dErr.p, K, p);
    HIPCHK(hipGetLastError());
    int err;
    RCCHK(read_err_word(st, dErr.p, &err));
    if (err != GGL_DIAG_OK)
        return fail(GGL_E_ARG, "bad argument: %s %d, variable %d has no observed entry (every sample is NaN)", what, err / p, err % p);
    launch_gram_nt_pairwise(st, a.X.p, a.off.p, a.N.p, (flags & GGL_COV_CENTER) ? dShift.p : nullptr, S_dev, cnt_dev, K, p,
                            cov_tile(flags));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(dPairErr.p, 0xff, sizeof(unsigned long long), st));
    launch_pair_count_check(st, cnt_dev, min_pairs, dPairErr.p, K, p);
    HIPCHK(hipGetLastError());
    unsigned long long perr;
    RCCHK(read_err_word64(st, dPairErr.p, &perr));
    if (perr != ~0ull) {
        int n = 0;
        HIPCHK(hipMemcpy(&n, cnt_dev + perr, sizeof(int), hipMemcpyDeviceToHost));
        return fail(GGL_E_ARG, "bad argument: %s %d, the pair of variables (%d, %d) shares %d samples, min_pairs = %d", what,
                    (int)(perr / pp), (int)(perr % pp / p), (int)(perr % p), n, min_pairs);
    }
    if (flags & GGL_COV_SCALE) RCCHK(scale_in_place(st, K, p, S_dev, var_dev, "the variance"));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}

// ... from the host data of K instances
int pairwise_to_device(hipStream_t st, int K, int p, const int* N, const double* const* X_host, int flags, int min_pairs,
                       double* S_dev, int* cnt_dev, double* var_dev)
{
    Arena a;
    RCCHK(a.from_instances(st, K, p, N, X_host));
    return pairwise_of_arena(st, a, p, flags, min_pairs, S_dev, cnt_dev, var_dev, "instance");
}

// ... of B column subsets of one X
int pairwise_subsets_to_device(hipStream_t st, int p, int N, const double* X_host, int B, int b, const int* idx, int flags,
                               int min_pairs, double* S_dev, int* cnt_dev, double* var_dev)
{
    Arena a;
    RCCHK(a.from_subsets(st, p, N, X_host, B, b, idx));
    return pairwise_of_arena(st, a, p, flags, min_pairs, S_dev, cnt_dev, var_dev, "subset");
}
}  // namespace

extern "C" int ggl_covariance_pairwise(int device, int K, int p, const int* N, const double* const* X_host, int flags,
                                       int min_pairs, double* S_out, double* scale_out, int* counts_out)
{
    RCCHK(check_data_args(K, p, N, X_host, flags));
    RCCHK(check_min_pairs(min_pairs, K, p));
    CovOut d;
    RCCHK(d.begin(device, K, p, flags, S_out, scale_out, true, false));
    RCCHK(pairwise_to_device(nullptr, K, p, N, X_host, flags, min_pairs, d.S.p, d.cnt.p, d.var.p));
    return d.down(flags, S_out, scale_out, counts_out);
}

extern "C" int ggl_covariance_pairwise_subsets(int device, int p, int N, const double* X_host, int B, int b, const int* idx,
                                               int flags, int min_pairs, double* S_out, double* scale_out, int* counts_out)
{
    RCCHK(check_subset_args(p, N, X_host, B, b, idx, flags));
    RCCHK(check_min_pairs(min_pairs, B, p));
    CovOut d;
    RCCHK(d.begin(device, B, p, flags, S_out, scale_out, true, false));
    RCCHK(pairwise_subsets_to_device(nullptr, p, N, X_host, B, b, idx, flags, min_pairs, d.S.p, d.cnt.p, d.var.p));
    return d.down(flags, S_out, scale_out, counts_out);
}

extern "C" int ggl_set_S_from_data_pairwise(ggl_ctx* c, const double* const* X_host, const int* N, int flags, int min_pairs)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_data_args(c->K, c->p, N, X_host, flags));
    RCCHK(check_min_pairs(min_pairs, c->K, c->p));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    // unlike ggl_set_S_from_data the K matrices are built beside the ctx's S: a refused call leaves the ctx as it was
    DevBuf dS, dVar;
    DevArr<int> dCnt;
    HIPCHK(dS.alloc(c->n));
    HIPCHK(dVar.alloc((size_t)c->K * c->p));
    HIPCHK(dCnt.alloc(c->n));
    RCCHK(pairwise_to_device(c->stream, c->K, c->p, N, X_host, flags, min_pairs, dS.p, dCnt.p, dVar.p));
    return install_subset_S(c, dS.p, c->K, dVar.p, flags);
}

extern "C" int ggl_set_S_from_subsets_pairwise(ggl_ctx* c, const double* X_host, int N, int B, int b, const int* idx, int flags,
                                               int min_pairs)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_subset_args(c->p, N, X_host, B, b, idx, flags));
    RCCHK(check_min_pairs(min_pairs, B, c->p));
    RCCHK(check_divides_K(c, B));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    const size_t n = (size_t)B * c->p * c->p;
    DevBuf dS, dVar;
    DevArr<int> dCnt;
    HIPCHK(dS.alloc(n));
    HIPCHK(dVar.alloc((size_t)B * c->p));
    HIPCHK(dCnt.alloc(n));
    RCCHK(pairwise_subsets_to_device(c->stream, c->p, N, X_host, B, b, idx, flags, min_pairs, dS.p, dCnt.p, dVar.p));
    return install_subset_S(c, dS.p, B, dVar.p, flags);
}

// ---------------------------------------------------------------------------------------------------------------------
// Weighted covariance of ONE data array under K weight rows (kernels: covariance_weighted.hip): X and the weights go up
// once, every instance reads the same X.  Every route builds S in a buffer of its own; the caller's S_out, or the S of a ctx,
// is written only after the weight check and (GGL_COV_SCALE) the variance check have passed.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_weighted_args(int p, int N, const double* X_host, int K, const double* w_host, int flags)
{
    ARGCHK(p >= 1 && N >= 1, "p >= 1, N >= 1");
    if (K < 1 || K > 65535) return fail(GGL_E_ARG, "bad argument: K = %d weight rows, 1 .. 65535 are possible", K);
    ARGCHK(X_host && w_host, "X, w");
    RCCHK(check_cov_flags(flags, WCOV_FLAGS));
    ARGCHK((size_t)K * p < (size_t)GGL_DIAG_OK, "K * p too large");
    return GGL_OK;
}

// S_dev (K,p,p), var_dev (K,p) with GGL_COV_SCALE and wsum_dev (K) on stream st; the arguments have been checked.  Waits for
// the stream: the tables go away behind it.  tc: the ctx whose event timeline (ggl_trace_start) takes the marks 30 / 31 in front
// of and behind the Gram launch, or null.
int weighted_to_device(hipStream_t st, int p, int N, const double* X_host, int K, const double* w_host, int flags, double* S_dev,
                       double* var_dev, double* wsum_dev, ggl_ctx* tc = nullptr)
{
    DevArr<double> dX, dW, dR, dMean;
    DevArr<int> dRng;
    DevArr<unsigned long long> dWErr;
    const size_t kn = (size_t)K * N;
    HIPCHK(dX.alloc((size_t)p * N));
    HIPCHK(dW.alloc(kn));
    HIPCHK(dR.alloc(kn));
    HIPCHK(dRng.alloc(2 * (size_t)K));
    HIPCHK(dWErr.alloc(1));
    HIPCHK(hipMemcpyAsync(dX.p, X_host, (size_t)p * N * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dW.p, w_host, kn * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dWErr.p, 0xff, sizeof(unsigned long long), st));
    launch_weight_prepare(st, dW.p, dR.p, wsum_dev, dRng.p, dWErr.p, K, N, (flags & GGL_COV_FULL_RANGE) != 0);
    HIPCHK(hipGetLastError());
    unsigned long long werr;
    RCCHK(read_err_word64(st, dWErr.p, &werr));
    if (werr != ~0ull) {
        if (werr < kn)
            return fail(GGL_E_ARG, "bad argument: instance %d, sample %d holds the weight %g; weights must be non-negative and finite",
                        (int)(werr / N), (int)(werr % N), w_host[werr]);
        const int k = (int)(werr - kn);
        double W = 0.0;
        HIPCHK(hipMemcpy(&W, wsum_dev + k, sizeof(double), hipMemcpyDeviceToHost));
        return fail(GGL_E_ARG, "bad argument: the weights of instance %d sum to %g; every weight row needs a positive finite sum", k, W);
    }
    const bool center = (flags & GGL_COV_CENTER) != 0;
    if (center) {
        HIPCHK(dMean.alloc((size_t)K * p));
        launch_row_means_weighted(st, dX.p, dW.p, wsum_dev, dRng.p, dMean.p, K, p, N);
        HIPCHK(hipGetLastError());
    }
    if (tc) trace_mark(tc, st, 30);
    launch_gram_nt_weighted(st, dX.p, dR.p, wsum_dev, dRng.p, center ? dMean.p : nullptr, S_dev, K, p, N, cov_tile(flags));
    HIPCHK(hipGetLastError());
    if (tc) trace_mark(tc, st, 31);
    if (flags & GGL_COV_SCALE) RCCHK(scale_in_place(st, K, p, S_dev, var_dev, "the weighted variance"));
    HIPCHK(hipStreamSynchronize(st));
    return GGL_OK;
}
}  // namespace

extern "C" int ggl_covariance_weighted(int device, int p, int N, const double* X_host, int K, const double* w_host, int flags,
                                       double* S_out, double* scale_out, double* wsum_out)
{
    RCCHK(check_weighted_args(p, N, X_host, K, w_host, flags));
    CovOut d;
    RCCHK(d.begin(device, K, p, flags, S_out, scale_out, false, true));
    RCCHK(weighted_to_device(nullptr, p, N, X_host, K, w_host, flags, d.S.p, d.var.p, d.wsum.p));
    return d.down(flags, S_out, scale_out, nullptr, wsum_out);
}

extern "C" int ggl_set_S_from_weighted(ggl_ctx* c, const double* X_host, int N, const double* w_host, int flags)
{
    RCCHK(check_ctx_takes_S(c));
    RCCHK(check_weighted_args(c->p, N, X_host, c->K, w_host, flags));
    HIPCHK(hipSetDevice(c->device));
    DROP_PRE(c);
    // as ggl_set_S_from_subsets: the K matrices are built beside the ctx's S; a refused call (a bad weight, a constant variable
    // under GGL_COV_SCALE) leaves S, its variances and what was built for them as they were
    DevBuf dS, dVar, dWsum;
    HIPCHK(dS.alloc(c->n));
    HIPCHK(dVar.alloc((size_t)c->K * c->p));
    HIPCHK(dWsum.alloc(c->K));
    RCCHK(weighted_to_device(c->stream, c->p, N, X_host, c->K, w_host, flags, dS.p, dVar.p, dWsum.p, c));
    return install_subset_S(c, dS.p, c->K, dVar.p, flags);
}

// ---------------------------------------------------------------------------------------------------------------------
// Gaussian predictive scores under weighted means and covariances: row r of w scores column target[r] of X.  The
// covariances are those of ggl_covariance_weighted -- the same three launches per chunk of rows -- and never leave the device:
// k_predict_rhs forms d = x_target - m_r from the means, k_chol_predict (cholesky.hip) factors S_r in place and leaves
// { log det, d^T S^-1 d, smallest pivot, status }.  X goes up once.  Here beside the weighted covariance because it shares its
// argument checks and its launch sequence.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t PREDICT_CHUNK_BYTES = (size_t)256 << 20;   // chunk = 0: the covariance stack of a chunk takes at most this
}

extern "C" int ggl_weighted_predictive_scores(int device, int p, int N, const double* X_host, int M, const double* w_host,
                                              const int* target, double ridge, int flags, int chunk, double* out)
{
    ARGCHK(M >= 1, "M >= 1");
    RCCHK(check_weighted_args(p, N, X_host, std::min(M, 65535), w_host, flags));
    ARGCHK(!(flags & GGL_COV_SCALE), "flags: GGL_COV_SCALE has no meaning for a predictive score");
    ARGCHK(target && out, "target and out must not be NULL");
    ARGCHK(ridge >= 0.0 && std::isfinite(ridge), "ridge must be non-negative and finite");
    ARGCHK(chunk >= 0, "chunk >= 0 (0: sized from the memory budget)");
    for (int r = 0; r < M; ++r)
        if (target[r] < 0 || target[r] >= N)
            return fail(GGL_E_ARG, "bad argument: row %d scores the sample %d, outside [0, %d)", r, target[r], N);
    // what k_weight_prepare would find, found here: a refused call does no device work
    for (int r = 0; r < M; ++r) {
        const double* wr = w_host + (size_t)r * N;
        bool any = false;
        for (int n = 0; n < N; ++n) {
            if (!(wr[n] >= 0.0) || !std::isfinite(wr[n]))
                return fail(GGL_E_ARG, "bad argument: instance %d, sample %d holds the weight %g; weights must be non-negative and finite",
                            r, n, wr[n]);
            any = any || wr[n] > 0.0;
        }
        if (!any)
            return fail(GGL_E_ARG, "bad argument: the weights of instance %d sum to %g; every weight row needs a positive finite sum",
                        r, 0.0);
    }
    const size_t pp = (size_t)p * p;
    int C = chunk;
    if (C == 0) C = (int)std::max<size_t>(1, std::min<size_t>(PREDICT_CHUNK_BYTES / (pp * sizeof(double)), 65535));
    C = std::min(std::min(C, M), 65535);
    ARGCHK((size_t)C * p < (size_t)GGL_DIAG_OK, "chunk * p too large");

    HIPCHK(hipSetDevice(device));
    hipStream_t st = nullptr;
    DevArr<double> dX, dW, dR, dWsum, dMean, dD, dS, dOut;
    DevArr<int> dRng, dTarget;
    DevArr<unsigned long long> dWErr;
    HIPCHK(dX.alloc((size_t)p * N));
    HIPCHK(dW.alloc((size_t)C * N));
    HIPCHK(dR.alloc((size_t)C * N));
    HIPCHK(dWsum.alloc(C));
    HIPCHK(dMean.alloc((size_t)C * p));
    HIPCHK(dD.alloc((size_t)C * p));
    HIPCHK(dS.alloc((size_t)C * pp));
    HIPCHK(dOut.alloc((size_t)M * 4));
    HIPCHK(dRng.alloc(2 * (size_t)C));
    HIPCHK(dTarget.alloc(M));
    HIPCHK(dWErr.alloc(1));
    HIPCHK(hipMemcpyAsync(dX.p, X_host, (size_t)p * N * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dTarget.p, target, (size_t)M * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dWErr.p, 0xff, sizeof(unsigned long long), st));
    const bool center = (flags & GGL_COV_CENTER) != 0;
    // the tile shape of ONE call on all M rows, whatever the chunk: out does not depend on chunk by construction
    const int tile = gram_tile(std::min(M, 65535), p, cov_tile(flags));
    for (int r0 = 0; r0 < M; r0 += C) {
        const int c = std::min(C, M - r0);
        HIPCHK(hipMemcpyAsync(dW.p, w_host + (size_t)r0 * N, (size_t)c * N * sizeof(double), hipMemcpyHostToDevice, st));
        launch_weight_prepare(st, dW.p, dR.p, dWsum.p, dRng.p, dWErr.p, c, N, (flags & GGL_COV_FULL_RANGE) != 0);
        if (center) launch_row_means_weighted(st, dX.p, dW.p, dWsum.p, dRng.p, dMean.p, c, p, N);
        launch_gram_nt_weighted(st, dX.p, dR.p, dWsum.p, dRng.p, center ? dMean.p : nullptr, dS.p, c, p, N, tile);
        launch_predict_rhs(st, dX.p, center ? dMean.p : nullptr, dTarget.p + r0, dD.p, c, p, N);
        launch_chol_predict(st, dS.p, dD.p, ridge, dOut.p + (size_t)r0 * 4, c, p);
        HIPCHK(hipGetLastError());
    }
    // a weight sum that overflowed is all the host check above leaves to the device's error word
    unsigned long long werr;
    RCCHK(read_err_word64(st, dWErr.p, &werr));
    if (werr != ~0ull)
        return fail(GGL_E_ARG, "bad argument: the weights of a row do not have a positive finite sum; every weight row needs one");
    DOWN(out, dOut.p, (size_t)M * 4);
    return GGL_OK;
}
