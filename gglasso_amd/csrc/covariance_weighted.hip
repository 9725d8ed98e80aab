// Weighted covariance of ONE data array under K weight rows, on the device -- the kernel-smoothed covariance stack of a
// time series (Zhou, Lafferty, Wasserman 2010; Monti et al. 2014), observation weights, EM responsibilities:
//
//     W_k      = sum_n w[k,n]                                              k_weight_prepare   (+ r = sqrt(w), the support)
//     m[k,i]   = (1/W_k) sum_n w[k,n] X[i,n]                               k_row_means_weighted
//     S_k      = (1/W_k) sum_n w[k,n] (x_n - m_k)(x_n - m_k)^T             k_gram_nt_weighted (numpy.cov(X, aweights=w_k, bias=True))
//
// X is (p, N) row-major, variables in rows, and is shared by all K instances: there is no per-instance copy of the data and
// no offset table.  k_gram_nt_weighted is the sibling of k_gram_nt (covariance.hip): same tiles, same LDS image
// [variable][sample] with row length BK + 2, tile pairs I <= J only with the mirror stored from the same accumulator.  It
// stages r[k,n] (x_in - m[k,i]) for BOTH operands, so a diagonal tile still has one operand and S_k is a true Gram matrix
// (positive semidefinite up to rounding, bitwise symmetric).
//
// Range rule.  Instance k loops over the samples [lo_k & ~63, hi_k) only, [lo_k, hi_k) being the support of its weights:
// with kernel weights of bandwidth h the work is proportional to the support, not to N.  The start is a multiple of 64, so
// the slabs (BK = 16 or 32 samples) are slabs of the loop over [0, N) and a lane of the means kernel owns the same samples
// n = lane (mod 64) either way.  What the full loop stages outside the support is r (x - m) = +-0, which leaves an
// accumulator that starts at +0 as it is: on finite data the result has the bits of the loop over [0, N)
// (GGL_COV_FULL_RANGE).  Inside the range nothing is skipped, whatever the weights are.
#include <cfloat>

#include "common.hpp"
#include "kernels.hpp"
#include "sym_tile.hpp"

namespace ggl {

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// One wave per weight row: W_k in the order of k_row_means (lane sums over n = lane, lane + 64, ..., then the xor tree), the
// table r = sqrt(w), the support rng[2k], rng[2k+1] = [lo, hi) (full: [0, N)), and the error word (every byte 0xff from the
// caller: none): the smallest k * N + n of a negative or non-finite weight, else K * N + k of a row whose sum is zero or not
// finite.  No floating-point atomics.
__global__ __launch_bounds__(64) void k_weight_prepare(const double* __restrict__ w, double* __restrict__ r,
                                                       double* __restrict__ wsum, int* __restrict__ rng,
                                                       unsigned long long* __restrict__ err, int K, int N, int full)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const double* wk = w + (size_t)k * N;
    double* rk = r + (size_t)k * N;
    double s = 0.0;
    int lo = N, hi = 0;
    unsigned long long bad = ~0ull;
    for (int n = lane; n < N; n += 64) {
        const double v = wk[n];
        if ((!(v >= 0.0) || !(v <= DBL_MAX)) && bad == ~0ull) bad = (unsigned long long)k * N + n;
        s += v;
        rk[n] = sqrt(v);
        if (v > 0.0) {
            lo = min(lo, n);
            hi = n + 1;
        }
    }
    s = wave_sum(s);
    lo = wave_min_i(lo);
    hi = wave_max_i(hi);
    if (bad != ~0ull) atomicMin(err, bad);
    if (lane == 0) {
        if (!(s > 0.0) || !(s <= DBL_MAX)) atomicMin(err, (unsigned long long)K * N + k);
        wsum[k] = s;
        rng[2 * k] = full ? 0 : lo;
        rng[2 * k + 1] = full ? N : hi;
    }
}

// One wave per (k, row): every lane sums w x over its samples n = lane (mod 64) of the range in order, then the xor tree.
// The range starts at a multiple of 64, so the order is fixed by (lane, support) and agrees with the loop over [0, N) up to
// terms that are +-0.
__global__ __launch_bounds__(256) void k_row_means_weighted(const double* __restrict__ X, const double* __restrict__ w,
                                                            const double* __restrict__ wsum, const int* __restrict__ rng,
                                                            double* __restrict__ mean, int p, int N)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p) return;
    const int n_lo = rng[2 * k] & ~63, n_hi = rng[2 * k + 1];
    const double* x = X + (size_t)row * N;
    const double* wk = w + (size_t)k * N;
    double s = 0.0;
    for (int n = n_lo + lane; n < n_hi; n += 64) s += wk[n] * x[n];
    s = wave_sum(s);
    if (lane == 0) mean[(size_t)k * p + row] = s / wsum[k];
}

// LDS image, fragment reads and tile decoding as k_gram_nt (covariance.hip); X is the one (p, N) array of all instances
template <int BM, int BK, int WM, int WN>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gram_nt_weighted(const double* __restrict__ X,
                                                                           const double* __restrict__ r,
                                                                           const double* __restrict__ wsum,
                                                                           const int* __restrict__ rng,
                                                                           const double* __restrict__ mean,
                                                                           double* __restrict__ S, int K, int p, int N)
{
    using Cfg = SymCfg<BM, BK, WM, WN, false>;
    constexpr int XLD = BK + 2, SLAB = BM * XLD;
    constexpr int RSTEP = Cfg::NT / BK;
    static_assert(Cfg::NT % BK == 0, "a row of the slab must be covered by whole thread rows");
    static_assert(64 % BK == 0, "a range that starts at a multiple of 64 must start at a slab of the full loop");
    __shared__ __attribute__((aligned(16))) double smem[2 * SLAB];
    const int T = (p + BM - 1) / BM;
    int k, b;
    if (!decode_block_xcd(T * (T + 1) / 2, K, k, b)) return;
    int I = 0;
    while (b >= T - I) { b -= T - I; ++I; }
    const int J = I + b;
    const bool diag = (I == J);
    const int I0 = I * BM, J0 = J * BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave / Cfg::NWC) * WM, wc = (wave % Cfg::NWC) * WN;
    const int n_lo = rng[2 * k] & ~63, n_hi = rng[2 * k + 1];
    const double* rk = r + (size_t)k * N;
    double* As = smem;
    double* Bs = diag ? smem : smem + SLAB;       // a diagonal tile has one operand

    v4d acc[Cfg::TI][Cfg::TJ];
#pragma unroll
    for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    // slab element (row lrow + q * RSTEP, sample lcol): consecutive lanes read consecutive samples of one row
    const int lcol = tid % BK, lrow = tid / BK;
    const double *pa[Cfg::LPT], *pb[Cfg::LPT];
    double ma[Cfg::LPT], mb[Cfg::LPT];
    bool oka[Cfg::LPT], okb[Cfg::LPT];
#pragma unroll
    for (int q = 0; q < Cfg::LPT; ++q) {
        const int rw = lrow + q * RSTEP;
        oka[q] = (I0 + rw) < p;
        okb[q] = (J0 + rw) < p;
        const int ia = min(I0 + rw, p - 1), ib = min(J0 + rw, p - 1);    // clamped: always a valid row
        pa[q] = X + (size_t)ia * N;
        pb[q] = X + (size_t)ib * N;
        ma[q] = mean ? mean[(size_t)k * p + ia] : 0.0;
        mb[q] = mean ? mean[(size_t)k * p + ib] : 0.0;
    }
    double ra[Cfg::LPT], rb[Cfg::LPT], rw_n;
    auto fetch = [&](int n0) {
        const int n = min(n0 + lcol, N - 1);                             // clamped: past the end is never staged as data
        rw_n = rk[n];
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            ra[q] = pa[q][n];
            if (!diag) rb[q] = pb[q][n];
        }
    };
    // Centring and weighting happen here, and the zero padding AFTER them: a sample index >= hi_k or a row >= p contributes
    // 0 to every product.
    auto stage = [&](int n0) {
        const bool in = (n0 + lcol) < n_hi;
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            const int rw = lrow + q * RSTEP;
            As[rw * XLD + lcol] = (in && oka[q]) ? rw_n * (ra[q] - ma[q]) : 0.0;
            if (!diag) Bs[rw * XLD + lcol] = (in && okb[q]) ? rw_n * (rb[q] - mb[q]) : 0.0;
        }
    };
    auto compute = [&](int nq) {
        double af[BK / 4][Cfg::TI], bf[BK / 4][Cfg::TJ];
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk >= nq) break;
            const int c = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i) af[kk][i] = As[(wr + i * 16 + (lane & 15)) * XLD + c];
#pragma unroll
            for (int j = 0; j < Cfg::TJ; ++j) bf[kk][j] = Bs[(wc + j * 16 + (lane & 15)) * XLD + c];
        }
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk >= nq) break;
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
                for (int j = 0; j < Cfg::TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
        }
    };

    // a wave whose sub-tile of a diagonal tile lies below the diagonal produces nothing that is kept
    const bool dead_wave = diag && (wr >= wc + WN);
    fetch(n_lo);
    for (int n0 = n_lo; n0 < n_hi; n0 += BK) {
        stage(n0);
        __syncthreads();
        fetch(n0 + BK);                                                   // past the end: clamped, never staged
        if (!dead_wave) compute(min(BK / 4, (n_hi - n0 + 3) / 4));
        __syncthreads();
    }

    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* Sk = S + (size_t)k * p * p;
    const double dn = wsum[k];
#pragma unroll
    for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < Cfg::TJ; ++tj)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * q;
                const int gj = J0 + wc + tj * 16 + (lane & 15);
                if (gi < p && gj < p && (!diag || gi <= gj)) {
                    const double v = acc[ti][tj][q] / dn;
                    Sk[(size_t)gi * p + gj] = v;
                    if (gi != gj) Sk[(size_t)gj * p + gi] = v;
                }
            }
}

void launch_weight_prepare(hipStream_t st, const double* w, double* r, double* wsum, int* rng, unsigned long long* err, int K,
                           int N, bool full)
{
    hipLaunchKernelGGL(k_weight_prepare, dim3(K), dim3(64), 0, st, w, r, wsum, rng, err, K, N, full ? 1 : 0);
}

void launch_row_means_weighted(hipStream_t st, const double* X, const double* w, const double* wsum, const int* rng,
                               double* mean, int K, int p, int N)
{
    hipLaunchKernelGGL(k_row_means_weighted, dim3((p + 3) / 4, K), dim3(256), 0, st, X, w, wsum, rng, mean, p, N);
}

void launch_gram_nt_weighted(hipStream_t st, const double* X, const double* r, const double* wsum, const int* rng,
                             const double* mean, double* S, int K, int p, int N, int tile)
{
    if (gram_tile(K, p, tile) == 64) {
        const int T = (p + 63) / 64;
        hipLaunchKernelGGL((k_gram_nt_weighted<64, 16, 32, 32>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(256), 0, st, X, r,
                           wsum, rng, mean, S, K, p, N);
    } else {
        const int T = (p + 31) / 32;
        hipLaunchKernelGGL((k_gram_nt_weighted<32, 32, 16, 16>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(256), 0, st, X, r,
                           wsum, rng, mean, S, K, p, N);
    }
}

}  // namespace ggl
