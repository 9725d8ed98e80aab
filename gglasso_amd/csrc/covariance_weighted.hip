// Weighted covariance of ONE data array under K weight rows, on the device -- the kernel-smoothed covariance stack of a
// time series (Zhou, Lafferty, Wasserman 2010; Monti et al. 2014), observation weights, EM responsibilities:
//
//     W_k      = sum_n w[k,n]                                              k_weight_prepare   (+ r = sqrt(w), the support)
//     m[k,i]   = (1/W_k) sum_n w[k,n] X[i,n]                               k_row_means_weighted
//     S_k      = (1/W_k) sum_n w[k,n] (x_n - m_k)(x_n - m_k)^T             k_gram_nt_weighted (numpy.cov(X, aweights=w_k, bias=True))
//
// X is (p, N) row-major, variables in rows, and is shared by all K instances: there is no per-instance copy of the data and
// no offset table.  k_gram_nt_weighted is the tile body of k_gram_nt (gram_nt_tile.hpp) under the policy GramWeighted: same
// tiles, same LDS image [variable][sample] with row length BK + 2, tile pairs I <= J only with the mirror stored from the same
// accumulator.  It stages r[k,n] (x_in - m[k,i]) for BOTH operands, so a diagonal tile still has one operand and S_k is a true
// Gram matrix (positive semidefinite up to rounding, bitwise symmetric).
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
#include "gram_nt_tile.hpp"

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

// Op of gram_nt_tile: X is the one (p, N) array of all instances, the samples [lo_k & ~63, hi_k) are looped, one plane
// r (x - m) with r[k,n] fetched beside the slab, one accumulator set, S = acc / W_k
struct GramWeighted {
    static constexpr int PLANES = 1, NACC = 1;
    static constexpr bool PRELOAD = true;
    const double* X;
    const double* r;
    const double* wsum;
    const int* rng;
    const double* mean;
    double* S;
    int N;
    const double* rk;
    double rw_n, dn;
    int n_lo, n_hi, n_last;
    __device__ __forceinline__ void instance(int k, int)
    {
        n_lo = rng[2 * k] & ~63;
        n_hi = rng[2 * k + 1];
        n_last = N - 1;
        rk = r + (size_t)k * N;
        dn = wsum[k];
    }
    __device__ __forceinline__ const double* row(int i) const { return X + (size_t)i * N; }
    __device__ __forceinline__ double shift(int k, int p, int i) const { return mean ? mean[(size_t)k * p + i] : 0.0; }
    __device__ __forceinline__ void fetch(int n) { rw_n = rk[n]; }
    __device__ __forceinline__ void stage(bool on, double x, double m, double (&v)[1]) const { v[0] = on ? rw_n * (x - m) : 0.0; }
    __device__ __forceinline__ void mma(const double (&a)[1], const double (&b)[1], v4d (&acc)[1]) const
    {
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc[0], 0, 0, 0);
    }
    __device__ __forceinline__ double value(const v4d (&acc)[1], int q) const { return acc[0][q] / dn; }
    __device__ __forceinline__ void store(double v, size_t e) const { S[e] = v; }
};

template <int BM, int BK, int WM, int WN>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gram_nt_weighted(const double* __restrict__ X,
                                                                           const double* __restrict__ r,
                                                                           const double* __restrict__ wsum,
                                                                           const int* __restrict__ rng,
                                                                           const double* __restrict__ mean,
                                                                           double* __restrict__ S, int K, int p, int N)
{
    GramWeighted op{X, r, wsum, rng, mean, S, N};
    gram_nt_tile<BM, BK, WM, WN>(op, K, p);
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
    gram_dispatch(K, p, tile, [&](auto s, dim3 grid, dim3 block) {
        using Sh = decltype(s);
        hipLaunchKernelGGL((k_gram_nt_weighted<Sh::BM, Sh::BK, Sh::WM, Sh::WN>), grid, block, 0, st, X, r, wsum, rng, mean, S, K,
                           p, N);
    });
}

}  // namespace ggl
