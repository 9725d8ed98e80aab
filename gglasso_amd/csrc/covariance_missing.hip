// Pairwise-complete sample covariance of observations with missing values (NaN) on the device -- what R's
// cov(use = "pairwise.complete.obs") and pandas' DataFrame.cov() compute, with the project's 1/n normalisation:
//
//     O_ij  = { n : x_in and x_jn are both observed },  n_ij = |O_ij|
//     S_ij  = (1/n_ij) sum_{O_ij} (x_in - m_i|j)(x_jn - m_j|i),   m_i|j = the mean of x_i over O_ij
//
// With y_in = x_in - c_i where observed and 0 where missing (c_i: any shift, here the mean of the observed entries of row i,
// k_row_stats_masked) and w_in = 1 where observed, 0 where missing, four Gram products hold everything:
//
//     P = Y Y^T,  A = Y W^T,  B = W Y^T,  C = W W^T          C_ij = n_ij (exact in fp64),  m_i|j - c_i = A_ij / C_ij
//     S_ij = (P_ij - A_ij B_ij / C_ij) / C_ij                center = false: Y = x (0 where missing), S_ij = P_ij / C_ij
//
// k_gram_nt_pairwise is the tile body of k_gram_nt (gram_nt_tile.hpp) under the policy GramPairwise: a mask plane beside
// every data plane and four accumulator sets, the same tile pairs I <= J, the same XCD decode, the mirror stored from the same
// evaluation (S and the counts are bitwise symmetric).  The mask is staged on its own -- an observed entry equal to its row
// mean has y = 0 -- and a padded position (sample >= N_k or row >= p, fetched clamped and possibly NaN) gets y = w = 0 by the
// index test alone.
#include "common.hpp"
#include "kernels.hpp"
#include "gram_nt_tile.hpp"

namespace ggl {

// One wave per row, lane order of k_row_means: every lane sums and counts its observed elements n = lane, lane + 64, ... in
// order, then the xor tree.  cnt[k,i] observed entries and their mean c[k,i]; a row without any: *err = smallest k * p + i
// (set to GGL_DIAG_OK by the caller) and c = 0.
__global__ __launch_bounds__(256) void k_row_stats_masked(const double* __restrict__ X, const long long* __restrict__ off,
                                                          const int* __restrict__ Ntab, double* __restrict__ c,
                                                          int* __restrict__ cnt, int* __restrict__ err, int p)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p) return;
    const int Nk = Ntab[k];
    const double* x = X + off[k] + (size_t)row * Nk;
    double s = 0.0, m = 0.0;
    for (int n = lane; n < Nk; n += 64) {
        const double v = x[n];
        if (v == v) { s += v; m += 1.0; }
    }
    s = wave_sum(s);
    m = wave_sum(m);                                                      // (an integer below 2^31: exact)
    if (lane == 0) {
        const size_t ki = (size_t)k * p + row;
        cnt[ki] = (int)m;
        c[ki] = m > 0.0 ? s / m : 0.0;
        if (!(m > 0.0)) atomicMin(err, (int)ki);
    }
}

// Op of gram_nt_tile: the planes Y and W, the accumulator sets P, A, B, C (without centring P, C: A and B are not needed),
// fragments read per k-step -- four fragment reads, four products per 16 x 16 block and k-step.
template <bool CENTER>
struct GramPairwise : GramArena {
    static constexpr int PLANES = 2, NACC = CENTER ? 4 : 2;
    static constexpr bool PRELOAD = false;
    const double* shift_tab;
    double* S;
    int* counts;
    struct Out { double v; int n; };
    __device__ __forceinline__ double shift(int k, int p, int i) const { return CENTER ? shift_tab[(size_t)k * p + i] : 0.0; }
    // A position is data only by its INDEX (on); only then does the value decide between observed and missing.
    __device__ __forceinline__ void stage(bool on, double x, double m, double (&v)[2]) const
    {
        const bool o = on && (x == x);
        v[0] = o ? x - m : 0.0;
        v[1] = o ? 1.0 : 0.0;
    }
    __device__ __forceinline__ void mma(const double (&a)[2], const double (&b)[2], v4d (&acc)[NACC]) const
    {
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc[0], 0, 0, 0);
        if (CENTER) {
            acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[1], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[0], acc[2], 0, 0, 0);
        }
        acc[NACC - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], acc[NACC - 1], 0, 0, 0);
    }
    // n_ij = 0 leaves a NaN for k_pair_count_check to refuse
    __device__ __forceinline__ Out value(const v4d (&acc)[NACC], int r) const
    {
        const double n = acc[NACC - 1][r];
        const double v = CENTER ? (acc[0][r] - acc[1][r] * acc[NACC - 2][r] / n) / n : acc[0][r] / n;
        return {v, (int)n};
    }
    __device__ __forceinline__ void store(Out o, size_t e) const
    {
        S[e] = o.v;
        counts[e] = o.n;
    }
};

template <int BM, int BK, int WM, int WN, bool CENTER>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gram_nt_pairwise(const double* __restrict__ X,
                                                                           const long long* __restrict__ off,
                                                                           const int* __restrict__ Ntab,
                                                                           const double* __restrict__ shift,
                                                                           double* __restrict__ S, int* __restrict__ counts,
                                                                           int K, int p)
{
    gram_nt_tile<BM, BK, WM, WN>(GramPairwise<CENTER>{{X, off, Ntab}, shift, S, counts}, K, p);
}

// *err (every byte 0xff from the caller: none) = smallest (k * p + i) * p + j with n_ij < min_pairs
__global__ __launch_bounds__(256) void k_pair_count_check(const int* __restrict__ counts, size_t total, int min_pairs,
                                                          unsigned long long* __restrict__ err)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total && counts[e] < min_pairs) atomicMin(err, (unsigned long long)e);
}

void launch_row_stats_masked(hipStream_t st, const double* X, const long long* off, const int* N, double* c, int* cnt, int* err,
                             int K, int p)
{
    hipLaunchKernelGGL(k_row_stats_masked, dim3((p + 3) / 4, K), dim3(256), 0, st, X, off, N, c, cnt, err, p);
}

void launch_gram_nt_pairwise(hipStream_t st, const double* X, const long long* off, const int* N, const double* shift, double* S,
                             int* counts, int K, int p, int tile)
{
    gram_dispatch(K, p, tile, [&](auto s, dim3 grid, dim3 block) {
        using Sh = decltype(s);
        if (shift)
            hipLaunchKernelGGL((k_gram_nt_pairwise<Sh::BM, Sh::BK, Sh::WM, Sh::WN, true>), grid, block, 0, st, X, off, N, shift, S,
                               counts, K, p);
        else
            hipLaunchKernelGGL((k_gram_nt_pairwise<Sh::BM, Sh::BK, Sh::WM, Sh::WN, false>), grid, block, 0, st, X, off, N, shift,
                               S, counts, K, p);
    });
}

void launch_pair_count_check(hipStream_t st, const int* counts, int min_pairs, unsigned long long* err, int K, int p)
{
    const size_t total = (size_t)K * p * p;
    hipLaunchKernelGGL(k_pair_count_check, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts, total, min_pairs, err);
}

}  // namespace ggl
