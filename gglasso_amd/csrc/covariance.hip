// Sample covariance from observations, and scaling by a diagonal, on the device (the input side of every solver):
//
//     m[k,i]   = (1/N_k) sum_n X_k[i,n]                                   k_row_means
//     S_k      = (1/N_k) Xc Xc^T,  Xc[i,n] = X_k[i,n] - m[k,i]            k_gram_nt      (numpy.cov(X_k, bias=True))
//     Y[k,i,j] = X[k,i,j] / (sqrt(d[k,i]) * sqrt(d[k,j]))                  k_scale_by_diag (helper/basic_linalg.py:46-65)
//
// X_k is (p, N_k) row-major, variables in rows.  The Gram product is the shared tile body gram_nt_tile (gram_nt_tile.hpp: slab
// loop, LDS image, tile pairs I <= J with the mirror stored from the same accumulator) under the policy GramPlain; the
// pairwise-complete and the weighted kernels (covariance_missing.hip, covariance_weighted.hip) are the same body under theirs.
#include "common.hpp"
#include "kernels.hpp"
#include "gram_nt_tile.hpp"

namespace ggl {

// One wave per row: every lane sums its elements n = lane, lane + 64, ... in order, then the xor tree of wave_sum.  The order
// is fixed by (N, lane) alone, so the means -- and with them S -- are bitwise reproducible.  No atomics.
__global__ __launch_bounds__(256) void k_row_means(const double* __restrict__ X, const long long* __restrict__ off,
                                                   const int* __restrict__ Ntab, double* __restrict__ mean, int p)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p) return;
    const int Nk = Ntab[k];
    const double* x = X + off[k] + (size_t)row * Nk;
    double s = 0.0;
    for (int n = lane; n < Nk; n += 64) s += x[n];
    s = wave_sum(s);
    if (lane == 0) mean[(size_t)k * p + row] = s / (double)Nk;
}

// Op of gram_nt_tile: one plane x - m, one accumulator set, S = acc / N_k
struct GramPlain : GramArena {
    static constexpr int PLANES = 1, NACC = 1;
    static constexpr bool PRELOAD = true;
    const double* mean;
    double* S;
    __device__ __forceinline__ double shift(int k, int p, int i) const { return mean ? mean[(size_t)k * p + i] : 0.0; }
    __device__ __forceinline__ void stage(bool on, double x, double m, double (&v)[1]) const { v[0] = on ? x - m : 0.0; }
    __device__ __forceinline__ void mma(const double (&a)[1], const double (&b)[1], v4d (&acc)[1]) const
    {
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc[0], 0, 0, 0);
    }
    __device__ __forceinline__ double value(const v4d (&acc)[1], int r) const { return acc[0][r] / (double)n_hi; }
    __device__ __forceinline__ void store(double v, size_t e) const { S[e] = v; }
};

template <int BM, int BK, int WM, int WN>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gram_nt(const double* __restrict__ X,
                                                                  const long long* __restrict__ off,
                                                                  const int* __restrict__ Ntab,
                                                                  const double* __restrict__ mean, double* __restrict__ S,
                                                                  int K, int p)
{
    gram_nt_tile<BM, BK, WM, WN>(GramPlain{{X, off, Ntab}, mean, S}, K, p);
}

int gram_tile(int K, int p, int force)
{
    if (force == 64 || force == 32) return force;
    const long T = (p + 63) / 64;
    return (long)K * T * (T + 1) / 2 >= 256 ? 64 : 32;      // enough 64 x 64 tile pairs for every CU, else the small tile
}

void launch_row_means(hipStream_t st, const double* X, const long long* off, const int* N, double* mean, int K, int p)
{
    hipLaunchKernelGGL(k_row_means, dim3((p + 3) / 4, K), dim3(256), 0, st, X, off, N, mean, p);
}

void launch_gram_nt(hipStream_t st, const double* X, const long long* off, const int* N, const double* mean, double* S, int K,
                    int p, int tile)
{
    gram_dispatch(K, p, tile, [&](auto s, dim3 grid, dim3 block) {
        using Sh = decltype(s);
        hipLaunchKernelGGL((k_gram_nt<Sh::BM, Sh::BK, Sh::WM, Sh::WN>), grid, block, 0, st, X, off, N, mean, S, K, p);
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// scaling by a diagonal
// ---------------------------------------------------------------------------------------------------------------------
// d (given, or the diagonal of X) is checked and its square roots are tabulated: err = smallest k * p + i with d[k,i] <= 0 or
// not finite (GGL_DIAG_OK: none)
__global__ __launch_bounds__(256) void k_diag_check(const double* __restrict__ X, const double* __restrict__ d,
                                                    double* __restrict__ d_out, double* __restrict__ sd,
                                                    int* __restrict__ err, int p)
{
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p) return;
    const size_t ki = (size_t)k * p + i;
    const double v = d ? d[ki] : X[(size_t)k * p * p + (size_t)i * p + i];
    if (!(v > 0.0) || !(v <= 1.79769313486231570815e308)) {
        atomicMin(err, (int)ki);
        return;
    }
    d_out[ki] = v;
    sd[ki] = sqrt(v);
}

// Y = X / (sd_i * sd_j): two square roots (tabulated above), one product, one division, each correctly rounded -- the
// operation order of scale_array_by_diagonal.  VEC = 2 (p even): 16-byte loads and stores.  Writes nothing when the check
// above raised the error word.  Y may be X (every element is read and written by the same thread).
template <int VEC>
__global__ __launch_bounds__(256) void k_scale_by_diag(const double* X, const double* __restrict__ sd, double* Y,
                                                       const int* __restrict__ err, int p)
{
    if (*err != GGL_DIAG_OK) return;
    const int k = blockIdx.y;
    const size_t pp = (size_t)p * p;
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e >= pp) return;
    const int i = (int)(e / p), j = (int)(e % p);
    const double* s = sd + (size_t)k * p;
    const double si = s[i];
    if (VEC == 2) {
        const double2 x = *reinterpret_cast<const double2*>(X + k * pp + e);
        double2 y;
        y.x = x.x / (si * s[j]);
        y.y = x.y / (si * s[j + 1]);
        *reinterpret_cast<double2*>(Y + k * pp + e) = y;
    } else {
        Y[k * pp + e] = X[k * pp + e] / (si * s[j]);
    }
}

void launch_scale_by_diag(hipStream_t st, const double* X, const double* d, double* Y, double* d_out, double* sd, int* err,
                          int K, int p)
{
    hipLaunchKernelGGL(k_diag_check, dim3((p + 255) / 256, K), dim3(256), 0, st, X, d, d_out, sd, err, p);
    const size_t pp = (size_t)p * p;
    if (p % 2 == 0)
        hipLaunchKernelGGL(k_scale_by_diag<2>, dim3((unsigned)((pp / 2 + 255) / 256), K), dim3(256), 0, st, X, sd, Y, err, p);
    else
        hipLaunchKernelGGL(k_scale_by_diag<1>, dim3((unsigned)((pp + 255) / 256), K), dim3(256), 0, st, X, sd, Y, err, p);
}

}  // namespace ggl
