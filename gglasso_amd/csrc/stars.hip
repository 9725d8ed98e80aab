// StARS stability selection (Liu, Roeder, Wasserman 2010) on the device: the two ends of a batch of B subsamples x L lambdas.
//
//     arena[r,i,c] = X[i, idx[r,c]]                                           k_gather_cols   (the input side)
//     c[l,i,j]     = #{ r : |Theta[l*B + r, i, j]| >= t },  i < j              k_edge_stability (the output side)
//     num[l]       = sum_{i<j} c (B - c)
//
// The gather writes the packed arena the covariance kernels read (covariance.hip: instance r is the row-major (p, b) array
// at r p b), so the B subset covariances are an ordinary K = B call of launch_row_means / launch_gram_nt /
// launch_scale_by_diag and bitwise those of host-gathered columns.  Both kernels move bytes and do next to no arithmetic.
#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

// One thread per column c of a subset: the index is read once and serves GATHER_ROWS rows, whose loads are independent
// (all in flight together); consecutive lanes write consecutive doubles of an arena row.  idx was checked on the host.
static constexpr int GATHER_ROWS = 8;

__global__ __launch_bounds__(256) void k_gather_cols(const double* __restrict__ X, const int* __restrict__ idx,
                                                     double* __restrict__ arena, int p, int N, int b)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.z;
    if (c >= b) return;
    const int i0 = blockIdx.y * GATHER_ROWS;
    const int n = idx[(size_t)r * b + c];
    const double* x = X + n;
    double* out = arena + (size_t)r * p * b + c;
    double v[GATHER_ROWS];
#pragma unroll
    for (int q = 0; q < GATHER_ROWS; ++q) v[q] = x[(size_t)min(i0 + q, p - 1) * N];        // clamped: always a valid row
#pragma unroll
    for (int q = 0; q < GATHER_ROWS; ++q)
        if (i0 + q < p) out[(size_t)(i0 + q) * b] = v[q];
}

void launch_gather_cols(hipStream_t st, const double* X, const int* idx, double* arena, int p, int N, int B, int b)
{
    hipLaunchKernelGGL(k_gather_cols, dim3((b + 255) / 256, (p + GATHER_ROWS - 1) / GATHER_ROWS, B), dim3(256), 0, st, X, idx,
                       arena, p, N, b);
}

// One workgroup per 32 x 32 tile pair I <= J of one lambda: thread (row ty + 8 q, column tx) owns four elements, a wave
// reads two 256-byte row segments per load.  The loop over the B snapshots keeps 4 x 4 loads of a thread in flight (the FGL
// Theta kernel does the same for its rows).  Only elements j > i are read: a Theta need not be symmetric, its upper
// triangle decides.  A NaN compares false and is no edge.  The counts leave as int32 to (i,j) from the registers and to
// (j,i) through a transposed LDS tile, so both stores run along rows; the diagonal is written as zero.
//
// Exactness: c <= B, so c (B - c) <= B^2 / 4 (formed in 64 bits) and num[l] <= p (p - 1) / 2 * B^2 / 4, which fits a 64-bit
// integer while p B < 8.5e9 (ggl_edge_stability checks it): B = 1000, p = 4000 gives 2.0e12.  Integer sums do not depend
// on their order, so the wave -> workgroup -> one atomic per workgroup reduction is bitwise reproducible.
static constexpr int ES_TILE = 32, ES_Q = 4, ES_RB = 4;

__global__ __launch_bounds__(256) void k_edge_stability(const double* __restrict__ T, int B, int p, double t,
                                                        int* __restrict__ counts, unsigned long long* __restrict__ num)
{
    __shared__ int tile[ES_TILE][ES_TILE + 1];
    __shared__ long long wsum[4];
    const int nT = (p + ES_TILE - 1) / ES_TILE;
    int b = blockIdx.x, I = 0;
    while (b >= nT - I) { b -= nT - I; ++I; }
    const int J = I + b, l = blockIdx.y;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int gj = J * ES_TILE + tx;
    const size_t pp = (size_t)p * p;
    const double* Tl = T + (size_t)l * B * pp;

    int cnt[ES_Q];
    bool own[ES_Q];
    size_t off[ES_Q];
#pragma unroll
    for (int q = 0; q < ES_Q; ++q) {
        const int gi = I * ES_TILE + ty + 8 * q;
        own[q] = gi < p && gj < p && gi < gj;
        off[q] = own[q] ? (size_t)gi * p + gj : 0;                      // not owned: never loaded
        cnt[q] = 0;
    }
    int r = 0;
    for (; r + ES_RB <= B; r += ES_RB) {
        double v[ES_RB][ES_Q];
#pragma unroll
        for (int s = 0; s < ES_RB; ++s)
#pragma unroll
            for (int q = 0; q < ES_Q; ++q) v[s][q] = own[q] ? Tl[(size_t)(r + s) * pp + off[q]] : 0.0;
#pragma unroll
        for (int s = 0; s < ES_RB; ++s)
#pragma unroll
            for (int q = 0; q < ES_Q; ++q) cnt[q] += (own[q] && fabs(v[s][q]) >= t) ? 1 : 0;
    }
    for (; r < B; ++r) {
#pragma unroll
        for (int q = 0; q < ES_Q; ++q) {
            const double v = own[q] ? Tl[(size_t)r * pp + off[q]] : 0.0;
            cnt[q] += (own[q] && fabs(v) >= t) ? 1 : 0;
        }
    }

    long long s = 0;
#pragma unroll
    for (int q = 0; q < ES_Q; ++q) s += (long long)cnt[q] * (long long)(B - cnt[q]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    if (counts) {
#pragma unroll
        for (int q = 0; q < ES_Q; ++q) tile[ty + 8 * q][tx] = cnt[q];    // zero where not owned
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(num + l, (unsigned long long)tot);
    }
    if (!counts) return;
    int* Cl = counts + (size_t)l * pp;
#pragma unroll
    for (int q = 0; q < ES_Q; ++q) {
        const int gi = I * ES_TILE + ty + 8 * q;
        if (gi < p && gj < p && gi <= gj) Cl[(size_t)gi * p + gj] = cnt[q];       // (gi == gj: zero)
        // the mirror: row J * 32 + ty + 8 q, column I * 32 + tx of the table is element (tx, ty + 8 q) of this tile
        const int mi = J * ES_TILE + ty + 8 * q, mj = I * ES_TILE + tx;
        if (mi < p && mj < p && mi > mj) Cl[(size_t)mi * p + mj] = tile[tx][ty + 8 * q];
    }
}

void launch_edge_stability(hipStream_t st, const double* T, int L, int B, int p, double t, int* counts,
                           unsigned long long* num)
{
    const int nT = (p + ES_TILE - 1) / ES_TILE;
    hipLaunchKernelGGL(k_edge_stability, dim3(nT * (nT + 1) / 2, L), dim3(256), 0, st, T, B, p, t, counts, num);
}

}  // namespace ggl
