// StARS stability selection (Liu, Roeder, Wasserman 2010) on the device: the two ends of a batch of B subsamples x L lambdas.
//
//     arena[r,i,c] = X[i, idx[r,c]]                                           k_gather_cols   (the input side)
//     c[l,i,j]     = #{ r : |Theta[l*B + r, i, j]| >= t },  i < j              k_edge_stability (the output side)
//     num[l]       = sum_{i<j} c (B - c)
//
// The gather writes the packed arena the covariance kernels read (covariance.hip: instance r is the row-major (p, b) array
// at r p b), so the B subset covariances are an ordinary K = B call of launch_row_means / launch_gram_nt /
// launch_scale_by_diag and bitwise those of host-gathered columns.  Both kernels move bytes and do next to no arithmetic.
//
// The same layout with folds for subsamples serves K-fold cross-validation, whose output side is at the end of this file:
//     out[l*F + f] = <S_test[f], Theta[l*F + f]>                              k_heldout_dot, k_heldout_final
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

// Held-out scores of a K-fold cross-validation: out[k] = <St[k % F], T[k]> for the K = L F snapshots T and the F test
// covariances St (ggl_heldout_scores).  Workgroup g of instance k takes the elements [g, g + 1) HO_CHUNK of the row-major
// matrix, i.e. whole consecutive rows and pieces of them, read once: a lane loads 16 bytes, a wave 1 KiB of one stack per
// instruction, and 4 + 4 such loads of a thread are issued before the first product (8 KiB per wave in flight).
//
// Order of the sum, fixed by p alone: a thread adds its elements, 256 apart, into four accumulators by turns and combines
// them as (a0 + a1) + (a2 + a3); wave_sum; the four wave sums as (w0 + w1) + (w2 + w3) into partials[k][g]; k_heldout_final
// adds the partials of an instance in index order g = 0, 1, ...  No atomics: the same inputs give the same bits, and
// instance k reads T[k] and St[k % F] and nothing else, whichever instances share the launch.
//
// What bounds it: memory traffic, 2 flops per 16 bytes.  The bytes of T come from HBM, each read once (400 MB at p = 500,
// K = 200); St is F matrices that L instances each re-read (10 MB there), so a workgroup moves as many bytes of St as of T,
// from whichever cache holds them.  Measured (profiles/cross_validation.txt): 32.9 us for the 100 MB of T at K = 50 and
// 117 us for 400 MB at K = 200, 0.38 and 0.43 of the 8 TB/s HBM peak counting T alone.  Not measured: where the St bytes
// come from, and how much of the gap to a streaming copy (0.79 of the peak) they explain.  The chunk size and the loads in
// flight were chosen from published figures for streaming reads on this chip, not tuned.  An odd p * p leaves every second matrix at
// an address that is no multiple of 16, in T and St independently: such p take 8-byte loads (HO_VEC false), still 512
// contiguous bytes per wave instruction.
static constexpr int HO_THREADS = 256, HO_CHUNK = 8192, HO_UNROLL = 4;

int heldout_blocks(int p) { return (int)(((size_t)p * p + HO_CHUNK - 1) / HO_CHUNK); }

template <bool HO_VEC>
__global__ __launch_bounds__(HO_THREADS) void k_heldout_dot(const double* __restrict__ T, const double* __restrict__ St, int F,
                                                            int G, size_t pp, double* __restrict__ partials)
{
    __shared__ double wsum[HO_THREADS / 64];
    const int k = blockIdx.x / G, g = blockIdx.x % G;
    const size_t e0 = (size_t)g * HO_CHUNK, e1 = min(pp, e0 + (size_t)HO_CHUNK);      // e0 < pp: G = ceil(pp / HO_CHUNK)
    const double* t = T + (size_t)k * pp + e0;
    const double* s = St + (size_t)(k % F) * pp + e0;
    double a[HO_UNROLL] = {0.0, 0.0, 0.0, 0.0};
    if (HO_VEC) {
        // pp and HO_CHUNK even: e0, e1 even, and the launcher checked that both stacks start at a multiple of 16 bytes
        const int n = (int)((e1 - e0) / 2);
        const double2* t2 = reinterpret_cast<const double2*>(t);
        const double2* s2 = reinterpret_cast<const double2*>(s);
        int i = threadIdx.x;
        for (; i + (HO_UNROLL - 1) * HO_THREADS < n; i += HO_UNROLL * HO_THREADS) {
            double2 x[HO_UNROLL], y[HO_UNROLL];
#pragma unroll
            for (int u = 0; u < HO_UNROLL; ++u) x[u] = t2[i + u * HO_THREADS];
#pragma unroll
            for (int u = 0; u < HO_UNROLL; ++u) y[u] = s2[i + u * HO_THREADS];
#pragma unroll
            for (int u = 0; u < HO_UNROLL; ++u) a[u] += x[u].x * y[u].x + x[u].y * y[u].y;
        }
        for (int u = 0; i < n; i += HO_THREADS, ++u) {
            const double2 x = t2[i], y = s2[i];
            a[u] += x.x * y.x + x.y * y.y;                                            // (at most HO_UNROLL - 1 turns)
        }
    } else {
        const int n = (int)(e1 - e0);
        int i = threadIdx.x;
        for (; i + (HO_UNROLL - 1) * HO_THREADS < n; i += HO_UNROLL * HO_THREADS) {
            double x[HO_UNROLL], y[HO_UNROLL];
#pragma unroll
            for (int u = 0; u < HO_UNROLL; ++u) x[u] = t[i + u * HO_THREADS];
#pragma unroll
            for (int u = 0; u < HO_UNROLL; ++u) y[u] = s[i + u * HO_THREADS];
#pragma unroll
            for (int u = 0; u < HO_UNROLL; ++u) a[u] += x[u] * y[u];
        }
        for (int u = 0; i < n; i += HO_THREADS, ++u) a[u] += t[i] * s[i];
    }
    const double w = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void k_heldout_final(const double* __restrict__ partials, int K, int G, double* __restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const double* row = partials + (size_t)k * G;
    double s = 0.0;
    for (int g0 = 0; g0 < G; g0 += 8) {                                 // eight loads in flight, added in index order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = row[min(g0 + u, G - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (g0 + u < G) s += v[u];
    }
    out[k] = s;
}

// (the caller checked K * heldout_blocks(p) < 2^31)
void launch_heldout_dot(hipStream_t st, const double* T, const double* St, int K, int F, int p, double* partials, double* out)
{
    const size_t pp = (size_t)p * p;
    const int G = heldout_blocks(p);
    const bool vec = pp % 2 == 0 && (reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(St)) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(k_heldout_dot<true>, dim3(K * G), dim3(HO_THREADS), 0, st, T, St, F, G, pp, partials);
    else
        hipLaunchKernelGGL(k_heldout_dot<false>, dim3(K * G), dim3(HO_THREADS), 0, st, T, St, F, G, pp, partials);
    hipLaunchKernelGGL(k_heldout_final, dim3((K + 255) / 256), dim3(256), 0, st, partials, K, G, out);
}

}  // namespace ggl
