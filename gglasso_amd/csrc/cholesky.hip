// Batched FP64 Cholesky that returns what a Gaussian predictive score needs: for K symmetric matrices S_k and
// right-hand sides d_k
//
//     S_k + ridge I = L L^T,    log det = 2 sum_j log l_jj,    q = d^T (S_k + ridge I)^-1 d = |L^-1 d|^2
//
// One workgroup of four waves per matrix, any p >= 1, one code path.  Left-looking, block columns of 16: for block column
// j0 the update A[i, j0:j0+16] - L[i, :j0] L[j0:j0+16, :j0]^T of the diagonal block and of every row block below it is an NT
// product of row panels, both contiguous along the contraction index m, on v_mfma_f64_16x16x4_f64 -- the LDS image of
// gram_nt_tile.hpp and debias.hip ([row][m], row length BK + 2, rows past the end staged as exact zeros), 64 rows of A (16 per
// wave) against the 16 rows of the block column per round.  The contraction length j0 is a multiple of BK = 16: no slab is
// partial.  What follows the product runs on the VALU, one lane per row, 16 rows per wave:
//
//     x_j = (u_j - sum_{m<j} x_m l_jm) / l_jj,   m ascending,                    a row below the diagonal block: l from LDS
//     the same line with l_jm = lane j's x_m (a wave shuffle) and x_j = sqrt(.)  a row of the diagonal block (wave 0)
//
// The right-hand side is a border row: d_k is row p of a (p + 1)-row matrix, goes through the same two steps as every other
// row below a diagonal block, and holds y = L^-1 d at the end; q = y^T y.  S_k is overwritten by L (lower triangle, diagonal
// included), d_k by y: both are temporaries of the call.  Only the lower triangle of S_k is read.
//
// Failure rule.  The pivot a_jj - sum_m l_jm^2 of every column is tested by wave 0 (positive and finite), the first failing
// column goes to LDS, and EVERY wave reads it from there behind a barrier: the decision to stop is uniform in the workgroup, no
// wave waits at a barrier the others have left.  A NaN anywhere in the lower triangle reaches a pivot (column i for an entry
// (i, j)) and ends as a status.
//
// Every sum runs in a fixed order (the MFMA accumulators over m in steps of four, the VALU lines over m ascending, log det and
// the smallest pivot over j ascending in wave 0, q by lane over m = lane (mod 64) then the xor tree), a workgroup reads nothing
// of another instance and there are no atomics: two calls give the same bits and instance k's bits do not depend on K.
#include <cfloat>

#include "common.hpp"
#include "kernels.hpp"
#include "sym_tile.hpp"

namespace ggl {

namespace {
constexpr int CH_NB = 16;            // block column = MFMA tile edge = BK
constexpr int CH_ROWS = 64;          // rows of A per round: 16 per wave
constexpr int CH_XLD = CH_NB + 2;    // operand slab row length ([row][m])
constexpr int CH_ULD = CH_NB + 1;    // row length of the updated block and of the diagonal factor (one lane per row)
}  // namespace

// MFMA: the update on the matrix cores; false: the same LDS image, the same order of m, on the VALU (the measured
// alternative, DESIGN 25.6 -- reached from ggl_dev_chol_bench only)
template <bool MFMA>
__global__ __launch_bounds__(256) void k_chol_predict(double* S, double* d, double ridge, double* __restrict__ out, int p)
{
    __shared__ __attribute__((aligned(16))) double As[CH_ROWS * CH_XLD];
    __shared__ __attribute__((aligned(16))) double Bs[CH_NB * CH_XLD];
    __shared__ double Us[CH_ROWS * CH_ULD];
    __shared__ double Ls[CH_NB * CH_ULD];
    __shared__ int sh_status;
    const int k = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* Sk = S + (size_t)k * p * p;
    double* dk = d ? d + (size_t)k * p : nullptr;
    const int R = p + (dk ? 1 : 0);                                       // rows: the border row is row p
    auto rowp = [&](int g) -> double* { return g < p ? Sk + (size_t)g * p : dk; };

    const int lcol = tid & (CH_NB - 1), lrow = tid >> 4;                  // slab element: consecutive lanes, consecutive m
    double lsum = 0.0, minpiv = INFINITY;                                 // wave 0: sum_j log l_jj and the smallest pivot
    int status = -1;

    for (int j0 = 0; j0 < p; j0 += CH_NB) {
        const int nb = min(CH_NB, p - j0);
        for (int g0 = j0; g0 < R; g0 += CH_ROWS) {
            // ---- the update of rows [g0, g0 + 64) against the block column: acc = L[rows, :j0] L[j0:j0+16, :j0]^T
            v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
            if (j0 > 0) {
                const double* pa[4];
                bool oka[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int g = g0 + lrow + 16 * q;
                    oka[q] = g < R;
                    pa[q] = rowp(min(g, R - 1));                          // clamped: always a valid row
                }
                const bool okb = (j0 + lrow) < p;
                const double* pb = Sk + (size_t)min(j0 + lrow, p - 1) * p;
                double ra[4], rb;
                auto fetch = [&](int m0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) ra[q] = pa[q][m0 + lcol];
                    rb = pb[m0 + lcol];
                };
                const bool live = (g0 + wave * 16) < R;                   // a wave whose 16 rows are past the end adds zeros
                fetch(0);
                for (int m0 = 0; m0 < j0; m0 += CH_NB) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) As[(lrow + 16 * q) * CH_XLD + lcol] = oka[q] ? ra[q] : 0.0;
                    Bs[lrow * CH_XLD + lcol] = okb ? rb : 0.0;
                    __syncthreads();
                    if (m0 + CH_NB < j0) fetch(m0 + CH_NB);
                    if (live) {
                        if constexpr (MFMA) {
#pragma unroll
                            for (int kk = 0; kk < CH_NB / 4; ++kk) {
                                const int c = kk * 4 + (lane >> 4);
                                const double af = As[(wave * 16 + (lane & 15)) * CH_XLD + c];
                                const double bf = Bs[(lane & 15) * CH_XLD + c];
                                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc, 0, 0, 0);
                            }
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const double* a = As + (wave * 16 + (lane >> 4) + 4 * r) * CH_XLD;
                                const double* b = Bs + (lane & 15) * CH_XLD;
#pragma unroll
                                for (int m = 0; m < CH_NB; ++m) acc[r] = fma(a[m], b[m], acc[r]);
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            // ---- u = a - acc -> LDS, [row][column].  C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15,
            // row = (lane >> 4) + 4 * reg.  Lower triangle only; the ridge goes on the diagonal as it is loaded.
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = wave * 16 + (lane >> 4) + 4 * r;
                const int g = g0 + lr, col = j0 + (lane & 15);
                double a = 0.0;
                if (g < R && col < p && col <= g) {
                    a = rowp(g)[col];
                    if (g == col) a += ridge;
                }
                Us[lr * CH_ULD + (lane & 15)] = a - acc[r];
            }
            __syncthreads();

            // ---- one lane per row: lanes 0..15 of every wave take the wave's 16 rows (the others repeat them and store nothing)
            const int lr = wave * 16 + (lane & 15);
            double x[CH_NB];
#pragma unroll
            for (int c = 0; c < CH_NB; ++c) x[c] = Us[lr * CH_ULD + c];
            const bool diag_round = (g0 == j0);
            if (diag_round) {
                if (wave == 0) {
                    // the diagonal block, and whatever rows of the border share its 16 rows: l_jm is lane j's x_m
#pragma unroll
                    for (int j = 0; j < CH_NB; ++j) {
                        if (j < nb) {
                            double t = x[j];
#pragma unroll
                            for (int m = 0; m < j; ++m) t = fma(-x[m], __shfl(x[m], j, 64), t);
                            const double piv = __shfl(t, j, 64);
                            const bool good = (piv > 0.0) && (piv <= DBL_MAX);
                            if (!good && status < 0) status = j0 + j;
                            if (status < 0 || status == j0 + j) minpiv = (piv < minpiv || piv != piv) ? piv : minpiv;
                            const double ljj = sqrt(piv);
                            if (status < 0) lsum += log(ljj);
                            x[j] = ((lane & 15) == j) ? ljj : t / ljj;
                        }
                    }
                    if (lane < CH_NB) {
#pragma unroll
                        for (int c = 0; c < CH_NB; ++c) Ls[lane * CH_ULD + c] = x[c];
                    }
                    if (lane == 0) sh_status = status;
                }
                __syncthreads();
                status = sh_status;                                       // the same word for every wave, behind the barrier
                if (status >= 0) {
                    if (tid == 0) {
                        out[(size_t)k * 4 + 0] = -INFINITY;
                        out[(size_t)k * 4 + 1] = NAN;
                        out[(size_t)k * 4 + 2] = minpiv;
                        out[(size_t)k * 4 + 3] = (double)status;
                    }
                    return;
                }
            }
            if (!(diag_round && wave == 0)) {
#pragma unroll
                for (int j = 0; j < CH_NB; ++j) {
                    if (j < nb) {
                        double t = x[j];
#pragma unroll
                        for (int m = 0; m < j; ++m) t = fma(-x[m], Ls[j * CH_ULD + m], t);
                        x[j] = t / Ls[j * CH_ULD + j];
                    }
                }
            }
            {
                const int g = g0 + lr;
                if (lane < CH_NB && g < R) {
                    double* row = rowp(g);
#pragma unroll
                    for (int c = 0; c < CH_NB; ++c)
                        if (c < nb && j0 + c <= g) row[j0 + c] = x[c];
                }
            }
            __syncthreads();                                              // Us and Ls are free; the rows are visible to the workgroup
        }
    }

    if (wave == 0) {
        double q = 0.0;
        if (dk) {
            for (int m = lane; m < p; m += 64) q = fma(dk[m], dk[m], q);
            q = wave_sum(q);
        }
        if (lane == 0) {
            out[(size_t)k * 4 + 0] = 2.0 * lsum;
            out[(size_t)k * 4 + 1] = q;
            out[(size_t)k * 4 + 2] = minpiv;
            out[(size_t)k * 4 + 3] = -1.0;
        }
    }
}

// d (K,p) = X[:, target[r]] - mean[r, :] (mean null: X[:, target[r]]): the right-hand sides of the predictive scores, from
// the means launch_row_means_weighted left on the device
__global__ __launch_bounds__(256) void k_predict_rhs(const double* __restrict__ X, const double* __restrict__ mean,
                                                     const int* __restrict__ target, double* __restrict__ d, int K, int p, int N)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)K * p) return;
    const int r = (int)(e / p), i = (int)(e % p);
    const double x = X[(size_t)i * N + target[r]];
    d[e] = mean ? x - mean[e] : x;
}

void launch_chol_predict(hipStream_t st, double* S, double* d, double ridge, double* out, int K, int p, bool mfma)
{
    if (mfma) hipLaunchKernelGGL(k_chol_predict<true>, dim3(K), dim3(256), 0, st, S, d, ridge, out, p);
    else hipLaunchKernelGGL(k_chol_predict<false>, dim3(K), dim3(256), 0, st, S, d, ridge, out, p);
}

void launch_predict_rhs(hipStream_t st, const double* X, const double* mean, const int* target, double* d, int K, int p, int N)
{
    const size_t n = (size_t)K * p;
    hipLaunchKernelGGL(k_predict_rhs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, mean, target, d, K, p, N);
}

}  // namespace ggl
