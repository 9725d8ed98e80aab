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
// k_gram_nt_pairwise is k_gram_nt (covariance.hip) with a mask slab beside every data slab and four accumulator sets: the
// same tile pairs I <= J, the same XCD decode, the mirror stored from the same evaluation (S and the counts are bitwise
// symmetric).  The mask is staged on its own -- an observed entry equal to its row mean has y = 0 -- and a padded position
// (sample >= N_k or row >= p, fetched clamped and possibly NaN) gets y = w = 0 by the index test alone.
#include "common.hpp"
#include "kernels.hpp"
#include "sym_tile.hpp"

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

// LDS: [Y of the I rows][W of the I rows][Y of the J rows][W of the J rows], each the [BM][BK + 2] image of k_gram_nt; a
// diagonal tile stages the first two only.
template <int BM, int BK, int WM, int WN, bool CENTER>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gram_nt_pairwise(const double* __restrict__ X,
                                                                           const long long* __restrict__ off,
                                                                           const int* __restrict__ Ntab,
                                                                           const double* __restrict__ shift,
                                                                           double* __restrict__ S, int* __restrict__ counts,
                                                                           int K, int p)
{
    using Cfg = SymCfg<BM, BK, WM, WN, false>;
    constexpr int XLD = BK + 2, SLAB = BM * XLD;
    constexpr int RSTEP = Cfg::NT / BK;
    static_assert(Cfg::NT % BK == 0, "a row of the slab must be covered by whole thread rows");
    __shared__ __attribute__((aligned(16))) double smem[4 * SLAB];
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
    const int Nk = Ntab[k];
    const double* Xk = X + off[k];
    double* Ay = smem;
    double* Aw = smem + SLAB;
    double* By = diag ? Ay : smem + 2 * SLAB;      // a diagonal tile has one operand pair
    double* Bw = diag ? Aw : smem + 3 * SLAB;

    v4d accP[Cfg::TI][Cfg::TJ], accA[Cfg::TI][Cfg::TJ], accB[Cfg::TI][Cfg::TJ], accC[Cfg::TI][Cfg::TJ];
#pragma unroll
    for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TJ; ++j)
            accP[i][j] = accA[i][j] = accB[i][j] = accC[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    const int lcol = tid % BK, lrow = tid / BK;
    const double *pa[Cfg::LPT], *pb[Cfg::LPT];
    double ma[Cfg::LPT], mb[Cfg::LPT];
    bool oka[Cfg::LPT], okb[Cfg::LPT];
#pragma unroll
    for (int q = 0; q < Cfg::LPT; ++q) {
        const int r = lrow + q * RSTEP;
        oka[q] = (I0 + r) < p;
        okb[q] = (J0 + r) < p;
        const int ia = min(I0 + r, p - 1), ib = min(J0 + r, p - 1);      // clamped: always a valid row
        pa[q] = Xk + (size_t)ia * Nk;
        pb[q] = Xk + (size_t)ib * Nk;
        ma[q] = CENTER ? shift[(size_t)k * p + ia] : 0.0;
        mb[q] = CENTER ? shift[(size_t)k * p + ib] : 0.0;
    }
    double ra[Cfg::LPT], rb[Cfg::LPT];
    auto fetch = [&](int n0) {
        const int n = min(n0 + lcol, Nk - 1);                            // clamped: what it reads there may be a NaN
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            ra[q] = pa[q][n];
            if (!diag) rb[q] = pb[q][n];
        }
    };
    // A position is data only by its INDEX (in && ok); only then does the value decide between observed and missing.
    auto stage = [&](int n0) {
        const bool in = (n0 + lcol) < Nk;
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            const int r = lrow + q * RSTEP;
            const bool oa = in && oka[q] && (ra[q] == ra[q]);
            Ay[r * XLD + lcol] = oa ? ra[q] - ma[q] : 0.0;
            Aw[r * XLD + lcol] = oa ? 1.0 : 0.0;
            if (!diag) {
                const bool ob = in && okb[q] && (rb[q] == rb[q]);
                By[r * XLD + lcol] = ob ? rb[q] - mb[q] : 0.0;
                Bw[r * XLD + lcol] = ob ? 1.0 : 0.0;
            }
        }
    };
    // four fragment reads, four products per 16 x 16 block and k-step (two without centring: A and B are not needed)
    auto compute = [&](int nq) {
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk >= nq) break;
            const int c = kk * 4 + (lane >> 4);
            double ay[Cfg::TI], aw[Cfg::TI], by[Cfg::TJ], bw[Cfg::TJ];
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i) {
                ay[i] = Ay[(wr + i * 16 + (lane & 15)) * XLD + c];
                aw[i] = Aw[(wr + i * 16 + (lane & 15)) * XLD + c];
            }
#pragma unroll
            for (int j = 0; j < Cfg::TJ; ++j) {
                by[j] = By[(wc + j * 16 + (lane & 15)) * XLD + c];
                bw[j] = Bw[(wc + j * 16 + (lane & 15)) * XLD + c];
            }
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
                for (int j = 0; j < Cfg::TJ; ++j) {
                    accP[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[i], by[j], accP[i][j], 0, 0, 0);
                    if (CENTER) {
                        accA[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ay[i], bw[j], accA[i][j], 0, 0, 0);
                        accB[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aw[i], by[j], accB[i][j], 0, 0, 0);
                    }
                    accC[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aw[i], bw[j], accC[i][j], 0, 0, 0);
                }
        }
    };

    const bool dead_wave = diag && (wr >= wc + WN);
    fetch(0);
    for (int n0 = 0; n0 < Nk; n0 += BK) {
        stage(n0);
        __syncthreads();
        fetch(n0 + BK);                                                   // past the end: clamped, never staged as data
        if (!dead_wave) compute(min(BK / 4, (Nk - n0 + 3) / 4));
        __syncthreads();
    }

    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.  (i,j) and (j,i) are stored from
    // one evaluation; n_ij = 0 leaves a NaN for k_pair_count_check to refuse.
    double* Sk = S + (size_t)k * p * p;
    int* Ck = counts + (size_t)k * p * p;
#pragma unroll
    for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < Cfg::TJ; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * r;
                const int gj = J0 + wc + tj * 16 + (lane & 15);
                if (gi < p && gj < p && (!diag || gi <= gj)) {
                    const double n = accC[ti][tj][r];
                    const double v = CENTER ? (accP[ti][tj][r] - accA[ti][tj][r] * accB[ti][tj][r] / n) / n : accP[ti][tj][r] / n;
                    const int ni = (int)n;
                    Sk[(size_t)gi * p + gj] = v;
                    Ck[(size_t)gi * p + gj] = ni;
                    if (gi != gj) {
                        Sk[(size_t)gj * p + gi] = v;
                        Ck[(size_t)gj * p + gi] = ni;
                    }
                }
            }
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

template <bool CENTER>
static void launch_pairwise(hipStream_t st, const double* X, const long long* off, const int* N, const double* shift, double* S,
                            int* counts, int K, int p, int tile)
{
    if (gram_tile(K, p, tile) == 64) {
        const int T = (p + 63) / 64;
        hipLaunchKernelGGL((k_gram_nt_pairwise<64, 16, 32, 32, CENTER>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(256), 0, st, X,
                           off, N, shift, S, counts, K, p);
    } else {
        const int T = (p + 31) / 32;
        hipLaunchKernelGGL((k_gram_nt_pairwise<32, 32, 16, 16, CENTER>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(256), 0, st, X,
                           off, N, shift, S, counts, K, p);
    }
}

void launch_gram_nt_pairwise(hipStream_t st, const double* X, const long long* off, const int* N, const double* shift, double* S,
                             int* counts, int K, int p, int tile)
{
    if (shift) launch_pairwise<true>(st, X, off, N, shift, S, counts, K, p, tile);
    else launch_pairwise<false>(st, X, off, N, shift, S, counts, K, p, tile);
}

void launch_pair_count_check(hipStream_t st, const int* counts, int min_pairs, unsigned long long* err, int K, int p)
{
    const size_t total = (size_t)K * p * p;
    hipLaunchKernelGGL(k_pair_count_check, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts, total, min_pairs, err);
}

}  // namespace ggl
