// De-sparsified ("debiased") graphical lasso on the device (Jankova & van de Geer 2015): for an estimate Theta_k
// of the precision matrix from a covariance S_k of n_k observations
//
//     M_k      = Theta_k S_k                                   launch_gemm_right (gemm_sym.hip), full output
//     T_k      = 2 Theta_k - M_k Theta_k                       k_debias: the product and both epilogues below
//     SE_k[ij] = sqrt((Theta_ii Theta_jj + Theta_ij^2) / n_k)
//
// M Theta is symmetric in exact arithmetic (Theta S Theta), so only the tile pairs I <= J are computed
// (v_mfma_f64_16x16x4_f64) and (i,j), (j,i) are stored from one evaluation: T and SE are bitwise symmetric.  Both operands
// are row panels contiguous along the contraction index m -- rows I of M_k and rows J of Theta_k (Theta is symmetric: its
// rows are its columns) -- but they are rows of two DIFFERENT arrays, so a diagonal tile stages both; that is what this body
// has of its own beside gram_nt_tile.hpp, whose diagonal tile stages one operand.  Tile geometry (SymCfg), the work decode
// and the LDS image ([row][m], row length BK + 2) are those of the Gram kernels.
//
// Every accumulator sums m = 0, 1, 2, ... in steps of four in that order whatever the tile shape, K or the block that owns
// it, and there are no atomics: two calls give the same bits, and instance k's bits do not depend on K.
#include "common.hpp"
#include "kernels.hpp"
#include "sym_tile.hpp"

namespace ggl {

template <int BM, int BK, int WM, int WN>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_debias(const double* __restrict__ M, const double* __restrict__ Theta,
                                                                 const double* __restrict__ nobs, double* __restrict__ Tout,
                                                                 double* __restrict__ SEout, int K, int p)
{
    using Cfg = SymCfg<BM, BK, WM, WN, false>;
    constexpr int XLD = BK + 2, SLAB = BM * XLD;
    constexpr int RSTEP = Cfg::NT / BK;
    static_assert(Cfg::NT % BK == 0, "a row of the slab must be covered by whole thread rows");
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
    const size_t pp = (size_t)p * p;
    const double* Mk = M + (size_t)k * pp;
    const double* Tk = Theta + (size_t)k * pp;
    double* As = smem;
    double* Bs = smem + SLAB;

    v4d acc[Cfg::TI][Cfg::TJ];
#pragma unroll
    for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    // slab element (row lrow + q * RSTEP, index lcol): consecutive lanes read consecutive m of one row.  8-byte loads only:
    // a row of an odd p starts on an odd multiple of 8 bytes.
    const int lcol = tid % BK, lrow = tid / BK;
    const double *pa[Cfg::LPT], *pb[Cfg::LPT];
    bool oka[Cfg::LPT], okb[Cfg::LPT];
#pragma unroll
    for (int q = 0; q < Cfg::LPT; ++q) {
        const int r = lrow + q * RSTEP;
        oka[q] = (I0 + r) < p;
        okb[q] = (J0 + r) < p;
        pa[q] = Mk + (size_t)min(I0 + r, p - 1) * p;                      // clamped: always a valid row
        pb[q] = Tk + (size_t)min(J0 + r, p - 1) * p;
    }
    double ra[Cfg::LPT], rb[Cfg::LPT];
    auto fetch = [&](int m0) {
        const int m = min(m0 + lcol, p - 1);                              // clamped: past the end is never staged as data
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            ra[q] = pa[q][m];
            rb[q] = pb[q][m];
        }
    };
    // rows >= p and contraction indices >= p are staged as exact zeros, whatever was fetched there
    auto stage = [&](int m0) {
        const bool in = (m0 + lcol) < p;
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            const int r = lrow + q * RSTEP;
            As[r * XLD + lcol] = (in && oka[q]) ? ra[q] : 0.0;
            Bs[r * XLD + lcol] = (in && okb[q]) ? rb[q] : 0.0;
        }
    };
    auto compute = [&](int nq) {
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk >= nq) break;
            const int c = kk * 4 + (lane >> 4);
            double af[Cfg::TI], bf[Cfg::TJ];
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i) af[i] = As[(wr + i * 16 + (lane & 15)) * XLD + c];
#pragma unroll
            for (int j = 0; j < Cfg::TJ; ++j) bf[j] = Bs[(wc + j * 16 + (lane & 15)) * XLD + c];
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
                for (int j = 0; j < Cfg::TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    };

    // a wave whose sub-tile of a diagonal tile lies below the diagonal produces nothing that is kept
    const bool dead_wave = diag && (wr >= wc + WN);
    fetch(0);
    for (int m0 = 0; m0 < p; m0 += BK) {
        stage(m0);
        __syncthreads();
        fetch(m0 + BK);                                                   // past the end: clamped, never staged as data
        if (!dead_wave) compute(min(BK / 4, (p - m0 + 3) / 4));
        __syncthreads();
    }
    if (dead_wave) return;

    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.  The epilogue reads the upper
    // triangle of Theta; (i,j) and (j,i) are stored from one evaluation.
    const double nk = nobs[k];
    double* To = Tout + (size_t)k * pp;
    double* So = SEout + (size_t)k * pp;
#pragma unroll
    for (int tj = 0; tj < Cfg::TJ; ++tj) {
        const int gj = J0 + wc + tj * 16 + (lane & 15);
        const double thjj = Tk[(size_t)min(gj, p - 1) * p + min(gj, p - 1)];
#pragma unroll
        for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * r;
                if (gi < p && gj < p && (!diag || gi <= gj)) {
                    const double thij = Tk[(size_t)gi * p + gj], thii = Tk[(size_t)gi * p + gi];
                    const double t = 2.0 * thij - acc[ti][tj][r];
                    const double se = sqrt((thii * thjj + thij * thij) / nk);
                    To[(size_t)gi * p + gj] = t;
                    So[(size_t)gi * p + gj] = se;
                    if (gi != gj) {
                        To[(size_t)gj * p + gi] = t;
                        So[(size_t)gj * p + gi] = se;
                    }
                }
            }
    }
}

// The two tile shapes of the Gram kernels under their fill rule (gram_tile): 64 x 64 (BK = 16, four waves of 32 x 32) where
// the 64 x 64 tile pairs fill the chip, else 32 x 32 (BK = 32, four waves of 16 x 16)
void launch_debias(hipStream_t st, const double* M, const double* Theta, const double* nobs, double* Tout, double* SEout, int K,
                   int p, int tile)
{
    if (gram_tile(K, p, tile) == 64) {
        const int T = (p + 63) / 64;
        hipLaunchKernelGGL((k_debias<64, 16, 32, 32>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(sym_nt(64, 32, 32)), 0, st, M,
                           Theta, nobs, Tout, SEout, K, p);
    } else {
        const int T = (p + 31) / 32;
        hipLaunchKernelGGL((k_debias<32, 32, 16, 16>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(sym_nt(32, 16, 16)), 0, st, M,
                           Theta, nobs, Tout, SEout, K, p);
    }
}

}  // namespace ggl
