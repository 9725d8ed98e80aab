// Sample covariance from observations, and scaling by a diagonal, on the device (the input side of every solver):
//
//     m[k,i]   = (1/N_k) sum_n X_k[i,n]                                   k_row_means
//     S_k      = (1/N_k) Xc Xc^T,  Xc[i,n] = X_k[i,n] - m[k,i]            k_gram_nt      (numpy.cov(X_k, bias=True))
//     Y[k,i,j] = X[k,i,j] / (sqrt(d[k,i]) * sqrt(d[k,j]))                  k_scale_by_diag (helper/basic_linalg.py:46-65)
//
// X_k is (p, N_k) row-major, variables in rows.  Both operands of the Gram product are rows of the same array, contiguous
// along the contraction index n ("NT"): a slab is fetched along n into registers, centred there, and written to LDS as
// [variable][n]; the centred copy never exists in HBM.  Only tile pairs I <= J are computed (v_mfma_f64_16x16x4_f64) and
// the mirror is stored from the same accumulator, so S is bitwise symmetric.  The tile machinery is that of the
// register-staged symmetric product (k_symm_tn, gemm_sym.hip): SymCfg, decode_block_xcd.
#include "common.hpp"
#include "kernels.hpp"
#include "sym_tile.hpp"

namespace ggl {

// One wave per row: every lane sums its elements n = lane, lane + 64, ... in order, then the xor tree of wave_sum.  The order
// is fixed by (N, lane) alone, so the means -- and with them S -- are bitwise reproducible.  No atomics.
__global__ __launch_bounds__(256) void k_row_means(const double* __restrict__ X, const long long* __restrict__ off,
                                                   const int* __restrict__ Ntab, int ld, double* __restrict__ mean, int p)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p) return;
    const int Nk = Ntab[k];
    const size_t rs = ld ? (size_t)ld : (size_t)Nk;
    const double* x = X + off[k] + (size_t)row * rs;
    double s = 0.0;
    for (int n = lane; n < Nk; n += 64) s += x[n];
    s = wave_sum(s);
    if (lane == 0) mean[(size_t)k * p + row] = s / (double)Nk;
}

// LDS image of an operand slab: [BM variables][BK samples], row length BK + 2 doubles.  A fragment read takes variable
// lane & 15 and sample 4 kk + (lane >> 4): within each group of 32 lanes the 16 variables fall on 16 different even
// (resp. odd) 8-byte bank pairs for BK = 16 and BK = 32, so ds_read_b64 runs without bank conflicts.
template <int BM, int BK, int WM, int WN>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gram_nt(const double* __restrict__ X,
                                                                  const long long* __restrict__ off,
                                                                  const int* __restrict__ Ntab, int ld,
                                                                  const double* __restrict__ mean, double* __restrict__ S,
                                                                  int K, int p)
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
    const int Nk = Ntab[k];
    const size_t rs = ld ? (size_t)ld : (size_t)Nk;
    const double* Xk = X + off[k];
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
        const int r = lrow + q * RSTEP;
        oka[q] = (I0 + r) < p;
        okb[q] = (J0 + r) < p;
        const int ia = min(I0 + r, p - 1), ib = min(J0 + r, p - 1);      // clamped: always a valid row
        pa[q] = Xk + (size_t)ia * rs;
        pb[q] = Xk + (size_t)ib * rs;
        ma[q] = mean ? mean[(size_t)k * p + ia] : 0.0;
        mb[q] = mean ? mean[(size_t)k * p + ib] : 0.0;
    }
    double ra[Cfg::LPT], rb[Cfg::LPT];
    auto fetch = [&](int n0) {
        const int n = min(n0 + lcol, Nk - 1);                            // clamped: past the end is never staged as data
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            ra[q] = pa[q][n];
            if (!diag) rb[q] = pb[q][n];
        }
    };
    // Centring happens here, and the zero padding AFTER it: a sample index >= N_k or a row >= p contributes 0 to every
    // product (not m_i m_j).
    auto stage = [&](int n0) {
        const bool in = (n0 + lcol) < Nk;
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            const int r = lrow + q * RSTEP;
            As[r * XLD + lcol] = (in && oka[q]) ? ra[q] - ma[q] : 0.0;
            if (!diag) Bs[r * XLD + lcol] = (in && okb[q]) ? rb[q] - mb[q] : 0.0;
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
    fetch(0);
    for (int n0 = 0; n0 < Nk; n0 += BK) {
        stage(n0);
        __syncthreads();
        fetch(n0 + BK);                                                   // past the end: clamped, never staged
        if (!dead_wave) compute(min(BK / 4, (Nk - n0 + 3) / 4));
        __syncthreads();
    }

    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* Sk = S + (size_t)k * p * p;
    const double dn = (double)Nk;
#pragma unroll
    for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < Cfg::TJ; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * r;
                const int gj = J0 + wc + tj * 16 + (lane & 15);
                if (gi < p && gj < p && (!diag || gi <= gj)) {
                    const double v = acc[ti][tj][r] / dn;
                    Sk[(size_t)gi * p + gj] = v;
                    if (gi != gj) Sk[(size_t)gj * p + gi] = v;
                }
            }
}

int gram_tile(int K, int p, int force)
{
    if (force == 64 || force == 32) return force;
    const long T = (p + 63) / 64;
    return (long)K * T * (T + 1) / 2 >= 256 ? 64 : 32;      // enough 64 x 64 tile pairs for every CU, else the small tile
}

void launch_row_means(hipStream_t st, const double* X, const long long* off, const int* N, int ld, double* mean, int K, int p)
{
    hipLaunchKernelGGL(k_row_means, dim3((p + 3) / 4, K), dim3(256), 0, st, X, off, N, ld, mean, p);
}

void launch_gram_nt(hipStream_t st, const double* X, const long long* off, const int* N, int ld, const double* mean,
                    double* S, int K, int p, int tile)
{
    if (gram_tile(K, p, tile) == 64) {
        const int T = (p + 63) / 64;
        hipLaunchKernelGGL((k_gram_nt<64, 16, 32, 32>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(256), 0, st, X, off, N, ld,
                           mean, S, K, p);
    } else {
        const int T = (p + 31) / 32;
        hipLaunchKernelGGL((k_gram_nt<32, 32, 16, 16>), dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(256), 0, st, X, off, N, ld,
                           mean, S, K, p);
    }
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
