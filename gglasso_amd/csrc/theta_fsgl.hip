// Theta-step of the Functional Single Graphical Lasso: the proximal map of l * sum_{I != J} |Theta_IJ|_F over the M x M
// blocks of a (pM,pM) matrix (prox_sum_Frob, solver/ggl_helper.py:45-66, called at solver/functional_sgl_admm.py:147;
// dual update :156, sums of ADMM_stopping_criterion :241-255).
//
// One workgroup owns a pair of tiles (I,J), I <= J, of edge T = M * floor(32 / M) (M <= 32: a tile holds whole blocks):
//   1. the upper tile's V = (Omega + L) + X is read in its native orientation (rows of 32 consecutive doubles) into LDS;
//   2. per-block sums of squares in a fixed order: row segments first (one thread per row and block column), then the M
//      row sums of a block;  a = max(sqrt(sum), l), as prox_2norm (ggl_helper.py:38-43);
//   3. every thread finishes its native element of the upper tile, Theta = V (a - l) / a, and then its native element of
//      the mirror tile (J,I) from the transposed LDS entry -- the upper block decides, whatever the lower triangle of V
//      holds -- with its own Omega, X (L, Omega_prev) read coalesced: Theta write, dual update, the five sums.
// Diagonal blocks pass V through bit for bit.  Nothing is read or written with a stride, Omega / X / L are read once and
// Theta / X written once.  No atomics: every workgroup writes its five partial sums to its own slot.
//
// M > 32: a block spans several tiles.  k_fsgl_blocksq writes the table of block sums of squares first (one workgroup per
// upper block, fixed order), the same tile-pair kernel then takes its (at most 2 x 2) scales from the table (TABLE).
#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

static constexpr int FS_T = 32;            // largest tile edge
static constexpr int FS_LD = FS_T + 1;     // padded row of the transposition tile: column reads hit 32 different banks
static constexpr int FS_THREADS = 256;

int fsgl_tile(int M) { return M <= FS_T ? M * (FS_T / M) : FS_T; }

int fsgl_partial_blocks(int p, int M)
{
    const int T = fsgl_tile(M), nT = (p + T - 1) / T;
    return nT * (nT + 1) / 2;
}

// pair index q -> (I,J), I <= J, rows of the upper triangle one after the other
__device__ __forceinline__ void fs_pair(int q, int nT, int& I, int& J)
{
    const double b = 2.0 * nT + 1.0;
    int i = (int)((b - sqrt(b * b - 8.0 * (double)q)) * 0.5);
    i = max(0, min(i, nT - 1));
    while (i > 0 && i * nT - i * (i - 1) / 2 > q) --i;
    while ((i + 1) * nT - (i + 1) * i / 2 <= q) ++i;
    I = i;
    J = i + (q - (i * nT - i * (i - 1) / 2));
}

// MODE 0: non-latent step (Theta, X <- (X + Omega) - Theta, five sums); 1: latent (Theta, C = (Theta - X) - Omega);
// 2: the operator alone (V = Omega, Theta)
template <int MODE, bool TABLE>
__global__ __launch_bounds__(FS_THREADS) void k_theta_fsgl(double* __restrict__ Theta, double* __restrict__ X,
                                                           double* __restrict__ C, const double* __restrict__ Omega,
                                                           const double* __restrict__ OmegaPrev,
                                                           const double* __restrict__ L, const double* __restrict__ l1K,
                                                           const double* __restrict__ sqtab, double* __restrict__ partials,
                                                           int p, int M, int T, int nT, const int* __restrict__ skip)
{
    __shared__ double sV[FS_T * FS_LD];
    __shared__ double sRow[FS_T * FS_T];
    __shared__ double sNum[FS_T * FS_T];
    __shared__ double sDen[FS_T * FS_T];
    __shared__ double scratch[GGL_NNORM * (FS_THREADS / 64)];
    if (spec_failed(skip)) return;
    const int k = blockIdx.y;
    int I, J;
    fs_pair(blockIdx.x, nT, I, J);
    const size_t base = (size_t)k * p * p;
    const double lk = l1K[k];
    const int r0 = I * T, c0 = J * T;
    const int rb0 = r0 / M, cb0 = c0 / M;           // first block row / column of the tile
    const int nbw = TABLE ? 2 : T / M;              // block columns (and rows) a tile touches
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;

    // ---- 1. upper tile, native orientation ----
    double om[4], x[4], v[4];
    bool in[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = ty + 8 * e;
        const int gr = r0 + r, gc = c0 + tx;
        in[e] = r < T && tx < T && gr < p && gc < p;
        om[e] = x[e] = v[e] = 0.0;
        if (in[e]) {
            const size_t i = base + (size_t)gr * p + gc;
            om[e] = Omega[i];
            if (MODE == 2) {
                v[e] = om[e];
            } else {
                x[e] = X[i];
                const double l = (MODE == 1) ? L[i] : 0.0;
                v[e] = (om[e] + l) + x[e];
            }
        }
        sV[r * FS_LD + tx] = v[e];
    }
    __syncthreads();

    // ---- 2. a = max(|V_block|_F, l) per block: sNum = a - l, sDen = a ----
    if (TABLE) {
        if (threadIdx.x < 4) {
            const int nB = p / M;
            const int bi = rb0 + (threadIdx.x >> 1), bj = cb0 + (threadIdx.x & 1);
            const double s = (bi < bj && bj < nB) ? sqtab[((size_t)k * nB + bi) * nB + bj] : 0.0;
            const double a = fmax(sqrt(s), lk);
            sNum[threadIdx.x] = a - lk;
            sDen[threadIdx.x] = a;
        }
    } else {
        for (int t = threadIdx.x; t < nbw * T; t += FS_THREADS) {
            const int bc = t / T, r = t - bc * T;
            const double* row = sV + r * FS_LD + bc * M;
            double s = 0.0;
            for (int j = 0; j < M; ++j) s += row[j] * row[j];
            sRow[t] = s;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < nbw * nbw; t += FS_THREADS) {
            const int br = t / nbw, bc = t - br * nbw;
            const double* col = sRow + bc * T + br * M;
            double s = 0.0;
            for (int i = 0; i < M; ++i) s += col[i];
            const double a = fmax(sqrt(s), lk);
            sNum[t] = a - lk;
            sDen[t] = a;
        }
    }
    __syncthreads();

    // ---- 3. native elements of the upper tile, then of the mirror tile ----
    double acc[GGL_NNORM] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (in[e]) {
            const int r = ty + 8 * e;
            const int gr = r0 + r, gc = c0 + tx;
            const int bi = gr / M, bj = gc / M;
            double th;
            if (bi == bj) {
                th = v[e];
            } else if (bi < bj) {
                const int b = (bi - rb0) * nbw + (bj - cb0);
                th = (v[e] * sNum[b]) / sDen[b];
            } else {
                // (a diagonal tile's blocks below the diagonal: mirror of the upper element (gc, gr) of the same tile)
                const int b = (bj - rb0) * nbw + (bi - cb0);
                th = (sV[tx * FS_LD + r] * sNum[b]) / sDen[b];
            }
            const size_t i = base + (size_t)gr * p + gc;
            Theta[i] = th;
            if (MODE == 1) {
                C[i] = (th - x[e]) - om[e];
            } else if (MODE == 0) {
                const double xn = (x[e] + om[e]) - th;      // functional_sgl_admm.py:156
                X[i] = xn;
                const double dp = om[e] - OmegaPrev[i];
                acc[0] += om[e] * om[e];
                acc[1] += th * th;
                acc[2] += xn * xn;
                acc[3] += (om[e] - th) * (om[e] - th);
                acc[4] += dp * dp;
            }
        }
    }
    if (I < J) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = ty + 8 * e;
            const int gr = c0 + r, gc = r0 + tx;        // element (gr, gc) of tile (J,I); its source is (gc, gr) = sV[tx][r]
            if (r < T && tx < T && gr < p && gc < p) {
                const size_t i = base + (size_t)gr * p + gc;
                const double o = Omega[i];
                const double xx = (MODE == 2) ? 0.0 : X[i];
                const int bi = gc / M, bj = gr / M;     // block of the source element, bi <= bj
                double th;
                if (bi == bj) {
                    // (M > 32 only: both tiles inside one diagonal block)
                    const double l = (MODE == 1) ? L[i] : 0.0;
                    th = (MODE == 2) ? o : (o + l) + xx;
                } else {
                    const int b = (bi - rb0) * nbw + (bj - cb0);
                    th = (sV[tx * FS_LD + r] * sNum[b]) / sDen[b];
                }
                Theta[i] = th;
                if (MODE == 1) {
                    C[i] = (th - xx) - o;
                } else if (MODE == 0) {
                    const double xn = (xx + o) - th;
                    X[i] = xn;
                    const double dp = o - OmegaPrev[i];
                    acc[0] += o * o;
                    acc[1] += th * th;
                    acc[2] += xn * xn;
                    acc[3] += (o - th) * (o - th);
                    acc[4] += dp * dp;
                }
            }
        }
    }
    if (MODE == 0) {
        block_sum<GGL_NNORM>(acc, scratch);
        if (threadIdx.x == 0) {
            double* o = partials + ((size_t)k * gridDim.x + blockIdx.x) * GGL_NNORM;
#pragma unroll
            for (int q = 0; q < GGL_NNORM; ++q) o[q] = acc[q];
        }
    }
}

// out[k][bi][bj] for the blocks bi <= bj of V = (Omega + L) + X (X, L may be null): the sum of squares (what == 0) or the
// Frobenius norm, mirrored into [bj][bi] (what == 1; what == 2: diagonal entries 0), frob_norm_per_block, helper/utils.py:69-87.
// One workgroup per block, elements in row-major order over the threads, fixed reduction order.
__global__ __launch_bounds__(FS_THREADS) void k_fsgl_blocksq(double* __restrict__ out, const double* __restrict__ Omega,
                                                             const double* __restrict__ X, const double* __restrict__ L,
                                                             int p, int M, int nB, int what, const int* __restrict__ skip)
{
    __shared__ double scratch[FS_THREADS / 64];
    if (spec_failed(skip)) return;
    const int bi = blockIdx.x / nB, bj = blockIdx.x - bi * nB;
    if (bi > bj) return;
    const int k = blockIdx.y;
    const size_t base = (size_t)k * p * p + (size_t)bi * M * p + (size_t)bj * M;
    double acc[1] = {0.0};
    const int n = M * M;
    for (int e = threadIdx.x; e < n; e += FS_THREADS) {
        const int r = e / M, c = e - r * M;
        const size_t i = base + (size_t)r * p + c;
        double v = Omega[i];
        if (L) v += L[i];
        if (X) v += X[i];
        acc[0] += v * v;
    }
    block_sum<1>(acc, scratch);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)k * nB * nB;
        if (what == 0) {
            o[(size_t)bi * nB + bj] = acc[0];
        } else {
            const double nrm = (what == 2 && bi == bj) ? 0.0 : sqrt(acc[0]);
            o[(size_t)bi * nB + bj] = nrm;
            o[(size_t)bj * nB + bi] = nrm;
        }
    }
}

void launch_fsgl_block_table(hipStream_t st, double* out, const double* Omega, const double* X, const double* L, int K,
                             int p, int M, int what, const int* skip)
{
    const int nB = p / M;
    hipLaunchKernelGGL(k_fsgl_blocksq, dim3(nB * nB, K), dim3(FS_THREADS), 0, st, out, Omega, X, L, p, M, nB, what, skip);
}

int launch_theta_fsgl(hipStream_t st, double* Theta, double* X, double* C, const double* Omega, const double* OmegaPrev,
                      const double* L, const double* l1K, int mode, double* sqtab, double* partials, int K, int p, int M,
                      const int* skip)
{
    const int T = fsgl_tile(M), nT = (p + T - 1) / T;
    const dim3 grid(nT * (nT + 1) / 2, K), blk(FS_THREADS);
    const bool table = M > FS_T;
    if (table) launch_fsgl_block_table(st, sqtab, Omega, mode == 2 ? nullptr : X, mode == 1 ? L : nullptr, K, p, M, 0, skip);
#define GGL_FS(MODE, TAB)                                                                                              \
    hipLaunchKernelGGL((k_theta_fsgl<MODE, TAB>), grid, blk, 0, st, Theta, X, C, Omega, OmegaPrev, L, l1K, sqtab, partials, p, \
                       M, T, nT, skip)
    if (mode == 0) { if (table) GGL_FS(0, true); else GGL_FS(0, false); }
    else if (mode == 1) { if (table) GGL_FS(1, true); else GGL_FS(1, false); }
    else { if (table) GGL_FS(2, true); else GGL_FS(2, false); }
#undef GGL_FS
    theta_note_kernel(table ? 5000 + T : 4000 + T);
    return table ? 2 : 1;
}

}  // namespace ggl
