// The one tile body of the FP64 Gram kernels S_k = f(X_k X_k^T): k_gram_nt (covariance.hip), k_gram_nt_pairwise
// (covariance_missing.hip) and k_gram_nt_weighted (covariance_weighted.hip).  Both operands are rows of the same array,
// contiguous along the contraction index n ("NT"): a slab is fetched along n into registers, turned into what is multiplied
// there (centred, weighted, masked) and written to LDS as [variable][n]; that copy never exists in HBM.  Only tile pairs
// I <= J are computed (v_mfma_f64_16x16x4_f64) and the mirror is stored from the same evaluation, so the result is bitwise
// symmetric.  Tile geometry and work decode are those of the register-staged symmetric product (sym_tile.hpp).
//
// What differs between the kernels is answered by an operand policy Op:
//
//     PLANES, NACC, PRELOAD      LDS planes per operand, accumulator sets per 16 x 16 block, and whether the fragments of a
//                                whole slab are read ahead of its products (true) or k-step by k-step (false)
//     instance(k, p)             called once; leaves n_lo, n_hi (the samples [n_lo, n_hi) are looped, n_lo a multiple of BK)
//                                and n_last (the last sample that may be read)
//     row(i), shift(k, p, i)     where row i lives, and what is subtracted from it
//     fetch(n)                   a per-sample value fetched beside the slab
//     stage(on, x, m, v)         one fetched value x of a position that is data by its INDEX (on) -> the PLANES values in LDS
//     mma(a, b, acc)             which plane pairs go into which accumulator set, in which order
//     value(acc, r), store(o, e) the result element from the accumulators, and where it goes (called for (i,j) and (j,i))
#pragma once
#include "kernels.hpp"
#include "sym_tile.hpp"

namespace ggl {

// Rows of an arena: instance k is the packed row-major (p, N[k]) array at off[k], all its samples are looped
struct GramArena {
    const double* X;
    const long long* off;
    const int* Ntab;
    const double* Xk;
    int n_lo, n_hi, n_last;
    __device__ __forceinline__ void instance(int k, int)
    {
        Xk = X + off[k];
        n_lo = 0;
        n_hi = Ntab[k];
        n_last = n_hi - 1;
    }
    __device__ __forceinline__ const double* row(int i) const { return Xk + (size_t)i * n_hi; }
    __device__ __forceinline__ void fetch(int) {}
};

// LDS image of an operand slab: [BM variables][BK samples], row length BK + 2 doubles, one image per plane ([planes of the
// I rows][planes of the J rows]; a diagonal tile stages the first half only).  A fragment read takes variable lane & 15 and
// sample 4 kk + (lane >> 4): within each group of 32 lanes the 16 variables fall on 16 different even (resp. odd) 8-byte
// bank pairs for BK = 16 and BK = 32, so ds_read_b64 runs without bank conflicts.
template <int BM, int BK, int WM, int WN, class Op>
__device__ __forceinline__ void gram_nt_tile(Op op, int K, int p)
{
    using Cfg = SymCfg<BM, BK, WM, WN, false>;
    constexpr int XLD = BK + 2, SLAB = BM * XLD, NP = Op::PLANES;
    constexpr int RSTEP = Cfg::NT / BK;
    constexpr int AHEAD = Op::PRELOAD ? BK / 4 : 1;       // k-steps whose fragments are read ahead of their products
    static_assert(Cfg::NT % BK == 0, "a row of the slab must be covered by whole thread rows");
    static_assert(64 % BK == 0, "a range that starts at a multiple of 64 must start at a slab of the full loop");
    __shared__ __attribute__((aligned(16))) double smem[2 * NP * SLAB];
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
    op.instance(k, p);
    double* As = smem;
    double* Bs = diag ? smem : smem + NP * SLAB;       // a diagonal tile has one operand

    v4d acc[Cfg::TI][Cfg::TJ][Op::NACC];
#pragma unroll
    for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TJ; ++j)
#pragma unroll
            for (int s = 0; s < Op::NACC; ++s) acc[i][j][s] = (v4d){0.0, 0.0, 0.0, 0.0};

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
        pa[q] = op.row(ia);
        pb[q] = op.row(ib);
        ma[q] = op.shift(k, p, ia);
        mb[q] = op.shift(k, p, ib);
    }
    double ra[Cfg::LPT], rb[Cfg::LPT];
    auto fetch = [&](int n0) {
        const int n = min(n0 + lcol, op.n_last);                         // clamped: past the end is never staged as data
        op.fetch(n);
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            ra[q] = pa[q][n];
            if (!diag) rb[q] = pb[q][n];
        }
    };
    // The policy's transform happens here, and the zero padding AFTER it: a sample index >= n_hi or a row >= p contributes 0
    // to every product (not m_i m_j), whatever was fetched there.
    auto stage = [&](int n0) {
        const bool in = (n0 + lcol) < op.n_hi;
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            const int r = lrow + q * RSTEP;
            double v[NP];
            op.stage(in && oka[q], ra[q], ma[q], v);
#pragma unroll
            for (int s = 0; s < NP; ++s) As[s * SLAB + r * XLD + lcol] = v[s];
            if (!diag) {
                op.stage(in && okb[q], rb[q], mb[q], v);
#pragma unroll
                for (int s = 0; s < NP; ++s) Bs[s * SLAB + r * XLD + lcol] = v[s];
            }
        }
    };
    auto frag = [&](const double* s, int w0, int i, int c, double (&f)[NP]) {
#pragma unroll
        for (int q = 0; q < NP; ++q) f[q] = s[q * SLAB + (w0 + i * 16 + (lane & 15)) * XLD + c];
    };
    auto compute = [&](int nq) {
#pragma unroll
        for (int k0 = 0; k0 < BK / 4; k0 += AHEAD) {
            if (k0 >= nq) break;
            double af[AHEAD][Cfg::TI][NP], bf[AHEAD][Cfg::TJ][NP];
#pragma unroll
            for (int g = 0; g < AHEAD; ++g) {
                if (k0 + g >= nq) break;
                const int c = (k0 + g) * 4 + (lane >> 4);
#pragma unroll
                for (int i = 0; i < Cfg::TI; ++i) frag(As, wr, i, c, af[g][i]);
#pragma unroll
                for (int j = 0; j < Cfg::TJ; ++j) frag(Bs, wc, j, c, bf[g][j]);
            }
#pragma unroll
            for (int g = 0; g < AHEAD; ++g) {
                if (k0 + g >= nq) break;
#pragma unroll
                for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
                    for (int j = 0; j < Cfg::TJ; ++j) op.mma(af[g][i], bf[g][j], acc[i][j]);
            }
        }
    };

    // a wave whose sub-tile of a diagonal tile lies below the diagonal produces nothing that is kept
    const bool dead_wave = diag && (wr >= wc + WN);
    fetch(op.n_lo);
    for (int n0 = op.n_lo; n0 < op.n_hi; n0 += BK) {
        stage(n0);
        __syncthreads();
        fetch(n0 + BK);                                                   // past the end: clamped, never staged as data
        if (!dead_wave) compute(min(BK / 4, (op.n_hi - n0 + 3) / 4));
        __syncthreads();
    }

    // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.  (i,j) and (j,i) are stored from
    // one evaluation.
#pragma unroll
    for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < Cfg::TJ; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * r;
                const int gj = J0 + wc + tj * 16 + (lane & 15);
                if (gi < p && gj < p && (!diag || gi <= gj)) {
                    const auto o = op.value(acc[ti][tj], r);
                    op.store(o, (size_t)k * p * p + (size_t)gi * p + gj);
                    if (gi != gj) op.store(o, (size_t)k * p * p + (size_t)gj * p + gi);
                }
            }
}

// The two tile shapes and their grids: 64 x 64 (BK = 16, four waves of 32 x 32) when gram_tile says so, else 32 x 32 (BK = 32,
// four waves of 16 x 16).  launch(shape, grid, block) starts the kernel instantiated with shape's BM, BK, WM, WN.
template <int BM_, int BK_, int WM_, int WN_>
struct GramShape {
    static constexpr int BM = BM_, BK = BK_, WM = WM_, WN = WN_;
};

template <class Shape, class F>
void gram_launch_shape(int K, int p, F&& launch)
{
    const int T = (p + Shape::BM - 1) / Shape::BM;
    launch(Shape{}, dim3(xcd_grid(T * (T + 1) / 2, K)), dim3(sym_nt(Shape::BM, Shape::WM, Shape::WN)));
}

template <class F>
void gram_dispatch(int K, int p, int tile, F&& launch)
{
    if (gram_tile(K, p, tile) == 64) gram_launch_shape<GramShape<64, 16, 32, 32>>(K, p, launch);
    else gram_launch_shape<GramShape<32, 32, 16, 16>>(K, p, launch);
}

}  // namespace ggl
