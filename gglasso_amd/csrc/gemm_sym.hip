// Batched FP64 matrix-core product of COMMUTING SYMMETRIC matrices, the workhorse of the
// eigendecomposition-free Omega-step (newton_schulz.hip):
//
//     C[k] = cI[k]*I + cAcc[k]*(A[k] * B[k]) + cE[k]*E[k]        (+ optional C2[k] = dI[k]*I + dC[k]*C[k])
//
// A, B symmetric and commuting  =>  A*B = A^T*B is symmetric.  Written as a "TN" product both
// operands are read along contiguous rows (row m of A, columns I0.. and row m of B, columns J0..),
// only tile pairs I<=J are computed (v_mfma_f64_16x16x4_f64), and the I<J tiles are mirrored through
// an LDS transpose, so every global access is row-contiguous and the output is bitwise symmetric.
//
// Tiling: BM x BM block tile, NW waves as a (BM/WM) x (BM/WN) grid, each wave WM x WN = (WM/16) x
// (WN/16) MFMA tiles; k-slab BK.  The next slab is fetched from HBM/L2 into registers while the
// current one is consumed from LDS (software prefetch), one barrier pair per slab.
#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "common.hpp"
#include "kernels.hpp"
#include "sym_tile.hpp"

namespace ggl {


// second output of a product launch, C2 = dI I + dC C + dE E: one fixed evaluation order at every store site (upper
// triangle, diagonal-tile mirror, LDS-transposed mirror), so that the output is bitwise symmetric
__device__ __forceinline__ double c2val(double dC, double v, double dE, double e) { return __builtin_fma(dE, e, dC * v); }
// ... with the second affine operand E2 (present: has2) added last: C2 = dI I + dC C + dE E + dE2 E2
__device__ __forceinline__ double c2val2(double dC, double v, double dE, double e, bool has2, double dE2, double f)
{
    const double w = c2val(dC, v, dE, e);
    return has2 ? __builtin_fma(dE2, f, w) : w;
}

// Cross-lane moves of the register epilogue (symm_dl_tile), doubles as two dwords each.
// lane_xor1: the value of lane ^ 1 (DPP quad_perm [1,0,3,2]: no LDS, no wait)
__device__ __forceinline__ double lane_xor1(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, 0xB1, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0xB1, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// swap_row16: the odd 16-lane rows of a <-> the even ones of b (v_permlane16_swap), a half exchange: the other rows stay
// where they are.  (The hazard "VALU write -> permlane read" is the compiler's: it pads the builtin itself.)
__device__ __forceinline__ void swap_row16(double& a, double& b)
{
    const unsigned long long x = (unsigned long long)__double_as_longlong(a), y = (unsigned long long)__double_as_longlong(b);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)y, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(x >> 32), (unsigned)(y >> 32), false, false);
    a = __longlong_as_double((long long)(((unsigned long long)hi[0] << 32) | lo[0]));
    b = __longlong_as_double((long long)(((unsigned long long)hi[1] << 32) | lo[1]));
}

// ABL != 0: timing ablations and the timeline probe, instantiated by GGL_DEV builds only (tools/bench_tail.py)
template <int BM, int BK, int WM, int WN, bool LM, int ABL = 0>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_symm_tn(
    const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C, double* __restrict__ C2,
    const double* __restrict__ E, const double* __restrict__ coef, int K, int p, const double* __restrict__ A1,
    const double* __restrict__ B1, double* __restrict__ C1, int K1, double* __restrict__ maxdev,
    const double* __restrict__ E2)
{
    // maxdev != null: maxdev[k] = max over the instance of |C - I| (atomic max on the bit pattern of a
    // non-negative double: order independent, hence deterministic).
    // Instances k < K use (A, B, C, C2, E); instances K <= k < K + K1 use the second set (A1, B1, C1):
    // two independent products of one Newton-Schulz step share a launch, so that the chip sees 2K
    // instances' worth of tiles at once.  coef is indexed by the combined k.
    using Cfg = SymCfg<BM, BK, WM, WN, LM>;
    __shared__ __attribute__((aligned(16))) double smem[Cfg::LDS_DOUBLES];
    double* As = smem;
    double* Bs = smem + Cfg::SLAB;
    const int T = (p + BM - 1) / BM;
    int k, b;
    if (!decode_block_xcd(T * (T + 1) / 2, K + K1, k, b)) return;
    const bool second = k >= K;
    const int kk = second ? k - K : k;
    int I = 0;
    while (b >= T - I) { b -= T - I; ++I; }
    const int J = I + b;
    const int I0 = I * BM, J0 = J * BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave / Cfg::NWC) * WM, wc = (wave % Cfg::NWC) * WN;
    const size_t pp = (size_t)p * p;
    const double* Ak = (second ? A1 : A) + (size_t)kk * pp;
    const double* Bk = (second ? B1 : B) + (size_t)kk * pp;

#ifdef GGL_DEV
    long long t_start = 0, t_loop = 0, t_loop_end = 0;
    if (ABL == 3) t_start = clock64();
#endif

    v4d acc[Cfg::TI][Cfg::TJ];
#pragma unroll
    for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    // slab element e = tid + q*NT -> row e / BM, col e % BM
    constexpr int RSTEP = Cfg::NT / BM;
    constexpr int NST = 1;                      // slabs in flight (register stages); 1 measured best, 3 was -8%
    const int lcol = tid % BM, lrow = tid / BM;
    const bool aok = (I0 + lcol) < p, bok = (J0 + lcol) < p;
    double ra[NST][Cfg::LPT], rb[NST][Cfg::LPT];

    // Unconditional fetch from clamped (always valid) addresses with 32-bit element offsets (p*p < 2^31);
    // out-of-range elements are zeroed only when the slab is staged into LDS, so nothing consumes a load
    // early and NST slabs (NST * 2 * BK * BM * 8 bytes per workgroup) stay in flight: the product is
    // latency-bound on the L2/MALL path otherwise.
    const unsigned pu = (unsigned)p, pm1 = (unsigned)(p - 1);
    const unsigned ca = min((unsigned)(I0 + lcol), pm1), cb = min((unsigned)(J0 + lcol), pm1);
    auto fetch = [&](int m0, double (&xa)[Cfg::LPT], double (&xb)[Cfg::LPT]) {
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            if (ABL == 1 || ABL == 4 || ABL == 5) { xa[q] = 1.0 + q; xb[q] = 2.0 + q; continue; }   // ablation: no global loads
            const unsigned ro = min((unsigned)(m0 + lrow + q * RSTEP), pm1) * pu;
            xa[q] = Ak[ro + ca];
            xb[q] = Bk[ro + cb];
        }
    };
    auto stage = [&](int m0, const double (&xa)[Cfg::LPT], const double (&xb)[Cfg::LPT]) {
#pragma unroll
        for (int q = 0; q < Cfg::LPT; ++q) {
            const int row = lrow + q * RSTEP;
            const bool in = (m0 + row) < p;
            As[row * Cfg::LDS_LD + lcol] = (in && aok) ? xa[q] : 0.0;
            Bs[row * Cfg::LDS_LD + lcol] = (in && bok) ? xb[q] : 0.0;
        }
    };
    // all fragment reads of the slab first, then the MFMAs back to back: one LDS round trip per slab
    // instead of one per k-quad
    // nq: k-quads of the slab that lie inside the matrix (the last slab of p = 200 at BK = 32 has 2 of 8)
    auto compute = [&](int nq) {
        double af[BK / 4][Cfg::TI], bf[BK / 4][Cfg::TJ];
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk >= nq) break;
            const int row = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i) af[kk][i] = As[row * Cfg::LDS_LD + wr + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < Cfg::TJ; ++j) bf[kk][j] = Bs[row * Cfg::LDS_LD + wc + j * 16 + (lane & 15)];
        }
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            if (kk >= nq) break;
#pragma unroll
            for (int i = 0; i < Cfg::TI; ++i)
#pragma unroll
                for (int j = 0; j < Cfg::TJ; ++j) {
                    if (ABL == 2) { acc[i][j][0] += af[kk][i] * bf[kk][j]; continue; }   // ablation: no MFMA
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk][i], bf[kk][j], acc[i][j], 0, 0, 0);
                }
        }
    };

    // On a diagonal tile a wave whose sub-tile lies entirely below the diagonal produces nothing that is
    // kept (only gi <= gj survives there): it still stages and synchronises, but issues no MFMA.
    const bool dead_wave = (I == J) && (wr >= wc + WN);
#pragma unroll
    for (int s = 0; s < NST; ++s) fetch(s * BK, ra[s], rb[s]);
#ifdef GGL_DEV
    if (ABL == 3) t_loop = clock64();
#endif
    for (int m0 = 0; m0 < p; m0 += NST * BK) {
#pragma unroll
        for (int s = 0; s < NST; ++s) {
            const int ms = m0 + s * BK;
            if (ms < p) {                                   // uniform over the workgroup
                if (ABL != 4) stage(ms, ra[s], rb[s]);       // ABL 4: ds_read + MFMA only; ABL 5: + ds_write
                if (ABL != 4 && ABL != 5) __syncthreads();
                fetch(ms + NST * BK, ra[s], rb[s]);          // past the end: clamped, never staged
                if (!dead_wave) compute(min(BK / 4, (p - ms + 3) / 4));
                if (ABL != 4 && ABL != 5) __syncthreads();
            }
        }
    }

#ifdef GGL_DEV
    if (ABL == 3) t_loop_end = clock64();
#endif
    // epilogue.  C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
    const double cI = coef[k * NS_NCOEF + 0], cAcc = coef[k * NS_NCOEF + 1], cE = coef[k * NS_NCOEF + 2];
    const double dI = coef[k * NS_NCOEF + 3], dC = coef[k * NS_NCOEF + 4], dE = coef[k * NS_NCOEF + 5];
    double* Ck = (second ? C1 : C) + (size_t)kk * pp;
    double* C2k = (C2 && !second) ? C2 + (size_t)kk * pp : nullptr;
    const double* Ek = (E && !second) ? E + (size_t)kk * pp : nullptr;
    const double* E2k = (E2 && !second) ? E2 + (size_t)kk * pp : nullptr;     // second affine operand, added last
    const double cE2 = E2k ? coef[k * NS_NCOEF + 6] : 0.0, dE2 = E2k ? coef[k * NS_NCOEF + 7] : 0.0;
#pragma unroll
    for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < Cfg::TJ; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wr + ti * 16 + (lane >> 4) + 4 * r;
                const int col = wc + tj * 16 + (lane & 15);
                const int gi = I0 + row, gj = J0 + col;
                double v = cAcc * acc[ti][tj][r];
                const bool in = gi < p && gj < p;
                if (in && (I != J || gi <= gj)) {
                    if (gi == gj) v += cI;
                    const double e0 = Ek ? Ek[(size_t)gi * p + gj] : 0.0;
                    v += cE * e0;
                    const double f0 = E2k ? E2k[(size_t)gi * p + gj] : 0.0;
                    if (E2k) v += cE2 * f0;
                    Ck[(size_t)gi * p + gj] = v;
                    if (C2k) C2k[(size_t)gi * p + gj] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0) + (gi == gj ? dI : 0.0);
                    // mirrored store.  Diagonal tiles: only the upper triangle is kept, so the result is
                    // bitwise symmetric even though A != B.  Off-diagonal tiles without the LDS transpose:
                    // the four r-values of a lane quad complete a 128-B line.
                    if ((I == J && gi != gj) || (!LM && I != J)) {
                        Ck[(size_t)gj * p + gi] = v;
                        if (C2k) C2k[(size_t)gj * p + gi] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0);
                    }
                }
                if (LM && I != J) smem[row * Cfg::CLD + col] = v;
            }
    if (maxdev && ABL != 3) {
        double dev = 0.0;
#pragma unroll
        for (int ti = 0; ti < Cfg::TI; ++ti)
#pragma unroll
            for (int tj = 0; tj < Cfg::TJ; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * r;
                    const int gj = J0 + wc + tj * 16 + (lane & 15);
                    if (gi < p && gj < p && (I != J || gi <= gj)) {
                        double v = cAcc * acc[ti][tj][r] + (gi == gj ? cI - 1.0 : 0.0);
                        if (Ek) v += cE * Ek[(size_t)gi * p + gj];      // the deviation of the OUTPUT, E term included
                        if (E2k) v += cE2 * E2k[(size_t)gi * p + gj];
                        dev = fmax(dev, fabs(v));
                    }
                }
        dev = wave_max(dev);
        if (lane == 0 && dev > 0.0)
            atomicMax(reinterpret_cast<unsigned long long*>(maxdev + k), (unsigned long long)__double_as_longlong(dev));
    }
    if (LM && I != J) {
        __syncthreads();
        for (int e = tid; e < BM * BM; e += Cfg::NT) {
            const int a = e / BM, c = e % BM;   // out[J0+a][I0+c] = tile[c][a]
            if (J0 + a < p && I0 + c < p) {
                const double v = smem[c * Cfg::CLD + a];
                Ck[(size_t)(J0 + a) * p + I0 + c] = v;
                if (C2k) {
                    // E is bitwise symmetric (an output of this kernel family): its mirrored entry IS the upper one
                    const double e0 = (dE != 0.0 && Ek) ? Ek[(size_t)(J0 + a) * p + I0 + c] : 0.0;
                    const double f0 = E2k ? E2k[(size_t)(J0 + a) * p + I0 + c] : 0.0;
                    C2k[(size_t)(J0 + a) * p + I0 + c] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0);
                }
            }
        }
    }
#ifdef GGL_DEV
    if (ABL == 3 && tid == 0) {
        // timeline probe: maxdev is (ab)used as a [gridDim.x][5] long long buffer
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        long long* tl = reinterpret_cast<long long*>(maxdev) + (size_t)blockIdx.x * 5;
        unsigned xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        tl[0] = t_start; tl[1] = t_loop; tl[2] = t_loop_end; tl[3] = clock64(); tl[4] = (long long)xcc;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// k_symm_dl: the same symmetric product with the operand slabs DMA'd straight into LDS
// (global_load_lds, 16 bytes per lane, no VGPR round trip and no ds_write pass) and a double-buffered
// LDS image, one barrier per k-slab.  64x64 tile, 4 waves (32x32 each), k-slab 16.
//   * one wave instruction moves 1 KiB = two 64-double rows; its LDS destination is wave-linear
//     (base + lane*16), so the slab is stored unpadded [16][64]; rows r and r+1 would put the two 16-lane
//     groups of a half wave on the same banks, so odd rows are stored with their 16-double halves
//     swapped -- done on the SOURCE address (the DMA cannot scatter), and undone in the fragment read.
//   * needs 16-byte aligned rows: p even (odd p takes k_symm_tn).  Out-of-range columns read a
//     clamped address (their products only reach outputs that are never stored); out-of-range k-rows of
//     the last slab are zeroed in LDS after the DMA has landed.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int N> __device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N <= 63, "vmcnt range");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else static_assert(N == 0, "add the immediate");
}

// BK: k-slab depth (16 or 32); NSTG: slabs resident in LDS (2 = double buffer; more = deeper DMA prefetch)
// BM: tile edge (64, or 32 for under-filled batches: 4x the workgroups, and with NSTG = 4 enough slabs in flight to
// cover the load latency that bounds the small-batch regime); ABL 1: no mirror write (timing ablation)
// NW: waves per workgroup (4: 2 x 2 waves of BM/2 x BM/2; 8: 4 x 2 waves of BM/4 x BM/2 -- two waves per SIMD, for batches
// so small that only one workgroup lands on a CU and a lone wave per SIMD cannot hide its LDS round trips and barriers)
// symm_dl_tile: one output tile (instance k of the combined batch, tile pair b) -- the whole body of k_symm_dl
// SER 1: the serial epilogue instead of the batched one, SER 2: the batched one with every off-diagonal tile staged in LDS
// (0: those of launches without bound partials are written from registers); 1 and 2 development library only

// one scalar load of the serial epilogue (SER 1, development library).  A function on purpose: with the subscript written out
// the compiler lays that epilogue's branches out differently -- same arithmetic, other machine code in 21 SER 1 instances --
// and the serial epilogue is the bitwise yardstick, kept exactly as measured
__device__ __forceinline__ double ld1(const double* p) { return *p; }

// the bound partials of one staged tile (symm_dl_tile: rowpart / fropart), by the first 2 BM threads of the workgroup
template <int BM>
__device__ __forceinline__ void symm_dl_partials(const double* smem, double* __restrict__ rowpart, double* __restrict__ fropart,
                                                 int k, int p, int T, int blockTile, int I, int J, int I0, int J0, int tid)
{
    // threads 0..BM-1: row t of the staged tile; threads BM..2BM-1 (off-diagonal tiles): column t of it, i.e. row
    // J0+t of the mirrored tile.  A diagonal tile holds its upper triangle U only: row t of the full symmetric tile
    // is row t of U plus column t of U minus the diagonal entry.
    const int t = tid & (BM - 1);
    const bool second = tid >= BM;
    const size_t slot_stride = (size_t)p;
    double rs = 0.0, sq = 0.0;
    if (!second) {
#pragma unroll 8
        for (int c = 0; c < BM; ++c) { const double x = smem[t * BM + (c ^ t)]; rs += fabs(x); sq += x * x; }
    }
    if (second || I == J) {
        double cs = 0.0;
#pragma unroll 8
        for (int r = 0; r < BM; ++r) cs += fabs(smem[r * BM + (t ^ r)]);
        if (I == J) {
            if (!second) {
                const double dg = smem[t * BM];
                rs = (rs + cs) - fabs(dg);
                sq = 2.0 * sq - dg * dg;
            }
        } else {
            rs = cs;
        }
    } else {
        sq *= 2.0;            // off-diagonal tile: its mirror has the same squares
    }
    if (I != J || !second) {
        const int T2 = (p + BM - 1) / BM;
        const int slot = second ? I : J, gi = (second ? J0 : I0) + t;
        if (gi < p) rowpart[((size_t)k * T2 + slot) * slot_stride + gi] = rs;
    }
    if (tid < 64) {                      // wave 0 holds the BM row threads
        sq = wave_sum((tid < BM) ? sq : 0.0);
        if (tid == 0) fropart[(size_t)k * (T * (T + 1) / 2) + blockTile] = sq;
    }

}

template <int BK, int NSTG, int ABL, int BM, int NW, int SER = 0>
__device__ __forceinline__ void symm_dl_tile(const double* __restrict__ A, const double* __restrict__ B,
                                             double* __restrict__ C, double* __restrict__ C2,
                                             const double* __restrict__ E, const double* __restrict__ E2,
                                             const double* __restrict__ coef, int K,
                                             int p, const double* __restrict__ A1, const double* __restrict__ B1,
                                             double* __restrict__ C1, int K1, double* __restrict__ maxdev,
                                             double* __restrict__ rowpart, double* __restrict__ fropart, int k, int b,
                                             double* smem)
{
    // smem: the caller's NSTG * 2 * BK * BM doubles of LDS ([buf][A|B][BK][BM]; later the mirror tile)
    // rowpart / fropart != null: the launch also leaves what a spectral bound of C needs, with no pass over C --
    // rowpart[k][s][i] = sum over the columns of tile-column s of |C[i][.]| (summed over s: the row sums of |C|) and
    // fropart[k][tile] = the tile's share of |C|_F^2 (mirror included), every slot written by exactly one workgroup
    constexpr int NT = NW * 64;
    constexpr int WM = BM / (NW / 2), WN = BM / 2, TI = WM / 16, TJ = WN / 16;
    constexpr int RPI = 128 / BM;                        // slab rows per DMA instruction (1 KiB)
    constexpr int LPR = 64 / RPI;                        // lanes per row
    constexpr int SLAB = BK * BM;                        // doubles per operand slab (8 KiB at BK = 16)
    constexpr int IPW = BK / (NW * RPI);                 // DMA instructions per wave, operand and slab
    constexpr int RPW = BK / NW;                         // slab rows a wave's DMA writes
    static_assert(NW == 4 || NW == 8, "waves per workgroup");
    static_assert(TI >= 1 && TJ >= 1, "wave tile");
    static_assert(BM == 64 || BM == 32, "tile edge");
    static_assert(IPW >= 1, "k-slab too shallow for this tile");
    static_assert(NSTG * 2 * SLAB >= BM * BM, "the mirror tile reuses the slab storage");
    const int T = (p + BM - 1) / BM;
    const int blockTile = b;
    const bool second = k >= K;
    const int kk = second ? k - K : k;
    int I = 0;
    while (b >= T - I) { b -= T - I; ++I; }
    const int J = I + b;
    const int I0 = I * BM, J0 = J * BM;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // wave-uniform: everything derived from it is scalar
    const int wr = (wave >> 1) * WM, wc = (wave & 1) * WN;
    const size_t pp = (size_t)p * p;
    const double* Ak = (second ? A1 : A) + (size_t)kk * pp;
    const double* Bk = (second ? B1 : B) + (size_t)kk * pp;

    v4d acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    // DMA geometry: wave w issues instructions i = 2w, 2w+1 per operand; instruction i covers slab rows
    // 2i, 2i+1; lane l -> row 2i + (l >> 5), LDS position (l & 31) * 2, source column position ^ 16*(row & 1).
    // The per-lane source pointers are kept for the NEXT slab to be issued and advanced by BK rows per slab: every vector
    // instruction beside an MFMA takes matrix-pipe issue slots (tools/probe_mfma_mix.py: 2 integer VALU per MFMA cost 11 % of
    // the FP64 MFMA rate, 8 cost 17 %), and recomputing min / mul / 64-bit adds per instruction was ~25 of them per slab.
    // Only the last, partial slab (rows beyond the matrix clamped to its last row) goes the long way.
    // (pm2: the last column PAIR a lane may start at -- p - 2 for even p; for odd p the pair (p - 1, p), whose second half is
    // the first element of the next row: in the stack for every row but the last row of the last instance, where it is the 8
    // bytes behind the stack -- every stack that can be an operand is allocated with that slack, stack_bytes())
    const unsigned pu = (unsigned)p, pm1 = (unsigned)(p - 1), pm2 = (unsigned)(p - 1) & ~1u;
    const int lrow = lane / LPR;
    const unsigned cpos = (unsigned)((lane % LPR) * 2) ^ (unsigned)(16 * (lrow & 1));
    const unsigned ca = min((unsigned)I0 + cpos, pm2), cb = min((unsigned)J0 + cpos, pm2);
    const double* pa[IPW];
    const double* pb[IPW];
#pragma unroll
    for (int j = 0; j < IPW; ++j) {
        const unsigned r0 = min((unsigned)(RPI * (wave * IPW + j) + lrow), pm1);
        pa[j] = Ak + (size_t)r0 * pu + ca;
        pb[j] = Bk + (size_t)r0 * pu + cb;
    }
    const size_t slab_step = (size_t)BK * pu;
    const int Sfull = p / BK;                                            // slabs that lie inside the matrix entirely
    auto issue = [&](int sidx, int buf) {                                // slabs are issued in increasing order
        if (ABL == 2) return;                                            // timing ablation: no operand loads at all
        double* base = smem + (size_t)buf * 2 * SLAB + (wave * IPW) * 128;   // wave-uniform LDS base
        if (sidx < Sfull) {
#pragma unroll
            for (int j = 0; j < IPW; ++j) {
                double* la = base + j * 128;
                __builtin_amdgcn_global_load_lds((gptr_t)pa[j], (lptr_t)la, 16, 0, 0);
                __builtin_amdgcn_global_load_lds((gptr_t)pb[j], (lptr_t)(la + SLAB), 16, 0, 0);
                pa[j] += slab_step;
                pb[j] += slab_step;
            }
        } else {
            const int m0 = sidx * BK;
#pragma unroll
            for (int j = 0; j < IPW; ++j) {
                const int i = wave * IPW + j;
                const unsigned ro = min((unsigned)(m0 + RPI * i + lrow), pm1) * pu;
                double* la = base + j * 128;
                __builtin_amdgcn_global_load_lds((gptr_t)(Ak + ro + ca), (lptr_t)la, 16, 0, 0);
                __builtin_amdgcn_global_load_lds((gptr_t)(Bk + ro + cb), (lptr_t)(la + SLAB), 16, 0, 0);
            }
        }
    };
    // Which 16x16 blocks this wave owns.  acc[i][j] belongs to rows rbk[i].., columns cbk[j].. of the tile and the MFMAs
    // of a k-quad run in the order X = acc[0][0], Y = acc[0][1], Z = acc[1][1], U = acc[1][0].  Off-diagonal tiles: the
    // wave's own 32x32 quadrant, all four.  A DIAGONAL tile is written from its upper triangle (in-tile mirror), i.e. 10
    // of its 16 blocks: the two diagonal quadrants need X, Y, Z (U lies below the diagonal); the upper-right quadrant needs
    // all four, and the wave of the lower-left quadrant would have nothing to do -- it takes that quadrant's block (1,1)
    // instead, and the quadrant's own wave names its column blocks the other way round so that what is left to it is again
    // X, Y, Z.  Every wave of a diagonal tile then skips U: 3 MFMAs per k-quad instead of 4 on the 8 diagonal tiles of the
    // 36 of a p = 500 product, for ONE wave-uniform branch per k-quad (the fourth wave runs Y and Z on accumulators nobody
    // reads: its SIMD would otherwise idle).  Where that branch sits matters more than what it saves: U is issued FIRST,
    // straight behind the k-quad's exit check (two adjacent scalar branches: +1.9 % at the headline, 0.0 % at p = 1000);
    // behind X, Y, Z, or as X / branch / Y Z / branch / U, the off-diagonal tiles lose 0.8-1.5 % at p = 1000, and a
    // separate copy of the k-quad loop for the partial waves makes the allocator shuffle the accumulators between the two
    // (-21 %).  In-box A/B: profiles/r3_product_kernel_round3.txt.  Same blocks, same k order: same bits.
    constexpr bool REBAL = (TI == 2 && TJ == 2 && NW == 4);
    int rbk[TI], cbk[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) rbk[i] = wr + 16 * i;
#pragma unroll
    for (int j = 0; j < TJ; ++j) cbk[j] = wc + 16 * j;
    const bool skipU = REBAL && I == J;
    int nval = TI * TJ;                                   // accumulators that hold blocks of the tile: X [, Y, Z [, U]]
    if (skipU) {
        nval = 3;
        if (wave == 1) { cbk[0] = wc + 16; cbk[TJ - 1] = wc; }                                   // X=(0,3) Y=(0,2) Z=(1,2)
        else if (wave == 2) { rbk[0] = 16; rbk[TI - 1] = 0; cbk[0] = WN + 16; cbk[TJ - 1] = WN; nval = 1; }   // X=(1,3)
    }
    const bool dead_wave = !REBAL && (I == J) && (wr >= wc + WN);
    // Epilogue operands.  The batched epilogue (SER != 1) fetches its coefficients HERE, ahead of the slab loop: eight scalar
    // loads whose latency the loop hides, instead of a scalar round trip between the last MFMA and the first epilogue load.
    double cI = 0.0, cAcc = 0.0, cE = 0.0, dI = 0.0, dC = 0.0, dE = 0.0, cE2 = 0.0, dE2 = 0.0;
    double* Ck = (second ? C1 : C) + (size_t)kk * pp;
    double* C2k = (C2 && !second) ? C2 + (size_t)kk * pp : nullptr;
    const double* Ek = (E && !second) ? E + (size_t)kk * pp : nullptr;
    // second affine operand (E2, coefficients cE2 / dE2): added after the E term, so a launch without it keeps its bits
    const double* E2k = (E2 && !second) ? E2 + (size_t)kk * pp : nullptr;
    auto load_coefs = [&] {
        cI = coef[k * NS_NCOEF + 0]; cAcc = coef[k * NS_NCOEF + 1]; cE = coef[k * NS_NCOEF + 2];
        dI = coef[k * NS_NCOEF + 3]; dC = coef[k * NS_NCOEF + 4]; dE = coef[k * NS_NCOEF + 5];
        cE2 = E2k ? coef[k * NS_NCOEF + 6] : 0.0; dE2 = E2k ? coef[k * NS_NCOEF + 7] : 0.0;
    };
    if constexpr (SER != 1 && ABL != 4) load_coefs();
    const int S = (p + BK - 1) / BK;
#pragma unroll
    for (int q = 0; q < NSTG - 1; ++q)
        if (q < S) issue(q, q);
    // per-lane LDS positions of the wave's fragments in k-quad 0 of a slab image: row (lane >> 4), column XOR-swizzled by the
    // row's parity -- rows of k-quad q are 4q + (lane >> 4), same parity -- so every fragment read of the slab loop is one
    // of these bases plus a COMPILE-TIME offset (stage, operand, k-quad): the loop is unrolled over the NSTG stages to make
    // the stage a constant, and the fragment reads carry no address arithmetic at all (see the note on issue slots above)
    const int fg = lane >> 4, fsw = 16 * (fg & 1);
    const double* pfa[TI];
    const double* pfb[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) pfa[i] = smem + fg * BM + ((rbk[i] + (lane & 15)) ^ fsw);
#pragma unroll
    for (int j = 0; j < TJ; ++j) pfb[j] = smem + SLAB + fg * BM + ((cbk[j] + (lane & 15)) ^ fsw);
    auto slab = [&](const int s, auto bufc) {
        constexpr int buf = decltype(bufc)::value;
        // this wave's DMA of slab s has landed: at most the later slabs' instructions may still be in flight
        const int ahead = min(NSTG - 2, S - 1 - s);
        if (NSTG >= 6 && ahead >= 4) wait_vmcnt<(NSTG >= 6 ? 8 * IPW : 0)>();
        else if (NSTG >= 5 && ahead >= 3) wait_vmcnt<(NSTG >= 5 ? 6 * IPW : 0)>();
        else if (NSTG >= 4 && ahead >= 2) wait_vmcnt<4 * IPW>();
        else if (NSTG >= 3 && ahead >= 1) wait_vmcnt<2 * IPW>();
        else wait_vmcnt<0>();
        const int valid = p - s * BK;                          // k-rows of this slab inside the matrix
        if (valid < BK) {
            // zero the rows beyond the matrix (each wave cleans the rows its own DMA wrote)
            for (int e = lane; e < RPW * BM; e += 64) {
                const int row = wave * RPW + e / BM;
                if (row >= valid) {
                    smem[(size_t)buf * 2 * SLAB + row * BM + (e % BM)] = 0.0;
                    smem[(size_t)buf * 2 * SLAB + SLAB + row * BM + (e % BM)] = 0.0;
                }
            }
        }
        // slab s visible to all, slab s-1 fully consumed.  A raw barrier with an LDS-only wait: __syncthreads() would
        // make hipcc drain vmcnt(0) here, i.e. wait for the slabs prefetched AHEAD as well and collapse the pipeline
        // to one slab of overlap whatever NSTG is (this wave's own slab-s DMA was waited for by the counted vmcnt above)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (ABL != 5) __builtin_amdgcn_s_barrier();                      // ABL 5: no slab barrier (timing ablation)
        asm volatile("" ::: "memory");
        if (s + NSTG - 1 < S) issue(s + NSTG - 1, (buf + NSTG - 1) % NSTG);
        if (!dead_wave) {
            const int nq = min(BK / 4, (valid + 3) / 4);      // k-quads inside the matrix (last slab: 1 of 4 at p = 500)
            // (The exit check between the k-quads stays even for slabs that lie inside the matrix.  Straight-line code --
            // with the compiler's own order, ds_read2st64 pairs ahead of 8 back-to-back MFMAs, or with a scheduling barrier
            // per k-quad that keeps read 4 / issue 4 -- measured 8-9 % SLOWER at the headline, in-box A/B: the scalar
            // branch is where a wave lets the other waves of its SIMD in.)
#pragma unroll
            for (int kq4 = 0; kq4 < BK / 4; ++kq4) {
                if (kq4 >= nq) break;
                constexpr int so = buf * 2 * SLAB;
                double af[TI], bf[TJ];
#pragma unroll
                for (int i = 0; i < TI; ++i) af[i] = pfa[i][so + kq4 * 4 * BM];
#pragma unroll
                for (int j = 0; j < TJ; ++j) bf[j] = pfb[j][so + kq4 * 4 * BM];
                if constexpr (REBAL && ABL != 3) {
                    if (!skipU) acc[TI - 1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[TI - 1], bf[0], acc[TI - 1][0], 0, 0, 0);
                    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[0], bf[0], acc[0][0], 0, 0, 0);
                    acc[0][TJ - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[0], bf[TJ - 1], acc[0][TJ - 1], 0, 0, 0);
                    acc[TI - 1][TJ - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[TI - 1], bf[TJ - 1], acc[TI - 1][TJ - 1], 0, 0, 0);
                } else {
#pragma unroll
                    for (int i = 0; i < TI; ++i)
#pragma unroll
                        for (int j = 0; j < TJ; ++j) {
                            if (ABL == 3) { acc[i][j][0] += af[i] * bf[j]; continue; }   // timing ablation: no MFMA
                            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
                        }
                }
            }
        }
    };
    auto stages = [&](const int s0, auto... bufs) {
        (void)std::initializer_list<int>{((s0 + (int)decltype(bufs)::value < S) ? (slab(s0 + (int)decltype(bufs)::value, bufs), 0) : 0)...};
    };
    static_assert(NSTG == 2 || NSTG == 3 || NSTG == 4 || NSTG == 6, "stage counts with an unrolled slab loop");
    for (int s0 = 0; s0 < S; s0 += NSTG) {
        if constexpr (NSTG == 2) stages(s0, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
        else if constexpr (NSTG == 3) stages(s0, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
        else if constexpr (NSTG == 4) stages(s0, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{});
        else stages(s0, std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{}, std::integral_constant<int, 3>{}, std::integral_constant<int, 4>{}, std::integral_constant<int, 5>{});
    }
    // all fragment reads done before the slabs are reused as the mirror tile (the batched epilogue has this barrier behind
    // its first loads, see there)
    if constexpr (ABL == 4 || SER == 1) __syncthreads();
    if (ABL == 4) {                                                      // timing ablation: no epilogue
        double keepalive = 0.0;
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) keepalive += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
        if (keepalive == 1234.5678) C[0] = keepalive;
        return;
    }

#ifdef GGL_DEV
    if constexpr (SER == 1) {
        // the serial epilogue (development library, ggl_dev_set_symm_epilogue): the bitwise yardstick of
        // the batched one below and the other side of its A/B -- one global round trip per trip of every pass
        load_coefs();
        double dev = 0.0;
        // Off-diagonal tiles: the accumulators go to the (XOR-swizzled) LDS tile first and BOTH copies -- the tile and its
        // mirror -- are written from there with 16-byte accesses, two consecutive columns per lane (p is even, tile columns start
        // on even indices): half the global store / E-load instructions of the layout the MFMA leaves the values in (one column
        // per lane: 8-byte accesses, which run at 0.54-0.70x the 16-byte rate on this chip).  Same arithmetic per element
        // (cAcc * acc, then + cE * E): same bits.  Diagonal tiles keep the direct path (upper triangle only, in-tile mirror).
        const bool wide = (I != J) && ABL != 1;
        if (wide) {
    #pragma unroll
            for (int ti = 0; ti < TI; ++ti)
    #pragma unroll
                for (int tj = 0; tj < TJ; ++tj)
    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = wr + ti * 16 + (lane >> 4) + 4 * r;
                        const int col = wc + tj * 16 + (lane & 15);
                        smem[row * BM + (col ^ row)] = cAcc * acc[ti][tj][r];
                    }
            __syncthreads();
            auto ld2 = [](const double* q) { return *reinterpret_cast<const double2*>(q); };
            auto lde2 = [](const double* q) { return *reinterpret_cast<const double2*>(q); };
            for (int e2 = tid; e2 < BM * BM / 2; e2 += NT) {
                const int row = e2 / (BM / 2), c2 = (e2 % (BM / 2)) * 2;
                const int gi = I0 + row, gj = J0 + c2;
                // columns c2, c2 + 1 of row `row` sit at (c2 ^ row), (c2 ^ row) ^ 1: one aligned pair, swapped for odd rows
                double2 t = ld2(smem + row * BM + ((c2 ^ row) & ~1));
                if (row & 1) { const double h = t.x; t.x = t.y; t.y = h; }
                if (gi < p && gj + 1 < p) {
                    double2 e = {0.0, 0.0}, f = {0.0, 0.0};
                    if (Ek) e = lde2(Ek + (size_t)gi * p + gj);
                    if (E2k) f = lde2(E2k + (size_t)gi * p + gj);
                    double2 v;
                    v.x = t.x + cE * e.x;
                    v.y = t.y + cE * e.y;
                    if (E2k) { v.x += cE2 * f.x; v.y += cE2 * f.y; }
                    dev = fmax(dev, fmax(fabs(v.x), fabs(v.y)));
                    *reinterpret_cast<double2*>(Ck + (size_t)gi * p + gj) = v;
                    if (C2k) {
                        double2 w;
                        w.x = c2val(dC, v.x, dE, e.x);
                        w.y = c2val(dC, v.y, dE, e.y);
                        if (E2k) { w.x = __builtin_fma(dE2, f.x, w.x); w.y = __builtin_fma(dE2, f.y, w.y); }
                        *reinterpret_cast<double2*>(C2k + (size_t)gi * p + gj) = w;
                    }
                    if (rowpart) {          // the bound partials (and then the mirror) read the FINAL values from the tile
                        if (row & 1) { const double h = v.x; v.x = v.y; v.y = h; }
                        *reinterpret_cast<double2*>(smem + row * BM + ((c2 ^ row) & ~1)) = v;
                    }
                } else if (gi < p && gj < p) {
                    // odd p: the last column is the first half of a pair whose second half lies outside the matrix
                    const double e0 = Ek ? ld1(Ek + (size_t)gi * p + gj) : 0.0;
                    const double f0 = E2k ? ld1(E2k + (size_t)gi * p + gj) : 0.0;
                    double v0 = t.x + cE * e0;
                    if (E2k) v0 += cE2 * f0;
                    dev = fmax(dev, fabs(v0));
                    Ck[(size_t)gi * p + gj] = v0;
                    if (C2k) C2k[(size_t)gi * p + gj] = c2val2(dC, v0, dE, e0, E2k != nullptr, dE2, f0);
                    if (rowpart) {
                        double2 v = {v0, 0.0};
                        if (row & 1) { v.x = 0.0; v.y = v0; }
                        *reinterpret_cast<double2*>(smem + row * BM + ((c2 ^ row) & ~1)) = v;
                    }
                } else if (rowpart) {
                    *reinterpret_cast<double2*>(smem + row * BM + ((c2 ^ row) & ~1)) = double2{0.0, 0.0};
                }
            }
        } else {
        if (REBAL && I == J && rowpart && ABL != 1) {
            // the staged tile of the bound partials wants zeros below the diagonal: the six blocks no wave owns any more
            for (int e = tid; e < 6 * 256; e += NT) {
                const int blk = e >> 8, br = (blk < 1) ? 1 : (blk < 3 ? 2 : 3), bc = blk - (br == 1 ? 0 : (br == 2 ? 1 : 3));
                const int row = br * 16 + ((e >> 4) & 15), col = bc * 16 + (e & 15);
                smem[row * BM + (col ^ row)] = 0.0;
            }
        }
    #pragma unroll
        for (int ti = 0; ti < TI; ++ti)
    #pragma unroll
            for (int tj = 0; tj < TJ; ++tj) {
                if (REBAL && ((ti != tj && tj == 0 && nval <= 3) || ((ti | tj) != 0 && nval <= 1))) continue;   // not a block of the tile
    #pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rbk[ti] + (lane >> 4) + 4 * r;
                    const int col = cbk[tj] + (lane & 15);
                    const int gi = I0 + row, gj = J0 + col;
                    double v = cAcc * acc[ti][tj][r];
                    const bool keep = gi < p && gj < p && (I != J || gi <= gj);
                    if (keep) {
                        if (gi == gj) v += cI;
                        const double e0 = Ek ? ld1(Ek + (size_t)gi * p + gj) : 0.0;
                        v += cE * e0;
                        const double f0 = E2k ? ld1(E2k + (size_t)gi * p + gj) : 0.0;
                        if (E2k) v += cE2 * f0;
                        dev = fmax(dev, fabs(v - (gi == gj ? 1.0 : 0.0)));
                        Ck[(size_t)gi * p + gj] = v;
                        if (C2k) C2k[(size_t)gi * p + gj] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0) + (gi == gj ? dI : 0.0);
                        if (I == J && gi != gj) {
                            Ck[(size_t)gj * p + gi] = v;
                            if (C2k) C2k[(size_t)gj * p + gi] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0);
                        }
                    }
                    // XOR-swizzled BM x BM tile in LDS: the mirror pass of an off-diagonal tile reads it transposed; with
                    // bound partials every tile is staged (entries that are not stored count as zero)
                    if ((I != J || rowpart) && ABL != 1) smem[row * BM + (col ^ row)] = (rowpart && !keep) ? 0.0 : v;
                }
            }
        }
        if (maxdev) {
            dev = wave_max(dev);
            if (lane == 0 && dev > 0.0)
                atomicMax(reinterpret_cast<unsigned long long*>(maxdev + k), (unsigned long long)__double_as_longlong(dev));
        }
        if (((I != J && !wide) || rowpart) && ABL != 1) __syncthreads();
        if (rowpart && ABL != 1 && tid < 2 * BM) symm_dl_partials<BM>(smem, rowpart, fropart, k, p, T, blockTile, I, J, I0, J0, tid);
        if (wide) {
            // the mirror: row a of it is column a of the staged tile; two consecutive columns c2, c2 + 1 per lane.  Without bound
            // partials the tile still holds cAcc * acc and the E term is added here as well (E is bitwise symmetric -- an output
            // of this kernel family -- so its mirrored entries ARE the upper ones); with them it holds the final values.
            auto lde2 = [](const double* q) { return *reinterpret_cast<const double2*>(q); };
            for (int e2 = tid; e2 < BM * BM / 2; e2 += NT) {
                const int a = e2 / (BM / 2), c2 = (e2 % (BM / 2)) * 2;      // out[J0+a][I0+c2 .. +1] = tile[c2 .. +1][a]
                if (J0 + a < p && I0 + c2 + 1 < p) {
                    double2 v;
                    v.x = smem[c2 * BM + (a ^ c2)];
                    v.y = smem[(c2 + 1) * BM + (a ^ (c2 + 1))];
                    double2 e = {0.0, 0.0}, f = {0.0, 0.0};
                    const bool need_e = Ek && (!rowpart || (C2k && dE != 0.0));
                    if (need_e) e = lde2(Ek + (size_t)(J0 + a) * p + I0 + c2);
                    const bool need_f = E2k && (!rowpart || (C2k && dE2 != 0.0));
                    if (need_f) f = lde2(E2k + (size_t)(J0 + a) * p + I0 + c2);
                    if (!rowpart) {
                        v.x += cE * e.x; v.y += cE * e.y;
                        if (E2k) { v.x += cE2 * f.x; v.y += cE2 * f.y; }
                    }
                    *reinterpret_cast<double2*>(Ck + (size_t)(J0 + a) * p + I0 + c2) = v;
                    if (C2k) {
                        double2 w;
                        w.x = c2val(dC, v.x, dE, e.x);
                        w.y = c2val(dC, v.y, dE, e.y);
                        if (E2k) { w.x = __builtin_fma(dE2, f.x, w.x); w.y = __builtin_fma(dE2, f.y, w.y); }
                        *reinterpret_cast<double2*>(C2k + (size_t)(J0 + a) * p + I0 + c2) = w;
                    }
                } else if (J0 + a < p && I0 + c2 < p) {
                    // (never taken: I < J, so the rows I0 .. I0 + BM - 1 of an off-diagonal tile all lie inside the matrix and an
                    // odd last column can only belong to tile column J; kept so that the pair test above stands on its own)
                    double v0 = smem[c2 * BM + (a ^ c2)];
                    const bool need_e = Ek && (!rowpart || (C2k && dE != 0.0));
                    const double e0 = need_e ? ld1(Ek + (size_t)(J0 + a) * p + I0 + c2) : 0.0;
                    const bool need_f = E2k && (!rowpart || (C2k && dE2 != 0.0));
                    const double f0 = need_f ? ld1(E2k + (size_t)(J0 + a) * p + I0 + c2) : 0.0;
                    if (!rowpart) { v0 += cE * e0; if (E2k) v0 += cE2 * f0; }
                    Ck[(size_t)(J0 + a) * p + I0 + c2] = v0;
                    if (C2k) C2k[(size_t)(J0 + a) * p + I0 + c2] = c2val2(dC, v0, dE, e0, E2k != nullptr, dE2, f0);
                }
            }
        }
        return;
    }
#endif
    // The batched epilogue.  The serial one paid a dependent global round trip per trip of every pass -- load E, load E2,
    // s_waitcnt vmcnt(0) (which also waits for the previous trip's store acknowledgements), store -- about 16 of them per
    // tile, its four waves holding a third of the CU's LDS and issuing no MFMA meanwhile.  Here
    //   * the E / E2 loads of a whole batch of trips are issued back to back (NB trips of an off-diagonal tile, DB 16x16
    //     blocks of a diagonal one: as many as fit the register budget of the kernel's residency, VBUD), the FIRST batch
    //     ahead of the barrier that closes the slab loop, so that its latency runs under the barrier, the staging of the
    //     accumulators and the barrier behind it.  (It is issued after the slab loop, i.e. after the last slab's vmcnt(0):
    //     the loop's counted wait_vmcnt<N> never see it.  Ahead of the last slab's MFMAs it would have to be counted into
    //     every immediate of the loop.)
    //   * the stores follow without a wait of their own: the compiler's counted vmcnt in front of a trip's arithmetic
    //     leaves the stores of the earlier trips in flight;
    //   * the barriers are LDS-only (lds_barrier): __syncthreads() drains vmcnt(0), i.e. loads AND store acknowledgements;
    //   * the direct pass writes the final values back to the staged tile and the mirror pass reads them from there: no
    //     second pass over E / E2 (they are bitwise symmetric -- outputs of this kernel family -- so the mirrored entry of
    //     the sum IS the upper one), except where the second output needs them, batched in the same way.
    // Same operations per element in the same order (the fused multiply-adds pinned with __builtin_fma): same bits.
    constexpr int LDSB = NSTG * 2 * SLAB * 8;
    constexpr int WGCU = (160 * 1024 / LDSB) < (8 / (NW / 4)) ? (160 * 1024 / LDSB) : (8 / (NW / 4));   // workgroups per CU
    constexpr int VBUD = (512 / (WGCU * (NW / 4))) & ~7;          // VGPRs per lane that keep that residency
    // of them, for loads in flight: what the accumulators and ~48 registers of addresses and values in work leave
    constexpr int BREG = VBUD - TI * TJ * 8 - 48;
    constexpr int NTRIP = BM * BM / 2 / NT;                       // trips of a pass over an off-diagonal tile
    constexpr int NB = (BREG / 8 >= NTRIP) ? NTRIP : (BREG / 8 >= NTRIP / 2 && NTRIP >= 2) ? NTRIP / 2 : 1;   // trips per batch (8 VGPRs each)
    constexpr int NBLK = TI * TJ;                                 // 16x16 blocks of a wave
    constexpr int DB = (BREG / 16 >= NBLK) ? NBLK : (BREG / 16 >= NBLK / 2 && NBLK >= 2) ? NBLK / 2 : 1;      // blocks per batch (16 VGPRs each)
    static_assert(NTRIP * NT * 2 == BM * BM && NTRIP % NB == 0 && NBLK % DB == 0, "epilogue batches");
    auto lds_barrier = [] {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // The ONE wait of a batch: an empty statement that reads the batch's registers, in workgroup-uniform control flow.  Left
    // to itself the compiler waits at the first use, which sits inside a lane-predicated region; behind such a region it no
    // longer knows what has landed and drains vmcnt(0) -- store acknowledgements included -- at every later trip.
    auto landed = [](const double& x) { asm volatile("" ::"v"(x)); };
    auto landed2 = [&](const double2& x) { landed(x.x); landed(x.y); };
    auto ld2 = [](const double* q) { return *reinterpret_cast<const double2*>(q); };
    auto lde2 = [](const double* q) { return *reinterpret_cast<const double2*>(q); };
    double dev = 0.0;
    // Off-diagonal tiles, staged (launches with bound partials, SER 2, and the instantiations the register path below leaves
    // out): the accumulators go to the (XOR-swizzled) LDS tile first and BOTH copies -- the tile and its
    // mirror -- are written from there with 16-byte accesses, two consecutive columns per lane (tile columns start on even
    // indices): half the global store / E-load instructions of the layout the MFMA leaves the values in (one column per
    // lane: 8-byte accesses, which run at 0.54-0.70x the 16-byte rate on this chip).  Diagonal tiles keep the direct path
    // (upper triangle only, in-tile mirror).
    const bool wide = (I != J) && ABL != 1;
    // The register epilogue (SER 0; SER 2 keeps the staged one selectable in the development library): an off-diagonal tile of
    // a launch without bound partials is written -- tile and mirror -- from the accumulator registers.  No LDS tile, no barrier
    // behind the slab loop (the slabs are not reused), every wave finishes on its own.
    // A 16x16 block leaves lane l with column c = l & 15, rows g + 4r (g = l >> 4, r = 0..3).
    //   * direct tile: lanes c and c ^ 1 exchange two of their four values; the even lane then holds rows g, g + 4 and the odd
    //     lane rows g + 8, g + 12 of the column PAIR (c & ~1, +1): trip h of a block is row g + 8 (c & 1) + 4h, one 16-byte
    //     load per operand and one 16-byte store per output, with the edge rules of the staged pass;
    //   * mirror: a lane's final pairs (x = first column, y = second) of the two trips h = 0, 1 are the rows g + 8 (c & 1) + 4h.
    //     Swapping the lane bit g & 1 with the register bit h -- v_permlane16_swap on the two trips' x and on their y -- leaves
    //     the lane with two CONSECUTIVE rows 2 (g >> 1) + 4 (g & 1) + 8 (c & 1) + 0, 1 of each of its two columns: 16 contiguous
    //     bytes of mirror row c & ~1 and 16 of the next one, and the eight lanes of a column pair cover 128 contiguous bytes
    //     of each -- per store instruction eight rows of 128 bytes, as in the direct pass.  (The 4 x 4 transpose with
    //     v_permlane32_swap as well gives a lane 32 contiguous bytes of ONE mirror row, but every one of its two stores then
    //     scatters 16-byte pieces 32 bytes apart, for twice the swaps.)  The second output is mirrored the same way (E and E2
    //     are bitwise symmetric -- outputs of this kernel family -- so the mirrored entry of every term IS the upper one, as
    //     the staged mirror already takes for the first output).
    // Same operations per element in the same order: same bits.  Blocks per batch as on the diagonal path: 16 VGPRs each.
    // (Not in the instantiations whose residency leaves one trip per batch, NB = 1 -- five workgroups per CU on 96 VGPRs: with
    // this path beside the staged one, which the bound partials keep, they need 108-110 and would lose a workgroup per CU.)
    constexpr bool REGEP = (SER == 0) && NB >= 2;
    const bool regs = REGEP && wide && !rowpart;
    if (regs) {
        constexpr int RB = DB;
        const int g = lane >> 4, odd = lane & 1, cc = lane & 14;
        // trip h of block (ti, tj): row I0 + wr + 16 ti + g + 8 odd + 4h -- a row of tile row I < J, inside the matrix whatever p
        // is -- and the column pair gj, gj + 1; the lane's offsets differ from those of its first trip by wave-uniform amounts
        const size_t o00 = (size_t)(I0 + wr + g + 8 * odd) * p + (size_t)(J0 + wc + cc);
        // the mirror of block (ti, tj): rows gj, gj + 1, two columns each from I0 + wr + 16 ti + 2 (g >> 1) + 4 (g & 1) + 8 odd
        // (rows of tile row I again)
        const size_t m00 = (size_t)(J0 + wc + cc) * p + (size_t)(I0 + wr + 2 * (g >> 1) + 4 * (g & 1) + 8 * odd);
        double2 re[RB * 2], rf[RB * 2];
        auto reg_loads = [&](const int b0) {          // one load instruction per operand and trip, see direct_loads below
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int ti = (b0 + q) / TJ, tj = (b0 + q) % TJ;
                const int gj = J0 + wc + 16 * tj + cc;
                const bool any = gj < p, half = any && gj + 1 >= p;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const size_t o = o00 + (size_t)(16 * ti + 4 * h) * p + 16 * tj - (half ? 1 : 0);
                    re[q * 2 + h] = double2{0.0, 0.0};
                    rf[q * 2 + h] = double2{0.0, 0.0};
                    if (any) {
                        if (Ek) re[q * 2 + h] = lde2(Ek + o);
                        if (E2k) rf[q * 2 + h] = lde2(E2k + o);
                    }
                }
            }
        };
        // block blk's accumulators, times cAcc, as the lane's two pairs: the even lane keeps registers 0, 1 and takes its
        // neighbour's, the odd lane keeps 2, 3
        auto exchange = [&](const int blk, double2* t) {
            const int ti = blk / TJ, tj = blk % TJ;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double lo = cAcc * acc[ti][tj][h], hi = cAcc * acc[ti][tj][2 + h];
                const double plo = lane_xor1(lo), phi = lane_xor1(hi);
                t[h].x = odd ? phi : lo;
                t[h].y = odd ? hi : plo;
            }
        };
        reg_loads(0);
#pragma unroll
        for (int b0 = 0; b0 < NBLK; b0 += RB) {
            if (b0 > 0) reg_loads(b0);
            // the first block's pair exchange runs under the loads
            double2 t0[2];
            exchange(b0, t0);
#pragma unroll
            for (int q = 0; q < RB * 2; ++q) { landed2(re[q]); landed2(rf[q]); }
#pragma unroll
            for (int q = 0; q < RB; ++q) {
                const int ti = (b0 + q) / TJ, tj = (b0 + q) % TJ;
                const int gj = J0 + wc + 16 * tj + cc;
                const bool any = gj < p, full = gj + 1 < p;
                double2 t[2], v[2], w[2];
                if (q == 0) { t[0] = t0[0]; t[1] = t0[1]; }
                else exchange(b0 + q, t);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const size_t o = o00 + (size_t)(16 * ti + 4 * h) * p + 16 * tj;
                    double2 e = re[q * 2 + h], f = rf[q * 2 + h];
                    if (any && !full) { e.x = e.y; f.x = f.y; }      // the odd last column, see direct_loads
                    // every lane does the arithmetic (what is not stored is not looked at); the guards are on the stores
                    v[h].x = __builtin_fma(cE, e.x, t[h].x);
                    v[h].y = __builtin_fma(cE, e.y, t[h].y);
                    if (E2k) { v[h].x = __builtin_fma(cE2, f.x, v[h].x); v[h].y = __builtin_fma(cE2, f.y, v[h].y); }
                    w[h] = double2{0.0, 0.0};
                    if (C2k) {
                        w[h].x = c2val(dC, v[h].x, dE, e.x);
                        w[h].y = c2val(dC, v[h].y, dE, e.y);
                        if (E2k) { w[h].x = __builtin_fma(dE2, f.x, w[h].x); w[h].y = __builtin_fma(dE2, f.y, w[h].y); }
                    }
                    dev = fmax(dev, fmax(any ? fabs(v[h].x) : 0.0, full ? fabs(v[h].y) : 0.0));
                    if (full) {
                        *reinterpret_cast<double2*>(Ck + o) = v[h];
                        if (C2k) *reinterpret_cast<double2*>(C2k + o) = w[h];
                    } else if (any) {
                        Ck[o] = v[h].x;
                        if (C2k) C2k[o] = w[h].x;
                    }
                }
                const size_t mo = m00 + (size_t)(16 * tj) * p + 16 * ti;
                swap_row16(v[0].x, v[1].x);
                swap_row16(v[0].y, v[1].y);
                if (any) *reinterpret_cast<double2*>(Ck + mo) = double2{v[0].x, v[1].x};
                if (full) *reinterpret_cast<double2*>(Ck + mo + p) = double2{v[0].y, v[1].y};
                if (C2k) {
                    swap_row16(w[0].x, w[1].x);
                    swap_row16(w[0].y, w[1].y);
                    if (any) *reinterpret_cast<double2*>(C2k + mo) = double2{w[0].x, w[1].x};
                    if (full) *reinterpret_cast<double2*>(C2k + mo + p) = double2{w[0].y, w[1].y};
                }
            }
        }
    } else if (wide) {
        double2 pe[NB], pf[NB];
        // trip u of the direct pass: lane -> row `row`, columns c2, c2 + 1 of the tile; the edge guards as ONE predicate per
        // trip.  (One load instruction per operand and trip, whatever the lane's case: a second one into the same registers
        // on another branch -- 8 bytes for the odd last column -- makes the compiler drain vmcnt(0) between the trips, a
        // write-after-write hazard it tracks per register, not per lane.)  Odd p: the last column is the first half of a
        // pair whose second half lies outside the matrix; its lane loads the pair ONE COLUMN TO THE LEFT (inside the row,
        // 4-byte aligned as the queues' unaligned-access mode allows) and takes the second half.
        auto direct_loads = [&](const int u0) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int e2 = tid + (u0 + q) * NT;
                const int row = e2 / (BM / 2), c2 = (e2 % (BM / 2)) * 2;
                const int gi = I0 + row, gj = J0 + c2;
                const bool any = gi < p && gj < p, half = any && gj + 1 >= p;
                const size_t o = (size_t)gi * p + gj - (half ? 1 : 0);
                pe[q] = double2{0.0, 0.0};
                pf[q] = double2{0.0, 0.0};
                if (any) {
                    if (Ek) pe[q] = lde2(Ek + o);
                    if (E2k) pf[q] = lde2(E2k + o);
                }
            }
        };
        direct_loads(0);
        lds_barrier();       // all fragment reads done before the slabs are reused as the mirror tile
#pragma unroll
        for (int ti = 0; ti < TI; ++ti)
#pragma unroll
            for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wr + ti * 16 + (lane >> 4) + 4 * r;
                    const int col = wc + tj * 16 + (lane & 15);
                    smem[row * BM + (col ^ row)] = cAcc * acc[ti][tj][r];
                }
        lds_barrier();
#pragma unroll
        for (int u0 = 0; u0 < NTRIP; u0 += NB) {
            if (u0 > 0) direct_loads(u0);
#pragma unroll
            for (int q = 0; q < NB; ++q) { landed2(pe[q]); landed2(pf[q]); }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int e2 = tid + (u0 + q) * NT;
                const int row = e2 / (BM / 2), c2 = (e2 % (BM / 2)) * 2;
                const int gi = I0 + row, gj = J0 + c2;
                // columns c2, c2 + 1 of row `row` sit at (c2 ^ row), (c2 ^ row) ^ 1: one aligned pair, swapped for odd rows
                double* tp = smem + row * BM + ((c2 ^ row) & ~1);
                double2 t = ld2(tp);
                if (row & 1) { const double h = t.x; t.x = t.y; t.y = h; }
                double2 e = pe[q], f = pf[q];
                if (gi < p && gj < p && gj + 1 >= p) { e.x = e.y; f.x = f.y; }      // the odd last column, see direct_loads
                // the final values go back to the tile: the bound partials and the mirror pass read them from there
                if (gi < p && gj + 1 < p) {
                    double2 v;
                    v.x = __builtin_fma(cE, e.x, t.x);
                    v.y = __builtin_fma(cE, e.y, t.y);
                    if (E2k) { v.x = __builtin_fma(cE2, f.x, v.x); v.y = __builtin_fma(cE2, f.y, v.y); }
                    dev = fmax(dev, fmax(fabs(v.x), fabs(v.y)));
                    *reinterpret_cast<double2*>(Ck + (size_t)gi * p + gj) = v;
                    if (C2k) {
                        double2 w;
                        w.x = c2val(dC, v.x, dE, e.x);
                        w.y = c2val(dC, v.y, dE, e.y);
                        if (E2k) { w.x = __builtin_fma(dE2, f.x, w.x); w.y = __builtin_fma(dE2, f.y, w.y); }
                        *reinterpret_cast<double2*>(C2k + (size_t)gi * p + gj) = w;
                    }
                    if (row & 1) { const double h = v.x; v.x = v.y; v.y = h; }
                    *reinterpret_cast<double2*>(tp) = v;
                } else if (gi < p && gj < p) {
                    double v0 = __builtin_fma(cE, e.x, t.x);
                    if (E2k) v0 = __builtin_fma(cE2, f.x, v0);
                    dev = fmax(dev, fabs(v0));
                    Ck[(size_t)gi * p + gj] = v0;
                    if (C2k) C2k[(size_t)gi * p + gj] = c2val2(dC, v0, dE, e.x, E2k != nullptr, dE2, f.x);
                    double2 v = {v0, 0.0};
                    if (row & 1) { v.x = 0.0; v.y = v0; }
                    *reinterpret_cast<double2*>(tp) = v;
                } else if (rowpart) {
                    *reinterpret_cast<double2*>(tp) = double2{0.0, 0.0};
                }
            }
        }
    } else {
        double de[DB * 4], df[DB * 4];
        // not a block of the tile (the diagonal tiles' rebalanced waves, see rbk / cbk above)
        auto no_block = [&](const int ti, const int tj) {
            return REBAL && ((ti != tj && tj == 0 && nval <= 3) || ((ti | tj) != 0 && nval <= 1));
        };
        auto diag_loads = [&](const int b0) {
#pragma unroll
            for (int q = 0; q < DB; ++q) {
                const int ti = (b0 + q) / TJ, tj = (b0 + q) % TJ;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    de[q * 4 + r] = 0.0;
                    df[q * 4 + r] = 0.0;
                }
                if (no_block(ti, tj)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = I0 + rbk[ti] + (lane >> 4) + 4 * r, gj = J0 + cbk[tj] + (lane & 15);
                    if (gi < p && gj < p && (I != J || gi <= gj)) {
                        if (Ek) de[q * 4 + r] = Ek[(size_t)gi * p + gj];
                        if (E2k) df[q * 4 + r] = E2k[(size_t)gi * p + gj];
                    }
                }
            }
        };
        diag_loads(0);
        lds_barrier();       // all fragment reads done before the slabs are reused as the mirror tile
        if (REBAL && I == J && rowpart && ABL != 1) {
            // the staged tile of the bound partials wants zeros below the diagonal: the six blocks no wave owns any more
            for (int e = tid; e < 6 * 256; e += NT) {
                const int blk = e >> 8, br = (blk < 1) ? 1 : (blk < 3 ? 2 : 3), bc = blk - (br == 1 ? 0 : (br == 2 ? 1 : 3));
                const int row = br * 16 + ((e >> 4) & 15), col = bc * 16 + (e & 15);
                smem[row * BM + (col ^ row)] = 0.0;
            }
        }
#pragma unroll
        for (int b0 = 0; b0 < NBLK; b0 += DB) {
            if (b0 > 0) diag_loads(b0);
#pragma unroll
            for (int q = 0; q < DB * 4; ++q) { landed(de[q]); landed(df[q]); }
#pragma unroll
            for (int q = 0; q < DB; ++q) {
                const int ti = (b0 + q) / TJ, tj = (b0 + q) % TJ;
                if (no_block(ti, tj)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = rbk[ti] + (lane >> 4) + 4 * r;
                    const int col = cbk[tj] + (lane & 15);
                    const int gi = I0 + row, gj = J0 + col;
                    double v = cAcc * acc[ti][tj][r];
                    const bool keep = gi < p && gj < p && (I != J || gi <= gj);
                    if (keep) {
                        if (gi == gj) v += cI;
                        const double e0 = de[q * 4 + r], f0 = df[q * 4 + r];
                        v = __builtin_fma(cE, e0, v);
                        if (E2k) v = __builtin_fma(cE2, f0, v);
                        dev = fmax(dev, fabs(v - (gi == gj ? 1.0 : 0.0)));
                        Ck[(size_t)gi * p + gj] = v;
                        if (C2k) C2k[(size_t)gi * p + gj] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0) + (gi == gj ? dI : 0.0);
                        if (I == J && gi != gj) {
                            Ck[(size_t)gj * p + gi] = v;
                            if (C2k) C2k[(size_t)gj * p + gi] = c2val2(dC, v, dE, e0, E2k != nullptr, dE2, f0);
                        }
                    }
                    // XOR-swizzled BM x BM tile in LDS: with bound partials every tile is staged (entries that are not stored
                    // count as zero); an off-diagonal tile comes here only without its mirror (ABL 1)
                    if ((I != J || rowpart) && ABL != 1) smem[row * BM + (col ^ row)] = (rowpart && !keep) ? 0.0 : v;
                }
            }
        }
    }
    if (maxdev) {
        dev = wave_max(dev);
        if (lane == 0 && dev > 0.0)
            atomicMax(reinterpret_cast<unsigned long long*>(maxdev + k), (unsigned long long)__double_as_longlong(dev));
    }
    if ((I != J || rowpart) && ABL != 1 && !regs) lds_barrier();      // the staged tile holds the final values
    if (rowpart && ABL != 1 && tid < 2 * BM) symm_dl_partials<BM>(smem, rowpart, fropart, k, p, T, blockTile, I, J, I0, J0, tid);
    if (wide && !regs) {
        // the mirror: row a of it is column a of the staged tile, two consecutive columns c2, c2 + 1 per lane -- final values,
        // no arithmetic left but the second output's, whose E / E2 terms are loaded at the mirrored addresses
        // (loaded under the serial epilogue's condition -- without bound partials also where dE or dE2 is zero: fma(0, e, x)
        // is x only up to the sign of a zero and for finite e, and the second output keeps its bits exactly)
        const bool need_e = Ek && C2k && (!rowpart || dE != 0.0), need_f = E2k && C2k && (!rowpart || dE2 != 0.0);
        double2 me[NB], mf[NB];
#pragma unroll
        for (int u0 = 0; u0 < NTRIP; u0 += NB) {
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int e2 = tid + (u0 + q) * NT;
                const int a = e2 / (BM / 2), c2 = (e2 % (BM / 2)) * 2;
                const size_t o = (size_t)(J0 + a) * p + I0 + c2;
                const bool any = J0 + a < p && I0 + c2 < p, half = any && I0 + c2 + 1 >= p;
                me[q] = double2{0.0, 0.0};
                mf[q] = double2{0.0, 0.0};
                if (any) {                       // (one load per operand and trip, as in direct_loads)
                    if (need_e) me[q] = lde2(Ek + o - (half ? 1 : 0));
                    if (need_f) mf[q] = lde2(E2k + o - (half ? 1 : 0));
                }
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) { landed2(me[q]); landed2(mf[q]); }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int e2 = tid + (u0 + q) * NT;
                const int a = e2 / (BM / 2), c2 = (e2 % (BM / 2)) * 2;      // out[J0+a][I0+c2 .. +1] = tile[c2 .. +1][a]
                const size_t o = (size_t)(J0 + a) * p + I0 + c2;
                double2 e = me[q], f = mf[q];
                if (J0 + a < p && I0 + c2 < p && I0 + c2 + 1 >= p) { e.x = e.y; f.x = f.y; }
                if (J0 + a < p && I0 + c2 + 1 < p) {
                    double2 v;
                    v.x = smem[c2 * BM + (a ^ c2)];
                    v.y = smem[(c2 + 1) * BM + (a ^ (c2 + 1))];
                    *reinterpret_cast<double2*>(Ck + o) = v;
                    if (C2k) {
                        double2 w;
                        w.x = c2val(dC, v.x, dE, e.x);
                        w.y = c2val(dC, v.y, dE, e.y);
                        if (E2k) { w.x = __builtin_fma(dE2, f.x, w.x); w.y = __builtin_fma(dE2, f.y, w.y); }
                        *reinterpret_cast<double2*>(C2k + o) = w;
                    }
                } else if (J0 + a < p && I0 + c2 < p) {
                    // (never taken: I < J, so the rows I0 .. I0 + BM - 1 of an off-diagonal tile all lie inside the matrix and an
                    // odd last column can only belong to tile column J; kept so that the pair test above stands on its own)
                    const double v0 = smem[c2 * BM + (a ^ c2)];
                    Ck[o] = v0;
                    if (C2k) C2k[o] = c2val2(dC, v0, dE, e.x, E2k != nullptr, dE2, f.x);
                }
            }
        }
    }
}

// The bound validation of a speculative Omega-step as extra workgroups of a product launch (CwRider, kernels.hpp): workgroup
// idx of the rider takes rows 16 bx .. 16 bx + 15 of instance k.  Arithmetic and order are those of k_bound_rows (row sums in
// tile-column order, their maximum) and k_cw_final (lane-strided products, wave sums, memory-side atomic max and arrival, the
// Frobenius shares added in tile order by the last workgroup of the instance) -- the bound and the vector left for the next
// iteration are the same bits.  Every workgroup adds the row sums of its instance itself (T p loads out of L2; the only thing
// it needs of them is their maximum, the scale of the next vector): hidden work on CUs the product leaves idle.
__device__ __forceinline__ void cw_rider_body(const CwRider& r, int idx, double* sh)
{
    const int k = idx / r.nbx, bx = idx - k * r.nbx;
    if (k >= r.K) return;
    const int p = r.p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mxd = 0.0;
    for (int j = threadIdx.x; j < p; j += 256) {
        const double* rp = r.rowpart + (size_t)k * r.T * p + j;
        double v = 0.0;
        for (int s2 = 0; s2 < r.T; ++s2) v += rp[(size_t)s2 * p];
        mxd = fmax(mxd, v);
        if (bx == 0 && r.d_out) r.d_out[(size_t)k * p + j] = v;
    }
    mxd = wave_max(mxd);
    if (lane == 0) sh[wave] = mxd;
    __syncthreads();
    const double inf0 = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    __syncthreads();
    const double scale = 1.0 / inf0;
    const double* dk = r.dprev + (size_t)k * p;
    const int r0 = bx * 16 + wave * 4;
    const double* w = r.B + (size_t)k * p * p;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    size_t ro[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ok[q] = (r0 + q) < p;
        ro[q] = (size_t)min(r0 + q, p - 1) * p;
    }
    for (int j = lane; j < p; j += 64) {
        const double dj = dk[j];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += fabs(w[ro[q] + j]) * dj;
    }
    double mx = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double y = wave_sum(a[q]);
        if (ok[q]) {
            mx = fmax(mx, y / dk[r0 + q]);
            if (r.dnext && lane == 0) {
                const double v = y * scale;
                r.dnext[(size_t)k * p + r0 + q] = (v > 0.0 && isfinite(v)) ? v : 1.0;
            }
        }
    }
    if (lane == 0) sh[wave] = mx;
    __syncthreads();
    int* last = reinterpret_cast<int*>(sh + 4);
    if (threadIdx.x == 0) {
        mx = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
        const unsigned long long old = __hip_atomic_fetch_max(r.cwmax + k, (unsigned long long)__double_as_longlong(mx),
                                                              __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned arrive = 1u + (unsigned)(old >> 63);
        *last = __hip_atomic_fetch_add(r.cnt + k, arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)r.nbx - 1;
    }
    __syncthreads();
    if (!*last) return;
    double cw = 0.0;
    if (threadIdx.x == 0) {
        cw = __longlong_as_double((long long)__hip_atomic_exchange(r.cwmax + k, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        __hip_atomic_store(r.cnt + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    double sq = 0.0;
    double* shfro = sh + 8;
    for (int t0 = 0; t0 < r.ntile; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        __syncthreads();
        shfro[threadIdx.x] = (t < r.ntile) ? r.fropart[(size_t)k * r.ntile + t] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(256, r.ntile - t0);
            for (int q = 0; q < m; ++q) sq += shfro[q];
        }
    }
    if (threadIdx.x != 0) return;
    double inf = inf0;
    const double fr = sqrt(sq);
    if (isfinite(cw) && cw > 0.0) { const double wv = cw * (1.0 + 1e-12); inf = (wv < inf) ? wv : inf; }
    const double b = sqrt((fr < inf) ? fr : inf);
    r.out[k] = b;
    if (r.flag && !(b <= r.cuse[k])) {
        atomicOr(r.flag + r.flag_slot, 1);
        r.flag_host[r.flag_slot] = 1;
    }
}

// the norm reduction as a rider (RedRider): k_reduce_partials' single row -- four rows per trip, strided per-thread sums in
// ascending order, wave sums, the four waves added in a fixed order -- then the sums and, behind them, the sequence number as
// system-scope stores.  No release FENCE here: inside a product launch it would write back an XCD's L2 (the tiles' output).
// What orders the two instead: the sums are system-scope (write-through, uncached) stores of ONE wave, `s_waitcnt vmcnt(0)`
// returns when they have been acknowledged, the barrier puts thread 0's store of the sequence number behind that -- and the
// row carries the sequence number a second time, in the same store instruction as the sums (slot nv), which the host checks
// after the poll (finish_norms): a sequence number that overtook its sums would be seen without its stamp.
__device__ __forceinline__ void red_rider_body(const RedRider& r, double* smem)
{
    double (*sh)[8] = reinterpret_cast<double (*)[8]>(smem);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nblk = r.nblk, nv = r.nv;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double* base = r.partials;
    // (two rows per trip where k_reduce_partials takes four -- the same rows per thread in the same ascending order, hence the
    // same sums -- so that this branch stays inside the product kernel's 81 registers: with four the 32x32 kernel went to 108
    // and from five to four workgroups per CU)
    for (int b = threadIdx.x; b < nblk; b += 512) {
        double t[2][8];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int bb = b + 256 * u;
#pragma unroll
            for (int v = 0; v < 8; ++v) t[u][v] = (v < nv && bb < nblk) ? base[(size_t)bb * nv + v] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (b + 256 * u < nblk) {
#pragma unroll
                for (int v = 0; v < 8; ++v)
                    if (v < nv) acc[v] += t[u][v];
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        if (v < nv) {
            const double s = wave_sum(acc[v]);
            if (lane == 0) sh[wid][v] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= nv) {
        const double s = (int)threadIdx.x == nv ? (double)r.seq_val
                                                : (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
        __hip_atomic_store(r.out + threadIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(r.seq, r.seq_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// a rider nobody took (symm_flush_rider)
__global__ __launch_bounds__(256) void k_cw_rider(const CwRider rider)
{
    __shared__ __attribute__((aligned(16))) double sh[8 + 256];
    cw_rider_body(rider, (int)blockIdx.x, sh);
}

// SER 1: the serial epilogue, SER 2: the staged batched one (development library only, see symm_dl_tile)
template <int BK, int NSTG, int ABL = 0, int BM = 64, int NW = 4, int SER = 0>
__global__ __launch_bounds__(NW * 64) void k_symm_dl(const double* __restrict__ A, const double* __restrict__ B,
                                                 double* __restrict__ C, double* __restrict__ C2,
                                                 const double* __restrict__ E, const double* __restrict__ E2,
                                                 const double* __restrict__ coef, int K,
                                                 int p, const double* __restrict__ A1, const double* __restrict__ B1,
                                                 double* __restrict__ C1, int K1, double* __restrict__ maxdev,
                                                 double* __restrict__ rowpart, double* __restrict__ fropart, const CwRider rider,
                                                 const CopySegs cps, const RedRider red)
{
    __shared__ __attribute__((aligned(16))) double smem[NSTG * 2 * BK * BM];
    const int T = (p + BM - 1) / BM;
    int bid = (int)blockIdx.x;
    if constexpr (NW == 4) {
        // The norm reduction the host is waiting for rides in FRONT of the product's workgroups (dispatched first: behind them
        // its result reached the host ~10 us after the Theta kernel had ended, in front ~5); NXCD slots, one of them working,
        // so that the tiles keep their XCDs.
        if (red.nblk > 0) {
            if (bid < NXCD) {
                if (bid == 0) red_rider_body(red, smem);
                return;
            }
            bid -= NXCD;
        }
        // workgroups behind the product's own: the bound validation of the previous launch's output (CwRider), table transfers
        const int base = xcd_grid(T * (T + 1) / 2, K + K1);
        if (bid >= base) {
            const int idx = bid - base, ncw = rider.K * rider.nbx;
            if (idx < ncw) cw_rider_body(rider, idx, smem);
            else {
                // (k_copy_small: words from the pinned tables, or zeros; 1024 words per workgroup, so that no thread waits for
                // more than four reads over PCIe one after the other -- one workgroup per segment took 45 us for the 30 KB of a
                // K = 64 schedule)
                int blk = idx - ncw;
                for (int sgi = 0; sgi < cps.n; ++sgi) {
                    const int nb = (int)((cps.words[sgi] + 1023u) / 1024u);
                    if (blk < nb) {
                        unsigned* d = (unsigned*)cps.dst[sgi];
                        const unsigned* src = (const unsigned*)cps.src[sgi];
                        const unsigned i0 = (unsigned)blk * 1024u + threadIdx.x;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned i = i0 + 256u * e;
                            if (i < cps.words[sgi]) d[i] = src ? src[i] : 0u;
                        }
                        break;
                    }
                    blk -= nb;
                }
            }
            return;
        }
    }
    int k, b;
    if (!decode_block_xcd(T * (T + 1) / 2, K + K1, k, b, bid)) return;
    symm_dl_tile<BK, NSTG, ABL, BM, NW, SER>(A, B, C, C2, E, E2, coef, K, p, A1, B1, C1, K1, maxdev, rowpart, fropart, k, b, smem);
}

#ifdef GGL_DEV
// which epilogue the direct-to-LDS launches of the development library run (ggl_dev_set_symm_epilogue): 0 the product's --
// batched, off-diagonal tiles written from registers --, 1 the serial one, 2 the batched one with the staged LDS tile (the
// product's before the register path); the product library compiles 0 only
static int g_symm_epilogue = 0;
int symm_set_epilogue(int mode)
{
    const int was = g_symm_epilogue;
    g_symm_epilogue = (mode == 1 || mode == 2) ? mode : 0;
    return was;
}
#endif

static thread_local CwRider g_rider;          // pending (K > 0): see symm_set_rider
static thread_local CopySegs g_copy_rider;    // pending (n > 0): see symm_set_copy_rider
static thread_local RedRider g_red_rider;     // pending (nblk > 0): see symm_set_reduce_rider
void symm_set_reduce_rider(const RedRider& r) { g_red_rider = r; }
void symm_set_rider(const CwRider& r) { g_rider = r; }
void symm_set_copy_rider(const CopySegs& sg) { g_copy_rider = sg; }
void symm_flush_rider(hipStream_t st)
{
    if (g_red_rider.nblk > 0) {
        launch_reduce_partials(st, g_red_rider.partials, 1, g_red_rider.nblk, g_red_rider.nv, g_red_rider.out, g_red_rider.seq,
                               g_red_rider.seq_val);
        g_red_rider = RedRider{};
    }
    if (g_copy_rider.n > 0) {
        launch_copy_small(st, g_copy_rider);
        g_copy_rider = CopySegs{};
    }
    if (g_rider.K <= 0) return;
    hipLaunchKernelGGL(k_cw_rider, dim3(g_rider.K * g_rider.nbx), dim3(256), 0, st, g_rider);
    g_rider = CwRider{};
}

// ---------------------------------------------------------------------------------------------
// General (non-symmetric result) product with a symmetric right factor:
//     C[b] = s[b] * A[b] * T[b % K],     b = 0 .. nbatch-1,
// used by the numerically stable Newton-Schulz path where Y and P = Z^T are both multiplied by
// the same T from the right (newton_schulz.hip); nbatch = 2K covers both in one launch.  A is
// read as row panels A[I0+i][m0+k] (k contiguous), T as row panels T[m0+k][J0+j] (T symmetric, so
// its rows are its columns); full output, no mirroring.
// ---------------------------------------------------------------------------------------------
template <int BM, int BK, int WM, int WN>
__global__ __launch_bounds__(sym_nt(BM, WM, WN)) void k_gemm_nt_right(const double* __restrict__ A,
                                                                      const double* __restrict__ T,
                                                                      double* __restrict__ C,
                                                                      const double* __restrict__ scal, int nbatch, int K, int p)
{
    constexpr int NWC = BM / WN, NT = sym_nt(BM, WM, WN), TI = WM / 16, TJ = WN / 16;
    constexpr int LDA = BK + 2;      // A tile [BM][BK]: (2 i + k) mod 32 distinct over a half wave
    constexpr int LDB = BM + 16;     // T tile [BK][BM]
    __shared__ __attribute__((aligned(16))) double smem[BM * LDA + BK * LDB];
    double* As = smem;
    double* Bs = smem + BM * LDA;
    const int Tn = (p + BM - 1) / BM;
    int b, tile;
    if (!decode_block_xcd(Tn * Tn, nbatch, b, tile)) return;
    const int kt = b % K;
    const int I0 = (tile / Tn) * BM, J0 = (tile % Tn) * BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = (wave / NWC) * WM, wc = (wave % NWC) * WN;
    const size_t pp = (size_t)p * p;
    const double* Ab = A + (size_t)b * pp;
    const double* Tb = T + (size_t)kt * pp;

    v4d acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

    constexpr int LPT = (BM * BK) / NT;
    static_assert((BM * BK) % NT == 0 && NT % BK == 0 && NT % BM == 0, "tile/thread mismatch");
    const int acol = tid % BK, arow = tid / BK;      // A tile element (arow + q*NT/BK, acol)
    const int bcol = tid % BM, brow = tid / BM;      // T tile element (brow + q*NT/BM, bcol)
    double ra[LPT], rb[LPT];
    auto fetch = [&](int m0) {
#pragma unroll
        for (int q = 0; q < LPT; ++q) {
            const int i = min(I0 + arow + q * (NT / BK), p - 1), m = min(m0 + acol, p - 1);
            ra[q] = Ab[(size_t)i * p + m];
            const int mb = min(m0 + brow + q * (NT / BM), p - 1), j = min(J0 + bcol, p - 1);
            rb[q] = Tb[(size_t)mb * p + j];
        }
    };
    auto stage = [&](int m0) {
#pragma unroll
        for (int q = 0; q < LPT; ++q) {
            const bool ina = (I0 + arow + q * (NT / BK)) < p && (m0 + acol) < p;
            const bool inb = (m0 + brow + q * (NT / BM)) < p && (J0 + bcol) < p;
            As[(arow + q * (NT / BK)) * LDA + acol] = ina ? ra[q] : 0.0;
            Bs[(brow + q * (NT / BM)) * LDB + bcol] = inb ? rb[q] : 0.0;
        }
    };
    fetch(0);
    for (int m0 = 0; m0 < p; m0 += BK) {
        stage(m0);
        __syncthreads();
        fetch(m0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const int kq = kk * 4 + (lane >> 4);
            double af[TI], bf[TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i) af[i] = As[(wr + i * 16 + (lane & 15)) * LDA + kq];
#pragma unroll
            for (int j = 0; j < TJ; ++j) bf[j] = Bs[kq * LDB + wc + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    const double sc = scal[b];
    double* Cb = C + (size_t)b * pp;
#pragma unroll
    for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = I0 + wr + ti * 16 + (lane >> 4) + 4 * r;
                const int gj = J0 + wc + tj * 16 + (lane & 15);
                if (gi < p && gj < p) Cb[(size_t)gi * p + gj] = sc * acc[ti][tj][r];
            }
}

void launch_gemm_right(hipStream_t st, const double* A, const double* T, double* C, const double* scal, int nbatch,
                       int K, int p, int variant)
{
    if (variant == 1) {
        const int Tn = (p + 127) / 128;
        hipLaunchKernelGGL((k_gemm_nt_right<128, 16, 32, 64>), dim3(xcd_grid(Tn * Tn, nbatch)), dim3(512), 0, st, A, T, C, scal, nbatch, K, p);
    } else {
        const int Tn = (p + 63) / 64;
        hipLaunchKernelGGL((k_gemm_nt_right<64, 32, 32, 32>), dim3(xcd_grid(Tn * Tn, nbatch)), dim3(256), 0, st, A, T, C, scal, nbatch, K, p);
    }
}

static constexpr int SMALL_DL_MIN_P = 16;         // (round 4: measured ahead of the register-staged 32x32 kernel at every even p from 16 up, tools/bench_symm_small.py)
static constexpr long SMALL_BATCH_TILES = 800;   // up to here the 32x32-tile kernel, above the 64x64 direct-to-LDS one

// ---------------------------------------------------------------------------------------------
// Product-kernel variants: ONE table.  What a variant number means -- kernel family, tile edge, template instance, ablation
// or not, in the product library or in the development library (GGL_DEV, libggl_hip_dev.so) only -- is written here and
// nowhere else: symm_variant_built, symm_effective_variant, symm_bounds_tile and the launches all read this table.
//   TN  k_symm_tn, register-staged: <BM, BK, WM, WN, LM, ABL>         DL  k_symm_dl, direct-to-LDS: <BK, NSTG, ABL, BM, NW>
// The tile edge of a row is its BM.  ABL != 0: a timing ablation (wrong results on purpose; tools/bench_tail.py and others).
// A DL row at a dimension the DMA kernel does not take (symm_dl_serves) runs the product's TN row of the same tile edge.
// (40 and 41 are not product-kernel variants: ggl_ns_stats reports 41 for the LDS Omega kernel, capi_omega.hip.)
// ---------------------------------------------------------------------------------------------
enum class Fam { TN, DL };
struct Variant {
    Fam fam;
    bool product;               // the product library carries it (the solvers dispatch to it)
    int bm, bk, abl;
    int wm, wn;                 // TN: wave tile
    bool lm;                    // TN: off-diagonal tiles mirrored through LDS
    int nstg, nw;               // DL: slabs resident in LDS, waves per workgroup
    const char* what;
};
constexpr bool PRODUCT = true, DEV = false;
constexpr Variant tn(bool product, int bm, int bk, int wm, int wn, bool lm, int abl, const char* what)
{
    return Variant{Fam::TN, product, bm, bk, abl, wm, wn, lm, 0, 0, what};
}
constexpr Variant dl(bool product, int bk, int nstg, int abl, int bm, int nw, const char* what)
{
    return Variant{Fam::DL, product, bm, bk, abl, 0, 0, false, nstg, nw, what};
}
constexpr Variant VARIANTS[] = {
    /*  0 */ tn(PRODUCT, 64, 16, 32, 32, true, 0, "64x64, k-slab 16: large batches at a p the DMA kernel does not take"),
    /*  1 */ tn(DEV, 64, 32, 32, 32, true, 0, "64x64, k-slab 32"),
    /*  2 */ tn(DEV, 128, 16, 64, 64, false, 0, "128x128, 64x64 wave tiles, direct mirror stores"),
    /*  3 */ tn(DEV, 128, 16, 32, 64, false, 0, "128x128, 32x64 wave tiles, direct mirror stores"),
    /*  4 */ tn(DEV, 64, 16, 32, 32, false, 0, "64x64, direct mirror stores"),
    /*  5 */ tn(DEV, 128, 32, 64, 64, false, 0, "128x128, k-slab 32, direct mirror stores"),
    /*  6 */ tn(DEV, 64, 16, 32, 32, true, 1, "ablation of 0: no global loads"),
    /*  7 */ tn(DEV, 64, 16, 32, 32, true, 2, "ablation of 0: no MFMA"),
    /*  8 */ tn(DEV, 32, 16, 16, 16, true, 0, "32x32, k-slab 16"),
    /*  9 */ tn(PRODUCT, 32, 32, 16, 16, true, 0, "32x32, k-slab 32: small batches at a p the DMA kernel does not take"),
    /* 10 */ tn(DEV, 64, 16, 32, 32, true, 3, "timeline probe of 0 (maxdev is a [grid][5] long long buffer)"),
    /* 11 */ tn(DEV, 64, 16, 16, 32, true, 0, "64x64, 16x32 wave tiles"),
    /* 12 */ tn(DEV, 64, 32, 16, 32, true, 0, "64x64, k-slab 32, 16x32 wave tiles"),
    /* 13 */ tn(DEV, 64, 16, 32, 16, true, 0, "64x64, 32x16 wave tiles"),
    /* 14 */ tn(DEV, 64, 16, 32, 32, true, 4, "ablation of 0: ds_read + MFMA only"),
    /* 15 */ tn(DEV, 64, 16, 32, 32, true, 5, "ablation of 0: ds_read + MFMA + ds_write"),
    /* 16 */ dl(PRODUCT, 16, 2, 0, 64, 4, "64x64, double-buffered DMA: large batches"),
    /* 17 */ dl(PRODUCT, 16, 3, 0, 64, 4, "64x64, three DMA stages: concurrent parts"),
    /* 18 */ dl(DEV, 16, 4, 0, 64, 4, "64x64, four DMA stages"),
    /* 19 */ dl(DEV, 32, 2, 0, 64, 4, "64x64, k-slab 32"),
    // 32x32 tiles, k-slab 32, double buffer: 32 KiB of LDS, five workgroups per CU.  Measured (MI355X, p = 500, us per launch
    // at K = 2 / 4 / 8 / 16): 15.9 / 21.8 / 35.0 / 58.6, against 16.3 / 26.4 / 40.2 / 70.3 with four slabs in flight (27: 64 KiB,
    // two workgroups per CU: residency, not prefetch depth, is what the small batches lack)
    /* 20 */ dl(PRODUCT, 32, 2, 0, 32, 4, "32x32, k-slab 32, double-buffered DMA: small batches"),
    /* 21 */ dl(DEV, 16, 2, 1, 64, 4, "ablation of 16: no mirror write (and no bound partials)"),
    // eight waves per workgroup (two per SIMD) for batches that leave one workgroup per CU.  Measured (MI355X, p = 500):
    // K = 4: 27.0 / 26.3 us vs 26.6 us for the 32x32 kernel; K = 8: 43.9 / 49.3 vs 40.4; K = 16: 68.6 / 74.9 vs 63.9 -- no gain
    // anywhere, so the product library does not carry them
    /* 22 */ dl(DEV, 16, 4, 0, 64, 8, "64x64, eight waves, four DMA stages"),
    /* 23 */ dl(DEV, 32, 3, 0, 64, 8, "64x64, eight waves, k-slab 32, three DMA stages"),
    // other slab / prefetch depths of the 32x32 kernel (LDS per workgroup: 32 / 48 / 48 / 64 / 16 / 24 KiB)
    /* 24 */ dl(DEV, 16, 4, 0, 32, 4, "32x32, k-slab 16, four DMA stages"),
    /* 25 */ dl(DEV, 32, 3, 0, 32, 4, "32x32, k-slab 32, three DMA stages"),
    /* 26 */ dl(DEV, 16, 6, 0, 32, 4, "32x32, k-slab 16, six DMA stages"),
    /* 27 */ dl(DEV, 32, 4, 0, 32, 4, "32x32, k-slab 32, four DMA stages"),
    /* 28 */ dl(DEV, 16, 2, 0, 32, 4, "32x32, k-slab 16, double-buffered DMA"),
    /* 29 */ dl(DEV, 16, 3, 0, 32, 4, "32x32, k-slab 16, three DMA stages"),
    /* 30 */ dl(DEV, 16, 3, 2, 64, 4, "ablation of 17: no operand loads"),
    /* 31 */ dl(DEV, 16, 3, 3, 64, 4, "ablation of 17: no MFMA"),
    /* 32 */ dl(DEV, 16, 3, 4, 64, 4, "ablation of 17: no epilogue"),
    /* 33 */ dl(DEV, 16, 3, 5, 64, 4, "ablation of 17: no slab barrier"),
    /* 34 */ dl(DEV, 32, 2, 2, 32, 4, "ablation of 20: no operand loads"),
    /* 35 */ dl(DEV, 32, 2, 3, 32, 4, "ablation of 20: no MFMA"),
    /* 36 */ dl(DEV, 32, 2, 4, 32, 4, "ablation of 20: no epilogue"),
    /* 37 */ dl(DEV, 32, 2, 5, 32, 4, "ablation of 20: no slab barrier"),
    // shallower slabs, more of them in flight: 32 KiB (4 x 8 KiB) / 48 KiB (6 x 8 KiB) of LDS
    /* 38 */ dl(DEV, 8, 4, 0, 64, 4, "64x64, k-slab 8, four DMA stages"),
    /* 39 */ dl(DEV, 8, 6, 0, 64, 4, "64x64, k-slab 8, six DMA stages"),
};
constexpr int NVARIANT = (int)(sizeof(VARIANTS) / sizeof(VARIANTS[0]));

constexpr bool variant_in_build(int v)
{
#ifdef GGL_DEV
    return v >= 0 && v < NVARIANT;
#else
    return v >= 0 && v < NVARIANT && VARIANTS[v].product;
#endif
}
// the product library's register-staged kernel of a tile edge: where a DL row goes at a dimension the DMA kernel does not take
constexpr int tn_fallback(int bm)
{
    for (int v = 0; v < NVARIANT; ++v)
        if (VARIANTS[v].fam == Fam::TN && VARIANTS[v].product && VARIANTS[v].bm == bm) return v;
    return -1;
}
constexpr int DEFAULT_VARIANT = tn_fallback(64);      // what a number outside the table or the build runs
constexpr bool variant_table_ok()
{
    int nproduct = 0;
    for (int v = 0; v < NVARIANT; ++v) {
        const Variant& r = VARIANTS[v];
        nproduct += r.product;
        if (r.product && r.abl != 0) return false;                                     // no ablation in the product library
        if (r.fam == Fam::DL && (tn_fallback(r.bm) < 0 || (r.nw != 4 && r.nw != 8))) return false;
        if (r.fam == Fam::TN && r.abl != 0 && tn_fallback(r.bm) < 0) return false;      // (pair launches, launch_variant)
    }
    return nproduct == 5;
}
static_assert(NVARIANT == 40, "variant numbers 0 .. 39");
static_assert(variant_table_ok(), "variant table");
static_assert(VARIANTS[0].product && VARIANTS[9].product && VARIANTS[16].product && VARIANTS[17].product && VARIANTS[20].product,
              "the product library carries exactly 0, 9, 16, 17 and 20");
static_assert(tn_fallback(64) == 0 && tn_fallback(32) == 9, "what ggl_ns_stats reports for the register-staged kernels");

int symm_variants() { return NVARIANT - 1; }
bool symm_variant_built(int v) { return variant_in_build(v); }

// Measured on MI355X (tools/bench_small_batches.py, profiles/r2_small_batches_product_kernel.txt), us per launch,
// 32x32 (20) against 64x64 (16) direct-to-LDS tiles: p = 500: K = 2: 16.1 / 28.3, K = 4: 21.6 / 29.7, K = 8: 34.7 / 44.7,
// K = 16 (576 64x64 tile pairs): 59.5 / 63.5; p = 1000: K = 4 (544): 111.5 / 116.4, K = 8 (1088): 220.5 / 199.8;
// p = 200, K = 20: 11.8 / 16.4 (register-staged 32x32: 14.7).  Four times the workgroups and five of them resident per CU
// fill the chip where the 64x64 tiles leave it waiting; from ~1000 tile pairs on the 64x64 tiles' halved L2 -> LDS
// traffic wins.  Odd p: the register-staged kernels 9 / 0.
// Odd p on the direct-to-LDS kernel (round 6).  Its DMA moves 16 bytes per lane, and for odd p every other row of a stack starts
// on an 8-byte boundary only: rounds 1-5 sent every odd p to the register-staged kernel, 25-37 % slower per product.  The
// hardware takes dword-aligned addresses for global_load_lds_dwordx4 and for 16-byte global loads / stores (the queues run in
// unaligned-access mode), so what odd p needs is (i) the last column as the first half of a pair whose second half lies
// outside the matrix (symm_dl_tile: clamp, epilogue) and (ii) 8 bytes of slack behind every stack that can be an operand.
// g_odd_dl = false restores the old dispatch (GGL_OPT_ODD_DL, for A/B runs and tests).
static bool g_odd_dl = true;
void symm_set_odd_dl(bool on) { g_odd_dl = on; }
bool symm_dl_serves(int p) { return p >= 2 && ((p & 1) == 0 || g_odd_dl); }

// the kernel a variant really runs for this p: a direct-to-LDS variant that the dimension does not allow falls to the
// register-staged kernel of the same tile (what ggl_ns_stats reports: the dispatch tests assert the kernel, not the request)
int symm_effective_variant(int variant, int p)
{
    if (variant >= 0 && variant < NVARIANT && VARIANTS[variant].fam == Fam::DL && !symm_dl_serves(p))
        return tn_fallback(VARIANTS[variant].bm);
    return variant;
}

int symm_auto_variant(int nprod, int p)
{
    const long T64 = (p + 63) / 64;
    return (T64 * (T64 + 1) / 2 * nprod <= SMALL_BATCH_TILES) ? (p >= SMALL_DL_MIN_P ? 20 : 9) : 16;
}

// tile edge of the direct-to-LDS kernel a variant resolves to, or 0 if the variant (or an odd p) runs the register-staged
// kernel, which does not produce bound partials (nor does the DL ablation without the mirror write, ABL 1: no staged tile)
int symm_bounds_tile(int K, int p, int variant)
{
    if (variant < 0) variant = symm_auto_variant(K, p);
    if (variant >= NVARIANT || !symm_dl_serves(p)) return 0;
    const Variant& r = VARIANTS[variant];
    return (r.fam == Fam::DL && r.abl != 1) ? r.bm : 0;
}

// everything a product launch takes; a pair launch (two independent products in one launch: C = coef[k]-affine(A*B) for k < K
// and C1 = coef[K + k]-scaled(A1*B1)) fills the second operand set, K1 = K
struct SymmArgs {
    hipStream_t st;
    const double *A, *B;
    double *C, *C2;
    const double *E, *E2, *coef;
    int K, p;
    const double *A1, *B1;
    double* C1;
    int K1;
    double *maxdev, *rowpart, *fropart;
};

template <int BM, int BK, int WM, int WN, bool LM, int ABL> static void launch_tn(const SymmArgs& a)
{
    using Cfg = SymCfg<BM, BK, WM, WN, LM>;
    const int T = (a.p + BM - 1) / BM;
    double* md = (ABL == 0 || ABL == 3) ? a.maxdev : nullptr;      // (ABL 3: the timeline buffer)
    hipLaunchKernelGGL((k_symm_tn<BM, BK, WM, WN, LM, ABL>), dim3(xcd_grid(T * (T + 1) / 2, a.K + a.K1)), dim3(Cfg::NT), 0, a.st,
                       a.A, a.B, a.C, a.C2, a.E, a.coef, a.K, a.p, a.A1, a.B1, a.C1, a.K1, md, a.E2);
}

template <int BK, int NSTG, int ABL, int BM, int NW> static void launch_dl(const SymmArgs& a)
{
    // (the eight-wave development variants do not carry riders: the rider stays pending)
    constexpr bool rides = NW == 4;
    const CwRider rider = (g_rider.K > 0 && rides) ? g_rider : CwRider{};
    if (rider.K > 0) g_rider = CwRider{};
    const CopySegs cps = (g_copy_rider.n > 0 && rides) ? g_copy_rider : CopySegs{};
    if (cps.n > 0) g_copy_rider = CopySegs{};
    const RedRider red = (g_red_rider.nblk > 0 && rides) ? g_red_rider : RedRider{};
    if (red.nblk > 0) g_red_rider = RedRider{};
    int ncopy = red.nblk > 0 ? NXCD : 0;          // (in front of the tiles, see k_symm_dl)
    for (int i = 0; i < cps.n; ++i) ncopy += (int)((cps.words[i] + 1023u) / 1024u);
    const int nride = rider.K * rider.nbx + ncopy;
    const int T = (a.p + BM - 1) / BM;
    const dim3 grid(xcd_grid(T * (T + 1) / 2, a.K + a.K1) + nride), block(NW * 64);
#define GGL_DL_LAUNCH(SER)                                                                                                      \
    hipLaunchKernelGGL((k_symm_dl<BK, NSTG, ABL, BM, NW, SER>), grid, block, 0, a.st, a.A, a.B, a.C, a.C2, a.E, a.E2, a.coef, a.K, \
                       a.p, a.A1, a.B1, a.C1, a.K1, a.maxdev, a.rowpart, a.fropart, rider, cps, red)
#ifdef GGL_DEV
    if (g_symm_epilogue == 1) GGL_DL_LAUNCH(1);       // the epilogue ggl_dev_set_symm_epilogue names
    else if (g_symm_epilogue == 2) GGL_DL_LAUNCH(2);
    else
#endif
        GGL_DL_LAUNCH(0);
#undef GGL_DL_LAUNCH
}

// row V of the table: the one place a template instance is chosen
template <int V> static void launch_variant(const SymmArgs& a)
{
    constexpr Variant r = VARIANTS[V];
    if constexpr (!variant_in_build(V)) {
        launch_variant<DEFAULT_VARIANT>(a);
    } else if constexpr (r.fam == Fam::DL) {
        if (!symm_dl_serves(a.p)) return launch_variant<tn_fallback(r.bm)>(a);
        launch_dl<r.bk, r.nstg, r.abl, r.bm, r.nw>(a);
    } else if constexpr (r.abl != 0) {
        // the ablations and the timeline probe (which needs the maxdev buffer) are single products: a pair runs the plain kernel
        if (a.K1 > 0) return launch_variant<tn_fallback(r.bm)>(a);
        launch_tn<r.bm, r.bk, r.wm, r.wn, r.lm, r.abl>(a);
    } else {
        launch_tn<r.bm, r.bk, r.wm, r.wn, r.lm, 0>(a);
    }
}
template <int... V> static void launch_row(int variant, const SymmArgs& a, std::integer_sequence<int, V...>)
{
    if (!((variant == V && (launch_variant<V>(a), true)) || ...)) launch_variant<DEFAULT_VARIANT>(a);
}

// Launch hook of the event timeline (ggl_trace_*, capi_stats.hip): called after every product launch with its stream.
static void (*g_symm_hook)(hipStream_t, int, void*) = nullptr;
static void* g_symm_hook_arg = nullptr;
void symm_set_launch_hook(void (*fn)(hipStream_t, int, void*), void* arg) { g_symm_hook = fn; g_symm_hook_arg = arg; }
struct SymmHookAtExit {
    hipStream_t st; int kind;
    ~SymmHookAtExit() { if (g_symm_hook) g_symm_hook(st, kind, g_symm_hook_arg); }
};

void launch_symm_pair(hipStream_t st, const double* A, const double* B, double* C, const double* A1, const double* B1,
                      double* C1, const double* coef2K, int K, int p, int variant)
{
    SymmHookAtExit hook{st, 1};
    if (variant < 0) variant = symm_auto_variant(2 * K, p);
    launch_row(variant, SymmArgs{st, A, B, C, nullptr, nullptr, nullptr, coef2K, K, p, A1, B1, C1, K, nullptr, nullptr, nullptr},
               std::make_integer_sequence<int, NVARIANT>{});
}

void launch_symm(hipStream_t st, const double* A, const double* B, double* C, double* C2, const double* E,
                 const double* coef, int K, int p, int variant, double* maxdev, double* rowpart, double* fropart,
                 const double* E2)
{
    SymmHookAtExit hook{st, 0};
    if (variant < 0) variant = symm_auto_variant(K, p);
    launch_row(variant, SymmArgs{st, A, B, C, C2, E, E2, coef, K, p, nullptr, nullptr, nullptr, 0, maxdev, rowpart, fropart},
               std::make_integer_sequence<int, NVARIANT>{});
}

}  // namespace ggl

