// Kendall's tau-b between every pair of variables, and the nonparanormal skeptic matrix sin(pi/2 tau) (Liu, Han, Yuan,
// Lafferty, Wasserman 2012), on the int8 matrix cores -- the rank-based input statistic of the solvers.
//
//     Z[i,(a,b)] = sgn(R[i,a] - R[i,b])  in {-1,0,1},  one column per sample pair a < b          (never in memory)
//     G          = Z Z^T:   G_ij = concordant - discordant pairs of (i,j),  G_ii = pairs not tied in i    k_kendall_counts
//     tau_b      = G_ij / sqrt(G_ii G_jj),   S_ij = sin(pi/2 tau_b),  S_ii = 1                             k_kendall_skeptic
//
// R holds dense integer ranks (equal values, equal ranks), so the sign of a rank difference is the sign of the value
// difference, also on any subset of the columns: B subsamples are one upload of R and an index array, gathered on the device
// (k_gather_ranks) into B packed (p,b) arrays.
//
// Tiling of k_kendall_counts.  A workgroup owns a tile pair I <= J of T x T variables (T = 64), one subset, one block of 64
// b-samples [b0, b0 + 64) and a chunk of at most KD_ACH a-samples; its four waves take the a-samples of the chunk in turn and
// each accumulates the WHOLE tile.  One a-sample against the 64 b-samples is one k = 64 step of v_mfma_i32_16x16x64_i8: lane l
// holds, per group of 16 variables, the 16 signs of variable (l & 15) against the b-samples b0 + 16 (l >> 4) + j -- generated
// in registers from the lane's 16 rank values (loaded once per workgroup) and the one rank value at a, so a sign row is built
// once per wave and serves all four 16 x 16 blocks of its row (one generated sign per 32 multiply-adds, no LDS on the way).
// Both operands use the same lane -> k map, and a sum over k does not depend on the order of k: only the row map (l & 15) and
// the C/D map (column l & 15, row 4 (l >> 4) + register) enter the result.  Pairs with a >= b (the blocks on the diagonal of
// the pair space) and b-samples beyond the subset are zeroed by a byte mask on the packed signs; rows beyond p are computed on
// a clamped row and never stored.
//
// Exactness.  A workgroup sums at most KD_ACH * 64 = 2^16 sign products per element, in int32 registers and an int32 LDS
// tile; the tile leaves as one 64-bit atomic add per element (and one for the mirror element, so G is symmetric without a
// second product).  Integer sums do not depend on their order: two calls return the same bits.
//
// What bounds it: the VALU.  A sign costs a subtraction, a v_med3_i32 and 3/4 of an instruction to pack it against 32 multiply-adds on the
// matrix core; DESIGN has the measurement.
#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

typedef int kd_v4i __attribute__((ext_vector_type(4)));

static constexpr int KD_T = 64;          // variables per tile side
static constexpr int KD_M = KD_T / 16;   // 16-row groups per tile side
static constexpr int KD_KB = 64;         // b-samples per block = the k of one MFMA
static constexpr int KD_ACH = 1024;      // a-samples per workgroup

// out[r,i,c] = R[i, idx[r,c]]: one thread per column of a subset, KD_GROWS rows per thread (k_gather_cols for ints)
static constexpr int KD_GROWS = 8;

__global__ __launch_bounds__(256) void k_gather_ranks(const int* __restrict__ R, const int* __restrict__ idx,
                                                      int* __restrict__ out, int p, int N, int b)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.z;
    if (c >= b) return;
    const int i0 = blockIdx.y * KD_GROWS;
    const int* x = R + idx[(size_t)r * b + c];
    int* o = out + (size_t)r * p * b + c;
    int v[KD_GROWS];
#pragma unroll
    for (int q = 0; q < KD_GROWS; ++q) v[q] = x[(size_t)min(i0 + q, p - 1) * N];          // clamped: always a valid row
#pragma unroll
    for (int q = 0; q < KD_GROWS; ++q)
        if (i0 + q < p) o[(size_t)(i0 + q) * b] = v[q];
}

// sgn(d) of a 32-bit difference.  (Written as min(max(d, -1), 1) the clamp is compiled to two compares and two selects; the
// instruction is named instead.)
__device__ __forceinline__ int kd_sgn(int d)
{
    int s;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(s) : "v"(d));
    return s;
}

// the 16 signs sgn(ra - rb[j]) as int8, j ascending from the low byte of word 0.  v_perm_b32 takes the low bytes of two signs
// at a time (selector 0 .. 3: a byte of the second operand, 4 .. 7: of the first, 0x0c: zero): 3 instructions per 4 signs
__device__ __forceinline__ kd_v4i kd_signs(int ra, const int (&rb)[16])
{
    kd_v4i f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned s0 = kd_sgn(ra - rb[4 * q]), s1 = kd_sgn(ra - rb[4 * q + 1]);
        const unsigned s2 = kd_sgn(ra - rb[4 * q + 2]), s3 = kd_sgn(ra - rb[4 * q + 3]);
        f[q] = (int)(__builtin_amdgcn_perm(s1, s0, 0x0c0c0400u) | __builtin_amdgcn_perm(s3, s2, 0x04000c0cu));
    }
    return f;
}

// bytes [0, t) of a word set, t clamped to 0 .. 4
__device__ __forceinline__ unsigned kd_low_bytes(int t)
{
    return t >= 4 ? 0xffffffffu : (t <= 0 ? 0u : ((1u << (8 * t)) - 1u));
}

template <bool DIAG>
__device__ __forceinline__ void kd_tile(const int* __restrict__ Rr, int p, int n, int I0, int J0, int b0, int a_lo, int a_end,
                                        int (*red)[KD_T + 1])
{
    const int lane = threadIdx.x & 63, lr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bq = b0 + 16 * g;                         // the lane's first b-sample

    // the lane's rows (clamped: a row beyond p is computed and not stored) and their 16 rank values of the b-block
    int rowI[KD_M], rowJ[KD_M];                         // offsets into Rr (p n < 2^31: kendall_counts_fit)
    int rbI[KD_M][16], rbJ[DIAG ? 1 : KD_M][16];
#pragma unroll
    for (int m = 0; m < KD_M; ++m) {
        rowI[m] = min(I0 + 16 * m + lr, p - 1) * n;
        rowJ[m] = min(J0 + 16 * m + lr, p - 1) * n;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int bpos = min(bq + j, n - 1);        // beyond the subset: masked below
            rbI[m][j] = Rr[rowI[m] + bpos];
            if (!DIAG) rbJ[m][j] = Rr[rowJ[m] + bpos];
        }
    }

    kd_v4i acc[KD_M][KD_M];
#pragma unroll
    for (int i = 0; i < KD_M; ++i)
#pragma unroll
        for (int j = 0; j < KD_M; ++j) acc[i][j] = (kd_v4i){0, 0, 0, 0};

    const bool tail = b0 + KD_KB > n;                   // the block reaches beyond the subset: every step is masked
    int a = a_lo + wave;
    int raI[KD_M], raJ[DIAG ? 1 : KD_M];
    {
        const int a0 = min(a, a_end - 1);
#pragma unroll
        for (int m = 0; m < KD_M; ++m) {
            raI[m] = Rr[rowI[m] + a0];
            if (!DIAG) raJ[m] = Rr[rowJ[m] + a0];
        }
    }
    for (; a < a_end; a += 4) {
        // the next step's values are on their way while this step's signs are built
        int nI[KD_M], nJ[DIAG ? 1 : KD_M];
        const int an = min(a + 4, a_end - 1);
#pragma unroll
        for (int m = 0; m < KD_M; ++m) {
            nI[m] = Rr[rowI[m] + an];
            if (!DIAG) nJ[m] = Rr[rowJ[m] + an];
        }
        kd_v4i af[KD_M];
#pragma unroll
        for (int m = 0; m < KD_M; ++m) af[m] = kd_signs(raI[m], rbI[m]);
        if (tail || a >= b0) {
            // valid j of this lane: a < bq + j < n
            const int lo = a - bq + 1, hi = n - bq;
            kd_v4i mk;
#pragma unroll
            for (int q = 0; q < 4; ++q) mk[q] = (int)(kd_low_bytes(hi - 4 * q) & ~kd_low_bytes(lo - 4 * q));
#pragma unroll
            for (int m = 0; m < KD_M; ++m) af[m] &= mk;        // (a zero in one operand zeroes the product)
        }
        // the J-side rows are built one group at a time, each followed by its four products: the matrix core works on one
        // column of blocks while the VALU builds the next operand
#pragma unroll
        for (int j = 0; j < KD_M; ++j) {
            const kd_v4i bf = DIAG ? af[j] : kd_signs(raJ[DIAG ? 0 : j], rbJ[DIAG ? 0 : j]);
#pragma unroll
            for (int i = 0; i < KD_M; ++i) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf, acc[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < KD_M; ++m) {
            raI[m] = nI[m];
            if (!DIAG) raJ[m] = nJ[m];
        }
    }

    // the four waves' partial tiles meet in LDS (C/D map of the 16 x 16 i32 MFMA: column lane & 15, row 4 (lane >> 4) + reg)
#pragma unroll
    for (int i = 0; i < KD_M; ++i)
#pragma unroll
        for (int j = 0; j < KD_M; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                atomicAdd(&red[16 * i + 4 * g + r][16 * j + lr], acc[i][j][r]);
}

__global__ __launch_bounds__(256) void k_kendall_counts(const int* __restrict__ Rg, int p, int n, int nb, int nac,
                                                        unsigned long long* __restrict__ G)
{
    __shared__ int red[KD_T][KD_T + 1];
    // blockIdx.x: the slice (b-block, a-chunk), the long b-blocks first; blockIdx.y: the tile pair; blockIdx.z: the subset
    const int sl = blockIdx.x;
    int tp = blockIdx.y;
    const int b0 = (nb - 1 - sl / nac) * KD_KB;
    const int a_lo = (sl % nac) * KD_ACH;
    const int a_end = min(a_lo + KD_ACH, min(b0 + KD_KB - 1, n - 1));       // a < b <= min(b0 + 63, n - 1)
    if (a_lo >= a_end) return;                                             // (the whole workgroup)
    const int nT = (p + KD_T - 1) / KD_T;
    int I = 0;
    while (tp >= nT - I) { tp -= nT - I; ++I; }
    const int J = I + tp;
    const int I0 = I * KD_T, J0 = J * KD_T;
    const int r = blockIdx.z;
    const int* Rr = Rg + (size_t)r * p * n;

    for (int e = threadIdx.x; e < KD_T * (KD_T + 1); e += 256) (&red[0][0])[e] = 0;
    __syncthreads();
    if (I == J) kd_tile<true>(Rr, p, n, I0, J0, b0, a_lo, a_end, red);
    else kd_tile<false>(Rr, p, n, I0, J0, b0, a_lo, a_end, red);
    __syncthreads();

    unsigned long long* Gr = G + (size_t)r * p * p;
    for (int e = threadIdx.x; e < KD_T * KD_T; e += 256) {
        const int row = e / KD_T, col = e % KD_T;
        const int gi = I0 + row, gj = J0 + col;
        const int v = red[row][col];
        if (v == 0 || gi >= p || gj >= p) continue;
        const unsigned long long add = (unsigned long long)(long long)v;
        atomicAdd(Gr + (size_t)gi * p + gj, add);
        if (I != J) atomicAdd(Gr + (size_t)gj * p + gi, add);              // the mirror tile
    }
}

void launch_gather_ranks(hipStream_t st, const int* R, const int* idx, int* out, int p, int N, int B, int b)
{
    hipLaunchKernelGGL(k_gather_ranks, dim3((b + 255) / 256, (p + KD_GROWS - 1) / KD_GROWS, B), dim3(256), 0, st, R, idx, out, p,
                       N, b);
}

// What a launch accepts: 256 * grid.x below 2^32 (the slices), grid.y and grid.z at most 65535 (tile pairs, subsets); and the
// offsets into one subset's ranks are 32-bit.
bool kendall_counts_fit(int p, int n, int B)
{
    const long long nT = (p + KD_T - 1) / KD_T, nb = (n + KD_KB - 1) / KD_KB, nac = (n + KD_ACH - 1) / KD_ACH;
    return nb * nac < (1ll << 24) && nT * (nT + 1) / 2 <= 65535 && (long long)p * n < (1ll << 31) && B <= 65535;
}

void launch_kendall_counts(hipStream_t st, const int* Rg, long long* G, int B, int p, int n)
{
    const int nT = (p + KD_T - 1) / KD_T, nb = (n + KD_KB - 1) / KD_KB, nac = (n + KD_ACH - 1) / KD_ACH;
    (void)hipMemsetAsync(G, 0, (size_t)B * p * p * sizeof(long long), st);
    hipLaunchKernelGGL(k_kendall_counts, dim3((unsigned)(nb * nac), (unsigned)(nT * (nT + 1) / 2), B), dim3(256), 0, st, Rg, p, n, nb, nac,
                       reinterpret_cast<unsigned long long*>(G));
}

// *err (GGL_DIAG_OK from the caller) = smallest r * p + i with G[r,i,i] = 0: variable i is constant over subset r
__global__ __launch_bounds__(256) void k_kendall_diag_check(const long long* __restrict__ G, int* __restrict__ err, int p)
{
    const int i = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (i >= p) return;
    if (G[(size_t)r * p * p + (size_t)i * p + i] <= 0) atomicMin(err, r * p + i);
}

// S[r,i,j] = sin(pi/2 G_ij / sqrt(G_ii G_jj)); the diagonal is 1; (i,j) and (j,i) evaluate the same expression on the same
// integers, so S is bitwise symmetric.  Nothing is written once the check above found a constant variable.
__global__ __launch_bounds__(256) void k_kendall_skeptic(const long long* __restrict__ G, double* __restrict__ S,
                                                         const int* __restrict__ err, int p)
{
    if (*err != GGL_DIAG_OK) return;
    const size_t pp = (size_t)p * p;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pp) return;
    const int i = (int)(e / p), j = (int)(e % p);
    const long long* Gr = G + blockIdx.y * pp;
    double s = 1.0;
    if (i != j) {
        const double tau = (double)Gr[e] / sqrt((double)Gr[(size_t)i * p + i] * (double)Gr[(size_t)j * p + j]);
        s = sin(1.5707963267948966 * tau);
    }
    S[blockIdx.y * pp + e] = s;
}

void launch_kendall_skeptic(hipStream_t st, const long long* G, double* S, int* err, int B, int p)
{
    hipLaunchKernelGGL(k_kendall_diag_check, dim3((p + 255) / 256, B), dim3(256), 0, st, G, err, p);
    const size_t pp = (size_t)p * p;
    hipLaunchKernelGGL(k_kendall_skeptic, dim3((unsigned)((pp + 255) / 256), B), dim3(256), 0, st, G, S, err, p);
}

}  // namespace ggl
