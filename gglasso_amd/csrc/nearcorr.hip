// Nearest-correlation projection of an indefinite S: the streaming kernels around the L-step's (C - mu I)_+.
// Higham's alternating projections with Dykstra's correction, a batch of B matrices in lock-step:
//     R = Y - dS;  X = eps I + (R - eps I)_+  (rank_step);  dS = X - R;  Y' = X with the diagonal set to 1.
// Every kernel works on 32 x 32 tiles of the upper triangle of tiles: a workgroup reads tile (ti,tj), ti <= tj, uses the
// entries i <= j only, and writes (i,j) and (j,i) from ONE value -- the mirror tile goes through LDS, so both writes are whole
// rows of a tile.  The stacks therefore stay bitwise symmetric whatever the eigen route returned.  Even p: 16-byte loads and
// stores (every row of a stack then starts on an even element); odd p: 8-byte ones.
// No floating-point atomics: sums leave the kernels as per-tile partials and k_nc_reduce adds them in a fixed order.
#include <initializer_list>

#include "common.hpp"

namespace ggl {

namespace {
constexpr int NC_T = 32;            // tile edge
constexpr int NC_LD = NC_T + 1;     // LDS row length (transposed reads without bank conflicts)
constexpr int NC_NT = 256;

// upper-triangular tile index -> (ti, tj), ti <= tj, T tiles per edge
__device__ __forceinline__ void nc_tile(int t, int T, int& ti, int& tj)
{
    ti = 0;
    while (t >= T - ti) { t -= T - ti; ++ti; }
    tj = ti + t;
}

template <int W> struct NcVec;
template <> struct NcVec<1> {
    double v[1];
    __device__ __forceinline__ void load(const double* p) { v[0] = *p; }
    __device__ __forceinline__ void store(double* p) const { *p = v[0]; }
};
template <> struct NcVec<2> {
    double v[2];
    __device__ __forceinline__ void load(const double* p) { const double2 t = *reinterpret_cast<const double2*>(p); v[0] = t.x; v[1] = t.y; }
    __device__ __forceinline__ void store(double* p) const { *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]); }
};

// units of W consecutive columns; a workgroup's thread takes the units tid, tid + 256, ... of its tile
template <int W> struct NcGeom {
    static constexpr int UPR = NC_T / W;                    // units per tile row
    static constexpr int UNITS = NC_T * UPR / NC_NT;        // units per thread
};

// Checks the input (finite, diagonal > 0: *err = smallest offending b * p + i, as k_kendall_diag_check) and forms the
// unit-diagonal A0 = D^-1/2 ((A + A^T) / 2) D^-1/2 with the diagonal set to exactly 1, Y0 = A0, dS0 = 0 and the first R = A0;
// dvec (B,p) = diag(A).  (a + a^T) / 2 leaves a bitwise-symmetric input alone, and d = 1 makes the scaling a division by 1.
template <int W>
__global__ __launch_bounds__(NC_NT) void k_nc_begin(const double* __restrict__ A, double* __restrict__ A0, double* __restrict__ Y,
                                                    double* __restrict__ dS, double* __restrict__ R, double* __restrict__ dvec,
                                                    int* __restrict__ err, int p)
{
    __shared__ double sV[NC_T * NC_LD], sA[NC_T * NC_LD];
    const int T = (p + NC_T - 1) / NC_T, b = blockIdx.y;
    int ti, tj;
    nc_tile(blockIdx.x, T, ti, tj);
    const size_t base = (size_t)b * p * p;
    const double* Ab = A + base;
    constexpr int UPR = NcGeom<W>::UPR, UNITS = NcGeom<W>::UNITS;
    NcVec<W> u[UNITS];
#pragma unroll
    for (int m = 0; m < UNITS; ++m) {
        const int un = threadIdx.x + NC_NT * m, r = un / UPR, c = (un % UPR) * W;
        const int i = ti * NC_T + r, j = tj * NC_T + c;        // tile (ti,tj)
        const int i2 = tj * NC_T + r, j2 = ti * NC_T + c;      // tile (tj,ti)
#pragma unroll
        for (int w = 0; w < W; ++w) u[m].v[w] = 0.0;
        NcVec<W> v;
#pragma unroll
        for (int w = 0; w < W; ++w) v.v[w] = 0.0;
        const bool inu = i < p && j < p, inv = i2 < p && j2 < p;
        if (inu) u[m].load(Ab + (size_t)i * p + j);
        if (inv) v.load(Ab + (size_t)i2 * p + j2);
        bool badu = false, badv = false;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            badu = badu || !isfinite(u[m].v[w]) || (i == j + w && !(u[m].v[w] > 0.0));
            badv = badv || !isfinite(v.v[w]);
            sV[r * NC_LD + c + w] = v.v[w];
        }
        if (inu && badu) atomicMin(err, b * p + i);
        if (inv && badv) atomicMin(err, b * p + i2);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < UNITS; ++m) {
        const int un = threadIdx.x + NC_NT * m, r = un / UPR, c = (un % UPR) * W;
        const int i = ti * NC_T + r;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int j = tj * NC_T + c + w;
            double a = 0.0;
            if (i < p && j < p && i <= j) {
                if (i == j) {
                    a = 1.0;
                    dvec[(size_t)b * p + i] = u[m].v[w];
                } else {
                    const double di = Ab[(size_t)i * p + i], dj = Ab[(size_t)j * p + j];
                    a = (u[m].v[w] + sV[(c + w) * NC_LD + r]) * 0.5 / sqrt(di * dj);
                }
            }
            sA[r * NC_LD + c + w] = a;
        }
    }
    __syncthreads();
    const bool diag = ti == tj;
#pragma unroll
    for (int m = 0; m < UNITS; ++m) {
        const int un = threadIdx.x + NC_NT * m, r = un / UPR, c = (un % UPR) * W;
        const int i = ti * NC_T + r, j = tj * NC_T + c;
        NcVec<W> o, z;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            o.v[w] = (diag && r > c + w) ? sA[(c + w) * NC_LD + r] : sA[r * NC_LD + c + w];
            z.v[w] = 0.0;
        }
        if (i < p && j < p) {
            const size_t e = base + (size_t)i * p + j;
            o.store(A0 + e); o.store(Y + e); o.store(R + e); z.store(dS + e);
        }
        if (!diag) {
            const int i2 = tj * NC_T + r, j2 = ti * NC_T + c;
#pragma unroll
            for (int w = 0; w < W; ++w) o.v[w] = sA[(c + w) * NC_LD + r];
            if (i2 < p && j2 < p) {
                const size_t e = base + (size_t)i2 * p + j2;
                o.store(A0 + e); o.store(Y + e); o.store(R + e); z.store(dS + e);
            }
        }
    }
}

// One pass per iteration.  X = L + eps I (L: rank_step's (R - eps I)_+, upper triangle read), with Y and dS of the stacks:
//     dS' = X - (Y - dS),  Y' = X with the diagonal 1,  R' = Y' - dS'   (R' into the stack rank_step reads next)
// part[b][tile][3] = sum (Y' - Y)^2, sum_i (1 - x_ii)^2, sum Y'^2 over the tile and its mirror.  An instance whose frozen flag
// is set keeps Y and dS; its R becomes the identity, so that it costs the batch's next rank_step no resolution.
template <int W>
__global__ __launch_bounds__(NC_NT) void k_nc_update(const double* __restrict__ L, double* __restrict__ Y, double* __restrict__ dS,
                                                     double* __restrict__ R, double* __restrict__ part,
                                                     const int* __restrict__ frozen, const int* __restrict__ err, double eps, int p)
{
    if (*err != GGL_DIAG_OK) return;
    __shared__ double sY[NC_T * NC_LD], sD[NC_T * NC_LD], red[3 * NC_NT / 64];
    const int T = (p + NC_T - 1) / NC_T, b = blockIdx.y;
    int ti, tj;
    nc_tile(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj, hold = frozen[b] != 0;
    const size_t base = (size_t)b * p * p;
    constexpr int UPR = NcGeom<W>::UPR, UNITS = NcGeom<W>::UNITS;
    double s[3] = {0.0, 0.0, 0.0};
    if (!hold) {
        NcVec<W> x[UNITS], y[UNITS], d[UNITS];
#pragma unroll
        for (int m = 0; m < UNITS; ++m) {
            const int un = threadIdx.x + NC_NT * m, r = un / UPR, c = (un % UPR) * W;
            const int i = ti * NC_T + r, j = tj * NC_T + c;
#pragma unroll
            for (int w = 0; w < W; ++w) x[m].v[w] = y[m].v[w] = d[m].v[w] = 0.0;
            if (i < p && j < p && (!diag || r <= c + W - 1)) {
                const size_t e = base + (size_t)i * p + j;
                x[m].load(L + e); y[m].load(Y + e); d[m].load(dS + e);
            }
        }
#pragma unroll
        for (int m = 0; m < UNITS; ++m) {
            const int un = threadIdx.x + NC_NT * m, r = un / UPR, c = (un % UPR) * W;
            const int i = ti * NC_T + r;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int j = tj * NC_T + c + w;
                double yn = 0.0, dn = 0.0;
                if (i < p && j < p && i <= j) {
                    const bool on = i == j;
                    const double xv = x[m].v[w] + (on ? eps : 0.0);
                    dn = xv - (y[m].v[w] - d[m].v[w]);
                    yn = on ? 1.0 : xv;
                    const double wgt = on ? 1.0 : 2.0, dy = yn - y[m].v[w];
                    s[0] += wgt * (dy * dy);
                    if (on) s[1] += (1.0 - xv) * (1.0 - xv);
                    s[2] += wgt * (yn * yn);
                }
                sY[r * NC_LD + c + w] = yn;
                sD[r * NC_LD + c + w] = dn;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < UNITS; ++m) {
        const int un = threadIdx.x + NC_NT * m, r = un / UPR, c = (un % UPR) * W;
        const int i = ti * NC_T + r, j = tj * NC_T + c;
        NcVec<W> oy, od, orr;
        if (i < p && j < p) {
            const size_t e = base + (size_t)i * p + j;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (hold) {
                    orr.v[w] = (i == j + w) ? 1.0 : 0.0;
                } else {
                    const int a = (diag && r > c + w) ? (c + w) * NC_LD + r : r * NC_LD + c + w;
                    oy.v[w] = sY[a];
                    od.v[w] = sD[a];
                    orr.v[w] = oy.v[w] - od.v[w];
                }
            }
            if (!hold) { oy.store(Y + e); od.store(dS + e); }
            orr.store(R + e);
        }
        const int i2 = tj * NC_T + r, j2 = ti * NC_T + c;
        if (!diag && i2 < p && j2 < p) {
            const size_t e = base + (size_t)i2 * p + j2;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (hold) {
                    orr.v[w] = 0.0;
                } else {
                    const int a = (c + w) * NC_LD + r;
                    oy.v[w] = sY[a];
                    od.v[w] = sD[a];
                    orr.v[w] = oy.v[w] - od.v[w];
                }
            }
            if (!hold) { oy.store(Y + e); od.store(dS + e); }
            orr.store(R + e);
        }
    }
    if (hold) return;
    block_sum<3>(s, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
}

// out[b][v] = sum over the nblk partials of instance b, v < nv <= 3: one wave per instance, every lane adds its partials in
// order, then the fixed butterfly of wave_sum -- the same bits from every call.  out may be pinned host memory (row length 8).
__global__ __launch_bounds__(64) void k_nc_reduce(const double* __restrict__ part, double* __restrict__ out, const int* __restrict__ err,
                                                  int nblk, int nv)
{
    if (*err != GGL_DIAG_OK) return;
    const int b = blockIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < nblk; t += 64)
        for (int v = 0; v < nv; ++v) s[v] += part[((size_t)b * nblk + t) * nv + v];
    for (int v = 0; v < nv; ++v) {
        const double r = wave_sum(s[v]);
        if (threadIdx.x == 0) out[(size_t)b * 8 + v] = r;
    }
}

// dst = (1 - nu_b) Y off the diagonal, scaled back by sqrt(d_i d_j); the diagonal is d_i itself.  An instance whose pass flag
// is set gets its input back bit for bit.  part[b][block] = sum (dst - A)^2.  dst may be A (every thread reads the entries it
// writes first).
template <int W>
__global__ __launch_bounds__(NC_NT) void k_nc_finish(const double* __restrict__ Y, const double* A, double* dst,
                                                     const double* __restrict__ dvec, const double* __restrict__ nu,
                                                     const int* __restrict__ pass, double* __restrict__ part,
                                                     const int* __restrict__ err, int p)
{
    if (*err != GGL_DIAG_OK) return;
    __shared__ double red[NC_NT / 64];
    const int b = blockIdx.y;
    const size_t pp = (size_t)p * p, base = (size_t)b * pp;
    const bool keep = pass[b] != 0;
    const double shrink = 1.0 - nu[b];
    const double* db = dvec + (size_t)b * p;
    double s[1] = {0.0};
    const size_t e = ((size_t)blockIdx.x * NC_NT + threadIdx.x) * W;
    if (e < pp) {
        const int i = (int)(e / p), j = (int)(e % p);       // (W = 2: p is even, the pair stays in row i)
        NcVec<W> a, y, o;
        a.load(A + base + e);
        y.load(Y + base + e);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            o.v[w] = keep ? a.v[w] : (i == j + w ? db[i] : y.v[w] * shrink * sqrt(db[i] * db[j + w]));
            const double df = o.v[w] - a.v[w];
            s[0] += df * df;
        }
        if (!keep || dst != A) o.store(dst + base + e);
    }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = s[0];
}

inline bool nc_vec(int p, std::initializer_list<const void*> ptrs)
{
    if (p & 1) return false;
    for (const void* q : ptrs)
        if ((uintptr_t)q & 15) return false;
    return true;
}
}  // namespace

int nc_update_blocks(int p) { const int T = (p + NC_T - 1) / NC_T; return T * (T + 1) / 2; }
int nc_finish_blocks(int p) { return (int)(((size_t)p * p + NC_NT - 1) / NC_NT); }   // (enough for either load width)

void launch_nc_begin(hipStream_t st, const double* A, double* A0, double* Y, double* dS, double* R, double* dvec, int* err, int B,
                     int p)
{
    const dim3 grid(nc_update_blocks(p), B);
    if (nc_vec(p, {A, A0, Y, dS, R}))
        hipLaunchKernelGGL(k_nc_begin<2>, grid, dim3(NC_NT), 0, st, A, A0, Y, dS, R, dvec, err, p);
    else
        hipLaunchKernelGGL(k_nc_begin<1>, grid, dim3(NC_NT), 0, st, A, A0, Y, dS, R, dvec, err, p);
}

void launch_nc_update(hipStream_t st, const double* L, double* Y, double* dS, double* R, double* part, const int* frozen,
                      const int* err, double eps, int B, int p)
{
    const dim3 grid(nc_update_blocks(p), B);
    if (nc_vec(p, {L, Y, dS, R}))
        hipLaunchKernelGGL(k_nc_update<2>, grid, dim3(NC_NT), 0, st, L, Y, dS, R, part, frozen, err, eps, p);
    else
        hipLaunchKernelGGL(k_nc_update<1>, grid, dim3(NC_NT), 0, st, L, Y, dS, R, part, frozen, err, eps, p);
}

void launch_nc_reduce(hipStream_t st, const double* part, double* out, const int* err, int B, int nblk, int nv)
{
    hipLaunchKernelGGL(k_nc_reduce, dim3(B), dim3(64), 0, st, part, out, err, nblk, nv);
}

void launch_nc_finish(hipStream_t st, const double* Y, const double* A, double* dst, const double* dvec, const double* nu,
                      const int* pass, double* part, const int* err, int B, int p)
{
    const dim3 grid(nc_finish_blocks(p), B);
    if (nc_vec(p, {Y, A, dst}))
        hipLaunchKernelGGL(k_nc_finish<2>, grid, dim3(NC_NT), 0, st, Y, A, dst, dvec, nu, pass, part, err, p);
    else
        hipLaunchKernelGGL(k_nc_finish<1>, grid, dim3(NC_NT), 0, st, Y, A, dst, dvec, nu, pass, part, err, p);
}

}  // namespace ggl
