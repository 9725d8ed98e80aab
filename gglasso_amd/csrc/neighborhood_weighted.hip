// Neighbourhood selection with per-entry penalty weights and the scaled lasso: k_mb_path's procedure
// (neighborhood.hip) with the threshold of coordinate k in node j's lasso  lambda sigma_j w_jk  instead of lambda.
//
//     plain  (mode 0):  min 1/2 beta' S beta - s_j' beta + lambda0 sum_k w_k |beta_k|          thr_k = lambda0 w_k
//     scaled (mode 1):  min sqrt(tau^2(beta)) + lambda0 sum_k w_k |beta_k|                      thr_k = lambda0 sigma w_k
//     tau^2(beta) = S_jj - 2 s_j' beta + beta' S beta,  sigma = sqrt(tau^2),  w_k = Wt[j,k] in [0, +inf]
//
// Weights (the adaptive lasso of Zou 2006, JASA 101; glmnet's penalty.factor): w_k = 0 is an unpenalised coordinate, it joins
// at the first screen; w_k = +inf excludes one -- |g_k| > inf is never true, so it never joins and its beta_k stays the exact
// zero it was set to.  The scaled lasso (Sun & Zhang 2012, Biometrika 99; the square-root lasso of Belloni, Chernozhukov, Wang
// 2011, Biometrika 98; TIGER, Liu & Wang 2017, EJS 11) is the alternation of Sun & Zhang around the plain procedure, per
// (node, lambda0):  sigma_t = sqrt(tau^2) of the warm start (sqrt(S_jj) at the first lambda0) -> the plain procedure to its
// finished state at thresholds (lambda0 sigma_t) w_k -> tau^2 by the formula below, sigma_new = sqrt(tau^2) -> finished if
// |sigma_new - sigma_t| <= sig_tol sigma_new, else sigma_t = sigma_new, at most max_outer times.  Plain mode runs the
// procedure once; with unit weights it is k_mb_path's arithmetic (lambda * 1.0 is exact).
//
// One wave per (matrix, node) as there; beta, the node's weights (ROW j of Wt, one contiguous read) and the active list live
// in LDS, 20 p bytes per unit: the sweep reads w_k for a wave-uniform k (a broadcast read, like beta[k]), the screen reads w
// lane-distributed.  No barrier in the coordinate loop, every value that steers a loop is wave-uniform (sigma and tau^2 are
// read from lane 0), fixed orders, no atomics.  Statuses: 0 finished, 1 a cap was reached (sweeps, screens, outer
// iterations), 2 a non-finite value, 3 (scaled) tau^2 <= 1e-10 S_jj or not positive -- a duplicated variable or a perfect
// fit, where sigma decays geometrically and the relative test can never end the loop.  2 and 3: the node is NaN (diagonal 0)
// at this and every later lambda0.  Nothing can hang: max_outer, max_sweeps and MBW_MAX_ROUNDS are trip-count caps and every
// continuing comparison is false for a NaN.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

static constexpr int MBW_MAX_ROUNDS = 100;
static constexpr double MBW_TAU_FLOOR = 1e-10;

__device__ __forceinline__ double mbw_lane_read(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ bool mbw_not_finite(double x) { return !(fabs(x) <= 1.79769313486231570815e308); }

// SCALED is a template parameter because the resource report says that it pays: as a runtime argument the alternation's state
// (sigma, tau^2, the outer counters) costs the plain body 10 to 16 VGPRs and with them one wave per SIMD at 4 and at 8 slots.
template <int NV, int WPB, bool SCALED>
__global__ __launch_bounds__(64 * WPB) void k_mb_path_w(const double* __restrict__ S, int M, int p,
                                                        const double* __restrict__ Wt, size_t wstride,
                                                        const double* __restrict__ lam, int L, double tol,
                                                        int max_sweeps, double sig_tol, int max_outer,
                                                        double* __restrict__ coef, double* __restrict__ resvar,
                                                        int* __restrict__ info, size_t strideM, size_t strideL)
{
    extern __shared__ __attribute__((aligned(16))) char mbw_smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long unit = (long long)blockIdx.x * WPB + w;                 // m-major: the units of one matrix are adjacent
    if (unit >= (long long)M * p) return;                                   // a whole wave; no barrier follows
    const int m = (int)(unit / p), j = (int)(unit % p);
    const size_t pp = (size_t)p * p;
    const double* Sm = S + (size_t)m * pp;
    double* beta = reinterpret_cast<double*>(mbw_smem) + (size_t)w * p;
    double* wts = reinterpret_cast<double*>(mbw_smem) + (size_t)(WPB + w) * p;
    int* act = reinterpret_cast<int*>(reinterpret_cast<double*>(mbw_smem) + (size_t)2 * WPB * p) + (size_t)w * p;
    const unsigned long long below = (1ull << lane) - 1ull;

    double g[NV];
    unsigned mem = 0;                                                       // bit v: variable v * 64 + lane is active
    int na = 0;

    auto load_row = [&](int k, double (&r)[NV]) {
        const double* row = Sm + (size_t)k * p;
#pragma unroll
        for (int v = 0; v < NV; ++v) r[v] = (v * 64 + lane < p) ? row[v * 64 + lane] : 0.0;
    };
    // element k of a distributed vector, k wave-uniform (the slot is chosen among scalars: see k_mb_path)
    auto pick = [&](const double (&a)[NV], int k) -> double {
        const int kv = k >> 6, kl = k & 63;
        double x = mbw_lane_read(a[0], kl);
#pragma unroll
        for (int v = 1; v < NV; ++v) {
            const double t = mbw_lane_read(a[v], kl);
            x = (kv == v) ? t : x;
        }
        return x;
    };
    auto active_at = [&](int i) -> int { return __builtin_amdgcn_readfirstlane(act[i]); };

    // one pass over the active set, ascending, at thresholds ls * w_k; returns max |d| S_kk
    auto sweep = [&](double ls) -> double {
        double dmax = 0.0, cur[NV], nxt[NV];
        if (na > 0) load_row(active_at(0), cur);
        for (int i = 0; i < na; ++i) {
            const int k = active_at(i);
            load_row(active_at(min(i + 1, na - 1)), nxt);
            const double skk = pick(cur, k), gk = pick(g, k), bk = beta[k];
            const double b = soft(gk + skk * bk, ls * wts[k]) / skk;
            const double d = b - bk;
            if (d != 0.0) {
#pragma unroll
                for (int v = 0; v < NV; ++v) g[v] -= d * cur[v];
                beta[k] = b;                                                // every lane the same value
            }
            const double c = fabs(d) * skk;
            dmax = c > dmax ? c : dmax;
#pragma unroll
            for (int v = 0; v < NV; ++v) cur[v] = nxt[v];
        }
        __builtin_amdgcn_wave_barrier();
        return dmax;
    };
    // every violator joins; the list is rebuilt in ascending order
    auto screen = [&](double ls) -> int {
        int added = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int idx = v * 64 + lane;
            const bool viol = idx < p && idx != j && !((mem >> v) & 1u) && fabs(g[v]) > ls * wts[idx < p ? idx : 0];
            if (viol) mem |= 1u << v;
            added += __popcll(__ballot(viol));
        }
        if (added) {
            int base = 0;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const bool in = (mem >> v) & 1u;
                const unsigned long long bal = __ballot(in);
                if (in) act[base + __popcll(bal & below)] = v * 64 + lane;
                base += __popcll(bal);
            }
            na = base;
            __builtin_amdgcn_wave_barrier();
        }
        return added;
    };
    // g = s_j - sum over the active set, ascending, of beta_l S[l, :]
    auto recompute = [&]() {
        double cur[NV], nxt[NV];
        load_row(j, g);
        if (na > 0) load_row(active_at(0), cur);
        for (int i = 0; i < na; ++i) {
            const double bk = beta[active_at(i)];
            load_row(active_at(min(i + 1, na - 1)), nxt);
            if (bk != 0.0) {
#pragma unroll
                for (int v = 0; v < NV; ++v) g[v] -= bk * cur[v];
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) cur[v] = nxt[v];
        }
    };
    auto bad = [&]() -> bool {
        bool nf = false;
#pragma unroll
        for (int v = 0; v < NV; ++v) nf |= (v * 64 + lane < p) && mbw_not_finite(g[v]);
        for (int i = lane; i < na; i += 64) nf |= mbw_not_finite(beta[act[i]]);
        return __ballot(nf) != 0ull;
    };
    // tau^2 = S_jj - s_j' beta - beta' g: a lane adds its active slots in ascending order, then the butterfly
    auto tau2 = [&]() -> double {
        double sj[NV], acc = 0.0;
        load_row(j, sj);
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if ((mem >> v) & 1u) acc += beta[v * 64 + lane] * (sj[v] + g[v]);
        return mbw_lane_read(pick(sj, j) - wave_sum(acc), 0);
    };

    const double* wrow = Wt ? Wt + (size_t)m * wstride + (size_t)j * p : nullptr;
    for (int i = lane; i < p; i += 64) {
        beta[i] = 0.0;
        wts[i] = wrow ? wrow[i] : 1.0;
    }
    __builtin_amdgcn_wave_barrier();
    load_row(j, g);
    const double sjj = pick(g, j);
    double tau = sjj;                                                       // tau^2 of the warm start: beta = 0
    bool dead = false;
    int dead_status = 2;
    const int nouter = SCALED ? max_outer : 1;

    for (int l = 0; l < L; ++l) {
        const double lamv = lam[l];
        int sweeps = 0, status = 1, outer = 0;
        if (dead) {
            status = dead_status;
        } else if (bad()) {
            status = 2;
        } else {
            double sig = SCALED ? mbw_lane_read(sqrt(tau), 0) : 1.0;           // (lane 0's: kept in scalar registers)
            for (int it = 0; it < nouter; ++it) {
                const double ls = SCALED ? mbw_lane_read(lamv * sig, 0) : lamv;
                int st = 1;
                double d1 = 0.0;
                for (int round = 0; round < MBW_MAX_ROUNDS; ++round) {
                    const int nviol = screen(ls);
                    if (nviol == 0 && (round > 0 ? !(d1 > tol) : na == 0)) { st = 0; break; }
                    bool conv = false;
                    while (sweeps < max_sweeps) {
                        const double dm = sweep(ls);
                        ++sweeps;
                        if (!(dm > tol)) { conv = true; break; }
                    }
                    if (!conv) break;                                       // max_sweeps reached
                    recompute();
                    if (sweeps >= max_sweeps) break;
                    d1 = sweep(ls);
                    ++sweeps;
                    if (bad()) { st = 2; break; }
                }
                if (st == 1 && bad()) st = 2;
                ++outer;
                if (!SCALED) { status = st; break; }
                if (st == 2) { status = 2; break; }
                tau = tau2();
                if (!(tau > MBW_TAU_FLOOR * sjj)) { status = 3; break; }
                if (st == 1) break;                                         // a cap of the inner procedure: status 1
                const double sn = mbw_lane_read(sqrt(tau), 0);
                const bool done = fabs(sn - sig) <= sig_tol * sn;
                sig = sn;
                if (done) { status = 0; break; }
            }
        }
        if (status >= 2) { dead = true; dead_status = status; }

        const size_t unit_out = (size_t)m * strideM + (size_t)l * strideL;
        double* out = coef + unit_out * pp + (size_t)j * p;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int idx = v * 64 + lane;
            if (idx < p) out[idx] = dead ? (idx == j ? 0.0 : __builtin_nan("")) : beta[idx];
        }
        if (resvar) {
            if (!SCALED && !dead) tau = tau2();
            if (lane == 0) resvar[unit_out * p + j] = dead ? __builtin_nan("") : tau;
        }
        if (lane == 0) {
            int* o = info + (unit_out * p + j) * 3;
            o[0] = sweeps;
            o[1] = status;
            o[2] = SCALED ? outer : 0;
        }
    }
}

template <int NV, int WPB, bool SCALED>
static hipError_t mbw_launch(hipStream_t st, const double* S, int M, int p, const double* Wt, size_t wstride, const double* lam,
                             int L, double tol, int max_sweeps, double sig_tol, int max_outer, double* coef, double* resvar,
                             int* info, size_t strideM, size_t strideL)
{
    const long long units = (long long)M * p;
    const size_t lds = (size_t)WPB * p * (2 * sizeof(double) + sizeof(int));
    if (lds > 64 * 1024) {
        // per launch: the attribute belongs to the current device's copy of the kernel
        const hipError_t e = hipFuncSetAttribute((const void*)k_mb_path_w<NV, WPB, SCALED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_mb_path_w<NV, WPB, SCALED>), dim3((unsigned)((units + WPB - 1) / WPB)), dim3(64 * WPB), lds, st, S, M, p,
                       Wt, wstride, lam, L, tol, max_sweeps, sig_tol, max_outer, coef, resvar, info, strideM, strideL);
    return hipGetLastError();
}

// (the caller checked 1 <= p <= MB_MAX_P, M * p < 2^31, mode 0 or 1, max_outer >= 1)
hipError_t launch_mb_path_w(hipStream_t st, const double* S, int M, int p, const double* Wt, size_t wstride, const double* lam,
                            int L, int mode, double tol, int max_sweeps, double sig_tol, int max_outer, double* coef,
                            double* resvar, int* info, size_t strideM, size_t strideL)
{
#define GGL_MBW(NV, WPB)                                                                                                        \
    (mode ? mbw_launch<NV, WPB, true>(st, S, M, p, Wt, wstride, lam, L, tol, max_sweeps, sig_tol, max_outer, coef, resvar, info,  \
                                      strideM, strideL)                                                                          \
          : mbw_launch<NV, WPB, false>(st, S, M, p, Wt, wstride, lam, L, tol, max_sweeps, sig_tol, max_outer, coef, resvar, info, \
                                       strideM, strideL))
    if (p <= 256) return GGL_MBW(4, 4);
    if (p <= 512) return GGL_MBW(8, 4);
    if (p <= 1024) return GGL_MBW(16, 4);
    return GGL_MBW(32, 2);
#undef GGL_MBW
}

}  // namespace ggl
