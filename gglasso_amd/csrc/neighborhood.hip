// Meinshausen-Buhlmann neighbourhood selection (2006; method = "mb" of R's huge): one lasso per node on a shared matrix,
// with per-entry penalty weights and the scaled lasso.
//
//     plain  (mode 0):  beta^(j) = argmin_{beta_j = 0} 1/2 beta' S beta - s_j' beta + lambda sum_k w_k |beta_k|      thr_k = lambda w_k
//     scaled (mode 1):  min sqrt(tau^2(beta)) + lambda sum_k w_k |beta_k|                                            thr_k = lambda sigma w_k
//     tau^2(beta) = S_jj - 2 s_j' beta + beta' S beta,  sigma = sqrt(tau^2),  w_k = Wt[j,k] in [0, +inf] (no table: all 1)
//     W_ij = W_ji = the one of beta^(j)_i, beta^(i)_j of smaller ('and') / larger ('or') magnitude      k_mb_symmetrize
//
// k_mb_path: one WAVE per unit of work (matrix m, node j), WPB units per workgroup, the whole descending lambda grid inside
// the kernel, each lambda warm-started from the one before.  Cyclic coordinate descent with covariance updates on an active
// set (glmnet, huge): with g = s_j - S beta held as NV = ceil(p / 64) doubles per lane (element k in lane k % 64, slot k / 64),
//     z = g_k + S_kk beta_k,  b = soft(z, thr_k) / S_kk,  d = b - beta_k,  g -= d S[k, :]   (row k = column k: contiguous)
// beta (8 bytes per variable) and the ascending list of the active set (4 bytes) live in LDS, 12 p bytes per unit; WEIGHTED
// adds the node's weights (ROW j of Wt, one contiguous read; 8 bytes), 20 p bytes per unit: the sweep reads w_k for a
// wave-uniform k (a broadcast read, like beta[k]), the screen reads w lane-distributed.  The waves of a workgroup never meet:
// there is no barrier in the kernel, and every value that steers a loop (the active count, the coordinate, the largest change
// of a sweep, sigma and tau^2 -- read from lane 0) is wave-uniform by construction -- ballots, cross-lane reads of a uniform
// lane.  The row of the NEXT active coordinate is loaded before the current one is applied, so one row latency per
// coordinate is hidden behind the other's arithmetic.  S_kk is element k of the row that is loaded anyway.
//
// Per lambda:  screen (all k != j outside the active set with |g_k| > thr_k join it, found in one step, the list
// rebuilt ascending) -> sweeps over the active set until max |d| S_kk <= tol -> g recomputed from beta in ascending order ->
// ONE further sweep -> screen again; finished only if that sweep moved nothing beyond tol and that screen found nothing.
// Weights (the adaptive lasso of Zou 2006, JASA 101; glmnet's penalty.factor): w_k = 0 is an unpenalised coordinate, it joins
// at the first screen; w_k = +inf excludes one -- |g_k| > inf is never true, so it never joins and its beta_k stays the exact
// zero it was set to.  With unit weights the thresholds are the unweighted ones bit for bit (lambda * 1.0 is exact).
// The scaled lasso (Sun & Zhang 2012, Biometrika 99; the square-root lasso of Belloni, Chernozhukov, Wang 2011, Biometrika
// 98; TIGER, Liu & Wang 2017, EJS 11) is the alternation of Sun & Zhang around that procedure, per (node, lambda):  sigma_t =
// sqrt(tau^2) of the warm start (sqrt(S_jj) at the first lambda) -> the procedure to its finished state at thresholds
// (lambda sigma_t) w_k -> tau^2, sigma_new = sqrt(tau^2) -> finished if |sigma_new - sigma_t| <= sig_tol sigma_new, else
// sigma_t = sigma_new, at most max_outer times.  Plain mode runs the procedure once.
//
// Statuses: 0 finished, 1 a cap was reached (sweeps, screens, outer iterations), 2 a non-finite g or beta, 3 (scaled)
// tau^2 <= 1e-10 S_jj or not positive -- a duplicated variable or a perfect fit, where sigma decays geometrically and the
// relative test can never end the loop.  2 and 3: that node's column is NaN (diagonal 0) at this and every later lambda,
// nobody else is touched.  Nothing can hang: max_outer, max_sweeps and MB_MAX_ROUNDS are trip-count caps and every
// continuing comparison is false for a NaN.
//
// Reproducibility: no atomics, fixed orders (the active list ascending, a lane's slots ascending, the xor butterfly for the one
// wave sum).  A unit reads its own matrix and writes its own rows: its bits do not depend on M, on its neighbours in the
// workgroup, or on the lambdas that follow.
//
// Largest p: MB_MAX_P = 2048 (kernels.hpp) -- 32 slots of g, of the current and of the prefetched row per lane, 24 KiB (40 KiB
// WEIGHTED) of LDS per unit.  The slot count is a template parameter (4, 8, 16, 32: p <= 256, 512, 1024, 2048) of ONE body, so
// that every register array is indexed by constants; units per workgroup 4, at 32 slots 2.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

static constexpr int MB_MAX_ROUNDS = 100;
static constexpr double MB_TAU_FLOOR = 1e-10;

// WEIGHTED and SCALED are template parameters because the resource report says that it pays.  SCALED as a runtime argument:
// the alternation's state (sigma, tau^2, the outer counters) costs the plain body 10 to 16 VGPRs and with them one wave per
// SIMD at 4 and at 8 slots.  WEIGHTED as a template parameter costs the unweighted body nothing: VGPRs at 4 / 8 / 16 / 32
// slots <false,false> 82 / 119 / 217 / 412, <true,false> 84 / 121 / 219 / 416, <true,true> 94 / 133 / 232 / 424, each what the
// two separate kernels had before they became one, and the unweighted units keep 12 p bytes of LDS.
template <int NV, int WPB, bool WEIGHTED, bool SCALED>
__global__ __launch_bounds__(64 * WPB) void k_mb_path(const double* __restrict__ S, int M, int p,
                                                      const double* __restrict__ Wt, size_t wstride,
                                                      const double* __restrict__ lam, int L, double tol, int max_sweeps,
                                                      double sig_tol, int max_outer, double* __restrict__ coef,
                                                      double* __restrict__ resvar, int* __restrict__ info, int ninfo,
                                                      size_t strideM, size_t strideL)
{
    static_assert(WEIGHTED || !SCALED, "the scaled lasso runs on the weighted body");
    extern __shared__ __attribute__((aligned(16))) char mb_smem[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long unit = (long long)blockIdx.x * WPB + w;                 // m-major: the units of one matrix are adjacent
    if (unit >= (long long)M * p) return;                                   // a whole wave; no barrier follows
    const int m = (int)(unit / p), j = (int)(unit % p);
    const size_t pp = (size_t)p * p;
    const double* Sm = S + (size_t)m * pp;
    double* beta = reinterpret_cast<double*>(mb_smem) + (size_t)w * p;
    double* wts = reinterpret_cast<double*>(mb_smem) + (size_t)(WPB + w) * p;                    // WEIGHTED only
    int* act = reinterpret_cast<int*>(reinterpret_cast<double*>(mb_smem) + (size_t)(WEIGHTED ? 2 : 1) * WPB * p) + (size_t)w * p;
    const unsigned long long below = (1ull << lane) - 1ull;

    double g[NV];
    unsigned mem = 0;                                                       // bit v: variable v * 64 + lane is active
    int na = 0;

    auto load_row = [&](int k, double (&r)[NV]) {
        const double* row = Sm + (size_t)k * p;
#pragma unroll
        for (int v = 0; v < NV; ++v) r[v] = (v * 64 + lane < p) ? row[v * 64 + lane] : 0.0;
    };
    // element k of a distributed vector, k wave-uniform
    // (every slot's lane is read first and the slot chosen among the scalars: a choice among the slots themselves the
    // compiler turns into an indexed load, which puts the whole array into scratch)
    auto pick = [&](const double (&a)[NV], int k) -> double {
        const int kv = k >> 6, kl = k & 63;
        double x = lane_read(a[0], kl);
#pragma unroll
        for (int v = 1; v < NV; ++v) {
            const double t = lane_read(a[v], kl);
            x = (kv == v) ? t : x;
        }
        return x;
    };
    auto active_at = [&](int i) -> int { return __builtin_amdgcn_readfirstlane(act[i]); };
    // the threshold of coordinate k at ls = lambda (sigma)
    auto thr = [&](double ls, int k) -> double {
        if constexpr (WEIGHTED) return ls * wts[k];
        else return ls;
    };

    // one pass over the active set, ascending; returns max |d| S_kk (a NaN change is found in g afterwards)
    auto sweep = [&](double ls) -> double {
        double dmax = 0.0, cur[NV], nxt[NV];
        if (na > 0) load_row(active_at(0), cur);
        for (int i = 0; i < na; ++i) {
            const int k = active_at(i);
            load_row(active_at(min(i + 1, na - 1)), nxt);
            const double skk = pick(cur, k), gk = pick(g, k), bk = beta[k];
            const double b = soft(gk + skk * bk, thr(ls, k)) / skk;
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
            const bool viol = idx < p && idx != j && !((mem >> v) & 1u) && fabs(g[v]) > thr(ls, idx < p ? idx : 0);
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
        for (int v = 0; v < NV; ++v) nf |= (v * 64 + lane < p) && not_finite(g[v]);
        for (int i = lane; i < na; i += 64) nf |= not_finite(beta[act[i]]);
        return __ballot(nf) != 0ull;
    };
    // tau^2 = S_jj - s_j' beta - beta' g: a lane adds its active slots in ascending order, then the butterfly
    auto tau2 = [&]() -> double {
        double sj[NV], acc = 0.0;
        load_row(j, sj);
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if ((mem >> v) & 1u) acc += beta[v * 64 + lane] * (sj[v] + g[v]);
        return lane_read(pick(sj, j) - wave_sum(acc), 0);
    };

    const double* wrow = WEIGHTED && Wt ? Wt + (size_t)m * wstride + (size_t)j * p : nullptr;
    for (int i = lane; i < p; i += 64) {
        beta[i] = 0.0;
        if constexpr (WEIGHTED) wts[i] = wrow ? wrow[i] : 1.0;
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
            double sig = SCALED ? lane_read(sqrt(tau), 0) : 1.0;            // (lane 0's: kept in scalar registers)
            for (int it = 0; it < nouter; ++it) {
                const double ls = SCALED ? lane_read(lamv * sig, 0) : lamv;
                int st = 1;
                double d1 = 0.0;
                for (int round = 0; round < MB_MAX_ROUNDS; ++round) {
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
                if (!(tau > MB_TAU_FLOOR * sjj)) { status = 3; break; }
                if (st == 1) break;                                         // a cap of the inner procedure: status 1
                const double sn = lane_read(sqrt(tau), 0);
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
            int* o = info + (unit_out * p + j) * ninfo;
            o[0] = sweeps;
            o[1] = status;
            if (ninfo > 2) o[2] = SCALED ? outer : 0;
        }
    }
}

template <int NV, int WPB, bool WEIGHTED, bool SCALED>
static hipError_t mb_launch(hipStream_t st, const double* S, int M, int p, const double* Wt, size_t wstride, const double* lam,
                            int L, double tol, int max_sweeps, double sig_tol, int max_outer, double* coef, double* resvar,
                            int* info, int ninfo, size_t strideM, size_t strideL)
{
    const long long units = (long long)M * p;
    const size_t lds = (size_t)WPB * p * ((WEIGHTED ? 2 : 1) * sizeof(double) + sizeof(int));
    if (lds > 64 * 1024) {
        // per launch: the attribute belongs to the current device's copy of the kernel
        const hipError_t e = hipFuncSetAttribute((const void*)k_mb_path<NV, WPB, WEIGHTED, SCALED>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_mb_path<NV, WPB, WEIGHTED, SCALED>), dim3((unsigned)((units + WPB - 1) / WPB)), dim3(64 * WPB), lds, st,
                       S, M, p, Wt, wstride, lam, L, tol, max_sweeps, sig_tol, max_outer, coef, resvar, info, ninfo, strideM,
                       strideL);
    return hipGetLastError();
}

// (the caller checked 1 <= p <= MB_MAX_P, M * p < 2^31, mode 0 or 1, max_outer >= 1, ninfo 2 or 3)
hipError_t launch_mb_path(hipStream_t st, const double* S, int M, int p, const double* Wt, size_t wstride, const double* lam, int L,
                          int mode, double tol, int max_sweeps, double sig_tol, int max_outer, double* coef, double* resvar,
                          int* info, int ninfo, size_t strideM, size_t strideL)
{
#define GGL_MB_ARGS st, S, M, p, Wt, wstride, lam, L, tol, max_sweeps, sig_tol, max_outer, coef, resvar, info, ninfo, strideM, strideL
#define GGL_MB(NV, WPB)                                                                       \
    (mode ? mb_launch<NV, WPB, true, true>(GGL_MB_ARGS)                                       \
          : Wt ? mb_launch<NV, WPB, true, false>(GGL_MB_ARGS) : mb_launch<NV, WPB, false, false>(GGL_MB_ARGS))
    if (p <= 256) return GGL_MB(4, 4);
    if (p <= 512) return GGL_MB(8, 4);
    if (p <= 1024) return GGL_MB(16, 4);
    return GGL_MB(32, 2);
#undef GGL_MB
#undef GGL_MB_ARGS
}

// k_mb_path leaves beta^(j) in ROW j (coalesced stores).  In place over the 32 x 32 tile pairs I <= J of every matrix, for
// i < j with a = beta^(j)_i (row j) and b = beta^(i)_j (row i):
//     rule 0 (raw):  (i,j) <- a, (j,i) <- b      the transpose: column j holds beta^(j)
//     rule 1 (and):  both <- |b| < |a| ? b : a    the smaller magnitude, a on a tie (and where one of them is a NaN)
//     rule 2 (or):   both <- |b| > |a| ? b : a    the larger magnitude, a on a tie
// Both tiles are read before the barrier and written behind it, the lower one through LDS so that every store runs along rows.
__global__ __launch_bounds__(256) void k_mb_symmetrize(double* __restrict__ C, int p, int rule)
{
    __shared__ double lo[32][33], outl[32][33];
    const int nT = (p + 31) / 32;
    int b = blockIdx.x, I = 0;
    while (b >= nT - I) { b -= nT - I; ++I; }
    const int J = I + b;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double* R = C + (size_t)blockIdx.y * p * p;
    double u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = ty + 8 * q;
        const int gi = I * 32 + r, gj = J * 32 + tx, li = J * 32 + r, lj = I * 32 + tx;
        u[q] = (gi < p && gj < p) ? R[(size_t)gi * p + gj] : 0.0;
        lo[r][tx] = (li < p && lj < p) ? R[(size_t)li * p + lj] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = ty + 8 * q;
        const int gi = I * 32 + r, gj = J * 32 + tx;
        const double a = lo[tx][r], bb = u[q];
        double ou, ol;
        if (rule == 0) {
            ou = a;
            ol = bb;
        } else {
            const bool take_b = rule == 1 ? fabs(bb) < fabs(a) : fabs(bb) > fabs(a);
            ou = ol = take_b ? bb : a;
        }
        if (gi < p && gj < p && gi < gj) R[(size_t)gi * p + gj] = ou;
        outl[r][tx] = ol;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = ty + 8 * q;
        const int mi = J * 32 + r, mj = I * 32 + tx;
        if (mi < p && mj < p && mi > mj) R[(size_t)mi * p + mj] = outl[tx][r];
    }
}

void launch_mb_symmetrize(hipStream_t st, double* C, size_t nmat, int p, int rule)
{
    const int nT = (p + 31) / 32;
    for (size_t z0 = 0; z0 < nmat; z0 += 65535) {
        const unsigned nz = (unsigned)std::min<size_t>(65535, nmat - z0);
        hipLaunchKernelGGL(k_mb_symmetrize, dim3(nT * (nT + 1) / 2, nz), dim3(256), 0, st, C + z0 * (size_t)p * p, p, rule);
    }
}

}  // namespace ggl
