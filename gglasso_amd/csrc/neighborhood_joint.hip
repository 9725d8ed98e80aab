// Joint neighbourhood selection for K instances that share structure: the regression counterpart of the GGL
// penalty (Chiquet, Grandvalet, Ambroise 2011; Danaher, Wang, Witten 2014).  For node j, with B = (beta^(1), ..., beta^(K)):
//
//     min_B  sum_k omega_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ]
//            + lambda1 sum_k sum_{i != j} |beta^(k)_i|  +  lambda2 sum_{i != j} || (beta^(1)_i, ..., beta^(K)_i) ||_2
//
// k_mb_joint_path: one WORKGROUP per unit of work (chain c, node j), W = min(K, 8) waves; wave w owns the instances
// k = w, w + W, ... (at most IPW of them).  A chain is a list of L penalty pairs walked in order with warm starts.  Block
// coordinate descent on an active set of GROUPS (one block = the K coefficients of one variable i; Simon, Friedman, Hastie,
// Tibshirani 2013): with g^(k) = omega_k (s_j^(k) - S^(k) beta^(k)), a_k = omega_k S^(k)_ii, z_k = g^(k)_i + a_k beta^(k)_i,
// u = soft(z, lambda1):
//     ||u|| <= lambda2: b = 0;   lambda2 = 0: b_k = u_k / a_k;   else b_k = u_k nu / (a_k nu + lambda2),
//     nu = ||b|| the root of phi(nu) = sum_k u_k^2 / (a_k nu + lambda2)^2 - 1 -- Newton from nu_0 = (||u|| - lambda2) / max a_k,
//     where phi >= 0: the iterates increase to the root and the loop ends when a step no longer increases nu (or at the cap);
//     g^(k) -= omega_k (b_k - beta^(k)_i) S^(k)[i, :].
//
// Where things live.  g^(k) of an owned instance: NV = ceil(p / 64) doubles per lane (element i in lane i % 64, slot i / 64),
// as k_mb_path keeps its g; NV and IPW are template parameters so that every register array is indexed by constants.  Where
// K p is too large for the registers of one workgroup (GMEM) the same vectors live in a workspace in device memory with the
// same distribution, every element touched by one lane of one wave only.  beta:
// in the OUTPUT row the unit writes anyway (row j of matrix (c, l, k) of coef) -- it is touched one element per instance and
// block update, and K p doubles fit neither the registers beside g nor, at K = 32, p = 500, the LDS beside anything else.  At
// the start of a pair the row of the pair before is copied forward.  LDS: the ascending active list, the exchange of
// (z_k, a_k, beta_k) of one block update (double-buffered: one workgroup barrier per update) and the per-wave partial sums
// of the screen.
//
// A block update: every wave writes (z, a, beta) of its instances; ONE barrier; every wave solves the block redundantly with
// instance k in lane k -- the norms go through the fixed xor butterfly, so all lanes of all waves hold the same bits; each
// wave applies d_k to its own gradients.  The first owned row is requested before the barrier.  Every value that steers a loop
// (the active count, the variable, the largest change, the Newton trip count, the statuses) is computed by every wave from
// the same LDS words and is therefore workgroup-uniform: all waves reach all barriers.
//
// Per pair, the procedure of k_mb_path: screen (every inactive group with ||soft(g_i, lambda1)|| > lambda2 joins,
// the list is rebuilt ascending) -> sweeps until max_k |d_k| a_k <= tol -> all gradients recomputed from B in ascending
// order -> ONE further sweep -> screen again; finished only if that sweep moved nothing beyond tol and that screen found
// nothing.  Caps: max_sweeps per (unit, pair), MBJ_MAX_ROUNDS screens, MBJ_NEWTON_CAP Newton steps; every continuing
// comparison is false for a NaN.  A non-finite value is status 2: all K rows of the unit are NaN (diagonal 0) at this pair
// and every later one of the chain; nobody else is touched.
//
// Reproducibility: no atomic updates, fixed orders (the list ascending, a wave's instances ascending, the screen's sum over waves
// ascending, the butterfly).  A unit reads S and its own rows only: its bits do not depend on C, on the other chains or on the
// pairs that follow.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

static constexpr int MBJ_MAX_ROUNDS = 100;
static constexpr int MBJ_NEWTON_CAP = 64;
static constexpr int MBJ_MAX_WAVES = 8;

__device__ __forceinline__ double mbj_lane_read(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ bool mbj_not_finite(double x) { return !(fabs(x) <= 1.79769313486231570815e308); }

template <int NV, int IPW, bool GMEM>
__global__ __launch_bounds__(64 * MBJ_MAX_WAVES) void k_mb_joint_path(const double* __restrict__ S, int K, int p,
                                                                      const double* __restrict__ omega,
                                                                      const double* __restrict__ lam1,
                                                                      const double* __restrict__ lam2, int L, double tol,
                                                                      int max_sweeps, double* coef, double* __restrict__ resvar,
                                                                      int* __restrict__ info, double* gws)
{
    __shared__ double xch[2][3][64];                                        // (z, a, beta) of a block update, instance k at [k]
    __shared__ double part[2][MBJ_MAX_WAVES][64];                           // the screen's partial sums of squares, per wave
    __shared__ int act[MBJ_MAX_P];
    __shared__ double oms[64];                                              // omega_k (uniform values read where they are used)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), W = (int)(blockDim.x >> 6);
    const int c = (int)(blockIdx.x / (unsigned)p), j = (int)(blockIdx.x % (unsigned)p);
    const size_t pp = (size_t)p * p;
    const bool in = lane < K;
    constexpr int QU = GMEM ? 1 : IPW;                                      // GMEM: the loops over a wave's instances stay rolled

    double g[GMEM ? 1 : IPW][GMEM ? 1 : NV];                                // (GMEM: the gradients live in gws, below)
    unsigned mem = 0;                                                       // bit v: group v * 64 + lane is active
    int na = 0, parity = 0;
    bool nfb = false;                                                       // a block's solution was not finite

    auto load_row = [&](int k, int i, double (&r)[NV]) {
        const double* row = S + (size_t)k * pp + (size_t)i * p;
#pragma unroll
        for (int v = 0; v < NV; ++v) r[v] = (v * 64 + lane < p) ? row[v * 64 + lane] : 0.0;
    };
    // element i of a distributed vector, i wave-uniform: every slot's lane is read and the choice made among the scalars
    // (k_mb_path's pick: a choice among the slots themselves becomes an indexed load and puts the array into scratch)
    auto pick = [&](const double (&a)[NV], int i) -> double {
        const int iv = i >> 6, il = i & 63;
        double x = mbj_lane_read(a[0], il);
#pragma unroll
        for (int v = 1; v < NV; ++v) {
            const double t = mbj_lane_read(a[v], il);
            x = (iv == v) ? t : x;
        }
        return x;
    };
    // Where the K gradients do not fit the registers (GMEM) they live in the workspace gws, (unit, k, p): the same
    // distribution, element idx of instance k touched by lane idx % 64 of the wave that owns k and by nobody else, so a lane
    // only ever reads what it wrote itself.  gload / gstore move one instance's vector, gelem one slot, gpick one element.
    auto gws_row = [&](int k) -> double* { return gws + ((size_t)blockIdx.x * K + k) * p; };
    auto gload = [&](int q, int k, double (&r)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if constexpr (GMEM) r[v] = (v * 64 + lane < p) ? gws_row(k)[v * 64 + lane] : 0.0;
            else r[v] = g[q][v];
        }
    };
    auto gstore = [&](int q, int k, const double (&r)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if constexpr (GMEM) { if (v * 64 + lane < p) gws_row(k)[v * 64 + lane] = r[v]; }
            else g[q][v] = r[v];
        }
    };
    auto gelem = [&](int q, int k, int v) -> double {                       // (0 for an instance not owned, a slot beyond p)
        if constexpr (GMEM) return (k < K && v * 64 + lane < p) ? gws_row(k)[v * 64 + lane] : 0.0;
        else return g[q][v];
    };
    auto gpick = [&](int q, int k, int i) -> double {
        if constexpr (GMEM) {
            const int idx = (i & ~63) + lane;
            const double t = idx < p ? gws_row(k)[idx] : 0.0;
            return mbj_lane_read(t, i & 63);
        } else {
            return pick(g[q], i);
        }
    };
    auto active_at = [&](int t) -> int { return __builtin_amdgcn_readfirstlane(act[t]); };
    // The working B.  INVARIANT: the rows of instance k (of this unit) are read and written by ONE wave only, the one that owns
    // k (k = w mod W), for the whole kernel; no other wave, workgroup or kernel touches them before the kernel ends.  Inside
    // that wave an element is written either by every lane with the same value (beta_put) or by the lane idx % 64 (the row
    // copied forward, behind a workgroup fence) and read either from one address by every lane (beta_at) or by the lane
    // idx % 64.  All of these are relaxed atomics of workgroup scope, so no access is formally a race; what orders them is the
    // wave's program order on one compute unit's L1.  beta_at is thereby a vector load, never the scalar cache, which does
    // not see the wave's own stores.
    auto beta_row = [&](int l, int k) -> double* { return coef + (((size_t)c * L + l) * K + k) * pp + (size_t)j * p; };
    auto beta_at = [&](int l, int k, int i) -> double {
        return __hip_atomic_load(beta_row(l, k) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto beta_put = [&](int l, int k, int i, double b) {
        __hip_atomic_store(beta_row(l, k) + i, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };

    // one pass over the active groups, ascending; returns max over blocks and instances of |d_k| a_k
    auto sweep = [&](int l, double l1, double l2, int& newton) -> double {
        double dmax = 0.0;
        for (int t = 0; t < na; ++t) {
            const int i = active_at(t), buf = parity;
            parity ^= 1;
            double row[NV];
            load_row(w, i, row);                                            // wave w always owns instance w
#pragma unroll QU
            for (int q = 0; q < IPW; ++q) {
                const int k = w + q * W;
                if (k < K) {
                    const double a = oms[k] * S[(size_t)k * pp + (size_t)i * p + i], bo = beta_at(l, k, i);
                    const double z = gpick(q, k, i) + a * bo;
                    if (lane == 0) {
                        xch[buf][0][k] = z;
                        xch[buf][1][k] = a;
                        xch[buf][2][k] = bo;
                    }
                }
            }
            __syncthreads();
            // instance k in lane k; a lane beyond K holds u = 0, a = 0 and adds nothing to a sum
            const double z = in ? xch[buf][0][lane] : 0.0, a = in ? xch[buf][1][lane] : 0.0, bold = in ? xch[buf][2][lane] : 0.0;
            const double u = soft(z, l1), un = sqrt(wave_sum(u * u));
            double b = 0.0;
            if (un > l2) {
                if (l2 == 0.0) {
                    b = in ? u / a : 0.0;
                } else {
                    double nu = (un - l2) / wave_max(a);
                    int it = 0;
                    for (; it < MBJ_NEWTON_CAP; ++it) {
                        const double tt = 1.0 / (a * nu + l2), ut = u * tt;
                        const double f = wave_sum(ut * ut) - 1.0, fp = -2.0 * wave_sum(ut * ut * a * tt);
                        const double nn = nu - f / fp;
                        if (!(nn > nu)) break;
                        nu = nn;
                    }
                    newton = it > newton ? it : newton;
                    b = u * nu / (a * nu + l2);
                }
            }
            nfb = nfb || __ballot(in && mbj_not_finite(b)) != 0ull;
            const double cm = wave_max(in ? fabs(b - bold) * a : 0.0);
            dmax = cm > dmax ? cm : dmax;
#pragma unroll QU
            for (int q = 0; q < IPW; ++q) {
                const int k = w + q * W;
                if (k < K) {
                    if (q > 0) load_row(k, i, row);
                    const double bn = mbj_lane_read(b, k), d = bn - xch[buf][2][k];
                    if (d != 0.0) {
                        const double wd = oms[k] * d;
                        double gq[NV];
                        gload(q, k, gq);
#pragma unroll
                        for (int v = 0; v < NV; ++v) gq[v] -= wd * row[v];
                        gstore(q, k, gq);
                        beta_put(l, k, i, bn);                              // every lane the same value: a lane reads its own
                    }
                }
            }
        }
        return dmax;
    };
    // every violating group joins; the list is rebuilt in ascending order.  The sum of squares of a variable over the
    // instances: a wave's own in ascending k, then the waves in ascending order -- the same in every wave.
    auto screen = [&](double l1, double l2) -> int {
        int added = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double s = 0.0;
#pragma unroll QU
            for (int q = 0; q < IPW; ++q) {                                 // (the g of an instance not owned stays 0)
                const double t = soft(gelem(q, w + q * W, v), l1);
                s += t * t;
            }
            part[v & 1][w][lane] = s;
            __syncthreads();
            double n2 = 0.0;
            for (int ww = 0; ww < W; ++ww) n2 += part[v & 1][ww][lane];
            const int idx = v * 64 + lane;
            const bool viol = idx < p && idx != j && !((mem >> v) & 1u) && sqrt(n2) > l2;
            if (viol) mem |= 1u << v;
            added += __popcll(__ballot(viol));
        }
        if (added) {
            const unsigned long long below = (1ull << lane) - 1ull;
            int base = 0;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const bool isin = (mem >> v) & 1u;
                const unsigned long long bal = __ballot(isin);
                if (isin && w == 0) act[base + __popcll(bal & below)] = v * 64 + lane;
                base += __popcll(bal);
            }
            na = base;
        }
        __syncthreads();
        return added;
    };
    // g^(k) = omega_k s_j - sum over the active groups, ascending, of omega_k beta_i S[i, :]
    auto recompute = [&](int l) {
#pragma unroll QU
        for (int q = 0; q < IPW; ++q) {
            const int k = w + q * W;
            if (k < K) {
                double row[NV], gq[NV];
                load_row(k, j, row);
#pragma unroll
                for (int v = 0; v < NV; ++v) gq[v] = oms[k] * row[v];
                for (int t = 0; t < na; ++t) {
                    const int i = active_at(t);
                    const double bi = beta_at(l, k, i);
                    if (bi != 0.0) {
                        load_row(k, i, row);
                        const double wb = oms[k] * bi;
#pragma unroll
                        for (int v = 0; v < NV; ++v) gq[v] -= wb * row[v];
                    }
                }
                gstore(q, k, gq);
            }
        }
    };
    auto bad = [&]() -> bool {
        bool nf = nfb;
#pragma unroll QU
        for (int q = 0; q < IPW; ++q)
#pragma unroll
            for (int v = 0; v < NV; ++v) nf |= mbj_not_finite(gelem(q, w + q * W, v));    // (slots beyond p and instances not owned hold 0)
        return __syncthreads_or(nf ? 1 : 0) != 0;
    };

#pragma unroll QU
    for (int q = 0; q < IPW; ++q) {
        const int k = w + q * W;
        if constexpr (!GMEM) {
#pragma unroll
            for (int v = 0; v < NV; ++v) g[q][v] = 0.0;
        }
        if (k < K) {
            const double omk = omega ? omega[k] : 1.0;
            double row[NV];
            load_row(k, j, row);
#pragma unroll
            for (int v = 0; v < NV; ++v) row[v] *= omk;
            gstore(q, k, row);
        }
    }
    if (threadIdx.x < 64) oms[lane] = (in && omega) ? omega[lane] : 1.0;
    __syncthreads();
    bool dead = false;

    for (int l = 0; l < L; ++l) {
        const double l1 = lam1[(size_t)c * L + l], l2 = lam2[(size_t)c * L + l];
        int sweeps = 0, status = 1, newton = 0;
        if (!dead) {
            // the working B of this pair: the rows of the pair before (zeros at the first), in place in the output
#pragma unroll QU
            for (int q = 0; q < IPW; ++q) {
                const int k = w + q * W;
                if (k < K) {
                    const double* Bp = beta_row(l > 0 ? l - 1 : 0, k);
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const int idx = v * 64 + lane;
                        if (idx < p) beta_put(l, k, idx, l > 0 ? Bp[idx] : 0.0);
                    }
                }
            }
            __threadfence_block();                                          // a lane's element is read by the whole wave below
        }
        if (dead) {
            status = 2;
        } else if (bad()) {
            status = 2;
        } else {
            double d1 = 0.0;
            for (int round = 0; round < MBJ_MAX_ROUNDS; ++round) {
                const int nviol = screen(l1, l2);
                if (nviol == 0 && (round > 0 ? !(d1 > tol) : na == 0)) { status = 0; break; }
                bool conv = false;
                while (sweeps < max_sweeps) {
                    const double dm = sweep(l, l1, l2, newton);
                    ++sweeps;
                    if (!(dm > tol)) { conv = true; break; }
                }
                if (!conv) break;                                           // max_sweeps reached
                recompute(l);
                if (sweeps >= max_sweeps) break;
                d1 = sweep(l, l1, l2, newton);
                ++sweeps;
                if (bad()) { status = 2; break; }
            }
            if (status == 1 && bad()) status = 2;
        }
        dead = status == 2;

#pragma unroll QU
        for (int q = 0; q < IPW; ++q) {
            const int k = w + q * W;
            if (k < K) {
                double* B = beta_row(l, k);
                if (dead) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const int idx = v * 64 + lane;
                        if (idx < p) B[idx] = idx == j ? 0.0 : __builtin_nan("");
                    }
                }
                if (resvar) {
                    // tau^2 = S_jj - sum over the active groups of beta_i (s_ji + g_i / omega): a lane adds its slots in
                    // ascending order, then the butterfly
                    double sj[NV], acc = 0.0;
                    load_row(k, j, sj);
                    if (!dead) {
#pragma unroll
                        for (int v = 0; v < NV; ++v)
                            if ((mem >> v) & 1u) acc += B[v * 64 + lane] * (sj[v] + gelem(q, k, v) / oms[k]);
                    }
                    const double tau = pick(sj, j) - wave_sum(acc);
                    if (lane == 0) resvar[(((size_t)c * L + l) * K + k) * p + j] = dead ? __builtin_nan("") : tau;
                }
            }
        }
        if (w == 0 && lane == 0) {
            int* o = info + (((size_t)c * L + l) * p + j) * 3;
            o[0] = sweeps;
            o[1] = status;
            o[2] = newton;
        }
    }
}

// The g of a workgroup's K regressions lives in its registers where it fits: 8 waves of 256 registers hold 48 slots of 64
// doubles each beside everything else, and a wave needs ceil(K / 8) (rounded up to 1, 2, 4, 8) times ceil(p / 64) (4, 6, 8,
// 16) of them -- K <= 64 up to p = 384, K <= 32 up to p = 512, K <= 16 up to p = 1024.  Beyond that the same body runs with g
// in a workspace in device memory (GMEM), K p doubles per unit.
static bool mbj_in_registers(int K, int p) { return K <= (p <= 384 ? 64 : (p <= 512 ? 32 : 16)); }

bool mb_joint_supported(int K, int p) { return K >= 1 && p >= 1 && K <= MBJ_MAX_K && p <= MBJ_MAX_P; }

size_t mb_joint_workspace(int K, int p) { return mbj_in_registers(K, p) ? 0 : (size_t)K * p; }

template <int NV, int IPW, bool GMEM>
static void mbj_launch(hipStream_t st, const double* S, int K, int p, const double* omega, const double* lam1, const double* lam2,
                       int C, int L, double tol, int max_sweeps, double* coef, double* resvar, int* info, double* gws)
{
    const int W = std::min(K, MBJ_MAX_WAVES);
    hipLaunchKernelGGL((k_mb_joint_path<NV, IPW, GMEM>), dim3((unsigned)C * (unsigned)p), dim3(64 * W), 0, st, S, K, p, omega, lam1,
                       lam2, L, tol, max_sweeps, coef, resvar, info, gws);
}

// (the caller checked mb_joint_supported(K, p) and C * p < 2^31; gws: C * p * mb_joint_workspace(K, p) doubles)
void launch_mb_joint_path(hipStream_t st, const double* S, int K, int p, const double* omega, const double* lam1,
                          const double* lam2, int C, int L, double tol, int max_sweeps, double* coef, double* resvar, int* info,
                          double* gws)
{
    const int W = std::min(K, MBJ_MAX_WAVES), ipw = (K + W - 1) / W;
#define MBJ_GO(NV, IPW, GM) mbj_launch<NV, IPW, GM>(st, S, K, p, omega, lam1, lam2, C, L, tol, max_sweeps, coef, resvar, info, gws)
    if (!mbj_in_registers(K, p)) {
        if (p <= 512) MBJ_GO(8, 8, true); else MBJ_GO(16, 8, true);
    } else if (p <= 256) {
        if (ipw == 1) MBJ_GO(4, 1, false); else if (ipw == 2) MBJ_GO(4, 2, false); else if (ipw <= 4) MBJ_GO(4, 4, false); else MBJ_GO(4, 8, false);
    } else if (p <= 384 && ipw > 4) {
        MBJ_GO(6, 8, false);
    } else if (p <= 512) {
        if (ipw == 1) MBJ_GO(8, 1, false); else if (ipw == 2) MBJ_GO(8, 2, false); else MBJ_GO(8, 4, false);
    } else {
        if (ipw == 1) MBJ_GO(16, 1, false); else MBJ_GO(16, 2, false);
    }
#undef MBJ_GO
}

}  // namespace ggl
