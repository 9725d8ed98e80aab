// The body that k_mb_joint_path (neighborhood_joint.hip) and k_mb_fused_path (neighborhood_fused.hip)
// share: one workgroup per (chain, node), block coordinate descent over an active set of blocks, one block being the K
// coefficients of one variable.  Everything but the penalty is common -- where g, beta and the active list live, the
// exchange of a block through LDS behind one barrier, the per-pair procedure, the caps and the statuses; each file's head
// describes it.  FUSED chooses the penalty across the instances: the group norm (false: the Newton root of DESIGN 30) or the
// total variation along k (true: Condat's scan, and the dual feasibility scan as the screen).  An `if constexpr` selects, so
// neither penalty carries the other's code, registers or LDS.
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

static constexpr int MBJ_MAX_ROUNDS = 100;
static constexpr int MBJ_NEWTON_CAP = 64;
static constexpr int MBJ_MAX_WAVES = 8;

// Condat's direct 1-D total-variation prox of y_0 .. y_{N-1}, y_k held by lane k, 2 <= N <= 64: the arithmetic and the order
// of condat_inplace (theta_pair.hip), one decision of the scan per trip as in condat_uniform.  Every lane runs the whole
// scan: an element is read from its lane into a scalar (k is wave-uniform), a closed segment [a, b] is written by the lanes
// a..b, so every steering value is wave-uniform and, the inputs being the same LDS words in every wave, workgroup-uniform.
// Returns x_k in lane k (lanes >= N: their y).
//
// Trip count.  A trip either extends the segment (k += 1, k <= N - 1) or closes one, and a close sets k0 to kminus + 1 or
// kplus + 1 or ends the scan.  The scan keeps k0 <= kminus and k0 <= kplus at every close (Condat 2013: the points where the
// two bounds last touched lie inside the current segment; tests/mbf_ref.py asserts it at every close of its own scan), so a
// close raises k0; at most N - 1 closes do, and between two of them k runs from the new k0 to at most N - 1: N - 1 - k0
// extensions.  With k0 = 0, 1, ..., N - 1 that is at most N (N - 1) / 2 extensions, N - 1 closes and the final trip:
// N (N + 1) / 2 trips, the cap below (2080 at N = 64).  A scan that reached the cap all the same returns NaN -- status 2 for
// its unit, never a silent wrong block.  Every comparison that closes a segment is false for a NaN, so with a NaN the scan
// extends to k = N - 1 and ends there.
__device__ __forceinline__ double mbf_condat(const double y, const int N, const double lam, const int lane)
{
    auto at = [&](int k) -> double { return lane_read(y, k); };
    double x = y;
    auto fill = [&](int a, int b, double v) { x = (lane >= a && lane <= b) ? v : x; };
    int k = 0, k0 = 0, kplus = 0, kminus = 0;
    const double y0 = at(0);
    double vmin = y0 - lam, vmax = y0 + lam, umin = lam, umax = -lam;
    const int cap = N * (N + 1) / 2;
    bool done = false;
    for (int trip = 0; trip < cap && !done; ++trip) {
        if (k == N - 1) {
            if (umin < 0.0) {
                fill(k0, kminus, vmin);
                kminus += 1;
                k = k0 = kminus;
                umin = lam;
                vmin = at(k);
                umax = vmin + lam - vmax;
                if (k == N - 1) { fill(k, k, vmin + umin); done = true; }
            } else if (umax > 0.0) {
                fill(k0, kplus, vmax);
                kplus += 1;
                k = k0 = kplus;
                umax = -lam;
                vmax = at(k);
                umin = vmax - lam - vmin;
                if (k == N - 1) { fill(k, k, vmin + umin); done = true; }
            } else {
                fill(k0, N - 1, vmin + umin / (double)(k - k0 + 1));
                done = true;
            }
        } else {
            const double yn = at(k + 1);
            if (yn + umin - vmin < -lam) {
                fill(k0, kminus, vmin);
                kminus += 1;
                k = kplus = k0 = kminus;
                vmin = at(k);
                vmax = vmin + 2 * lam;
                umin = lam;
                umax = -lam;
            } else if (yn + umax - vmax > lam) {
                fill(k0, kplus, vmax);
                kplus += 1;
                k = kminus = k0 = kplus;
                vmax = at(k);
                vmin = vmax - 2 * lam;
                umin = lam;
                umax = -lam;
            } else {
                k += 1;
                umin = umin + yn - vmin;
                umax = umax + yn - vmax;
                if (umin >= lam) {
                    vmin += (umin - lam) / (double)(k - k0 + 1);
                    umin = lam;
                    kminus = k;
                }
                if (umax <= -lam) {
                    vmax += (umax + lam) / (double)(k - k0 + 1);
                    umax = -lam;
                    kplus = k;
                }
            }
        }
    }
    return done ? x : __builtin_nan("");
}

// (FUSED: the launch passes K * 64 doubles of dynamic LDS, the screen's exchange)
template <int NV, int IPW, bool GMEM, bool FUSED>
__device__ __forceinline__ void mb_joint_body(const double* __restrict__ S, int K, int p, const double* __restrict__ omega,
                                              const double* __restrict__ lam1, const double* __restrict__ lam2, int L, double tol,
                                              int max_sweeps, double* coef, double* __restrict__ resvar, int* __restrict__ info,
                                              double* gws)
{
    __shared__ double xch[2][3][64];                                        // (z, a, beta) of a block update, instance k at [k]
    __shared__ double part[FUSED ? 1 : 2][FUSED ? 1 : MBJ_MAX_WAVES][64];   // the group screen's partial sums of squares, per wave
    extern __shared__ double gx[];                                          // FUSED: the screen's g of one slot, [k][lane]
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
        double x = lane_read(a[0], il);
#pragma unroll
        for (int v = 1; v < NV; ++v) {
            const double t = lane_read(a[v], il);
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
            return lane_read(t, i & 63);
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
            double a, bold, b = 0.0;
            if constexpr (FUSED) {
                // ONE curvature for the block, a_i = max_k omega_k S^(k)_ii: every wave gathers the K diagonals (instance k in
                // lane k) and holds the same bits, as a scalar.  v_k = beta_k + g_k / a_i goes through the exchange; behind
                // the barrier every wave runs the scan on the same K words.
                const double ai =
                    lane_read(wave_max(in ? oms[lane] * S[(size_t)lane * pp + (size_t)i * p + i] : 0.0), 0);
#pragma unroll QU
                for (int q = 0; q < IPW; ++q) {
                    const int k = w + q * W;
                    if (k < K) {
                        const double bo = beta_at(l, k, i), vk = bo + gpick(q, k, i) / ai;
                        if (lane == 0) {
                            xch[buf][0][k] = vk;
                            xch[buf][2][k] = bo;
                        }
                    }
                }
                __syncthreads();
                const double v = in ? xch[buf][0][lane] : 0.0;
                a = ai;
                bold = in ? xch[buf][2][lane] : 0.0;
                const double x = (l2 == 0.0 || K == 1) ? v : mbf_condat(v, K, l2 / ai, lane);    // (K = 1: lambda2 is inert)
                nfb = nfb || __ballot(in && not_finite(x)) != 0ull;        // (soft turns a NaN into 0: it is caught here)
                b = in ? soft(x, l1 / ai) : 0.0;
            } else {
#pragma unroll QU
                for (int q = 0; q < IPW; ++q) {
                    const int k = w + q * W;
                    if (k < K) {
                        const double ak = oms[k] * S[(size_t)k * pp + (size_t)i * p + i], bo = beta_at(l, k, i);
                        const double z = gpick(q, k, i) + ak * bo;
                        if (lane == 0) {
                            xch[buf][0][k] = z;
                            xch[buf][1][k] = ak;
                            xch[buf][2][k] = bo;
                        }
                    }
                }
                __syncthreads();
                // instance k in lane k; a lane beyond K holds u = 0, a = 0 and adds nothing to a sum
                const double z = in ? xch[buf][0][lane] : 0.0;
                a = in ? xch[buf][1][lane] : 0.0;
                bold = in ? xch[buf][2][lane] : 0.0;
                const double u = soft(z, l1), un = sqrt(wave_sum(u * u));
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
            }
            nfb = nfb || __ballot(in && not_finite(b)) != 0ull;
            const double cm = wave_max(in ? fabs(b - bold) * a : 0.0);
            dmax = cm > dmax ? cm : dmax;
#pragma unroll QU
            for (int q = 0; q < IPW; ++q) {
                const int k = w + q * W;
                if (k < K) {
                    if (q > 0) load_row(k, i, row);
                    const double bn = lane_read(b, k), d = bn - xch[buf][2][k];
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
            bool out;                                                       // the zero block is not optimal for variable v * 64 + lane
            if constexpr (FUSED) {
                // soft(tv(g_i, lambda2), lambda1) = 0 exactly if 0 solves the fused-lasso prox of g_i, that is if there are
                // t_1 .. t_{K-1} in [-lambda2, lambda2], t_0 = t_K = 0, with |g_k - (t_k - t_{k-1})| <= lambda1 for every k.
                // The set of admissible t_k is an interval: [lo, hi] <- ([lo, hi] + g_k + [-lambda1, lambda1]) cut to
                // [-lambda2, lambda2], and at k = K it must contain 0.  The K gradients of the slot's 64 variables meet in
                // LDS ([k][lane], written by the owner of k); every wave walks them in ascending k for its lane's variable --
                // K fixed trips, no branch, the same bits in every wave.  A NaN fails a comparison and the variable joins.
#pragma unroll QU
                for (int q = 0; q < IPW; ++q) {
                    const int k = w + q * W;
                    if (k < K) gx[k * 64 + lane] = gelem(q, k, v);
                }
                __syncthreads();
                double lo = 0.0, hi = 0.0;
                bool ok = true;
                for (int k = 0; k < K - 1; ++k) {
                    const double gk = gx[k * 64 + lane];
                    lo = lo + gk - l1;
                    hi = hi + gk + l1;
                    lo = lo < -l2 ? -l2 : lo;
                    hi = hi > l2 ? l2 : hi;
                    ok = ok && lo <= hi;
                }
                const double gl = gx[(K - 1) * 64 + lane];
                out = !(ok && lo + gl - l1 <= 0.0 && hi + gl + l1 >= 0.0);
                __syncthreads();                                            // (the next slot overwrites gx)
            } else {
                double s = 0.0;
#pragma unroll QU
                for (int q = 0; q < IPW; ++q) {                             // (the g of an instance not owned stays 0)
                    const double t = soft(gelem(q, w + q * W, v), l1);
                    s += t * t;
                }
                part[v & 1][w][lane] = s;
                __syncthreads();
                double n2 = 0.0;
                for (int ww = 0; ww < W; ++ww) n2 += part[v & 1][ww][lane];
                out = sqrt(n2) > l2;
            }
            const int idx = v * 64 + lane;
            const bool viol = idx < p && idx != j && !((mem >> v) & 1u) && out;
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
            for (int v = 0; v < NV; ++v) nf |= not_finite(gelem(q, w + q * W, v));    // (slots beyond p and instances not owned hold 0)
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

// The variant of the body for (K, p): NV = ceil(p / 64) rounded up to 4, 6, 8, 16 slots per lane, IPW = ceil(K / W) rounded up
// to 1, 2, 4, 8 instances per wave; `in_registers` false: the memory-resident body (GMEM).  go(NV, IPW, GMEM) receives them as
// integral constants.  WIDE2: whether NV = 16 with IPW = 2 exists (a penalty whose body spills there routes K > 8 above p = 512
// to the memory-resident body and never instantiates it).
template <int N> using mbj_int = std::integral_constant<int, N>;
template <bool WIDE2, class Go>
static void mbj_dispatch(int K, int p, bool in_registers, Go go)
{
    const int W = std::min(K, MBJ_MAX_WAVES), ipw = (K + W - 1) / W;
    const std::false_type reg;
    const std::true_type gmem;
    if (!in_registers) {
        if (p <= 512) go(mbj_int<8>{}, mbj_int<8>{}, gmem); else go(mbj_int<16>{}, mbj_int<8>{}, gmem);
    } else if (p <= 256) {
        if (ipw == 1) go(mbj_int<4>{}, mbj_int<1>{}, reg); else if (ipw == 2) go(mbj_int<4>{}, mbj_int<2>{}, reg);
        else if (ipw <= 4) go(mbj_int<4>{}, mbj_int<4>{}, reg); else go(mbj_int<4>{}, mbj_int<8>{}, reg);
    } else if (p <= 384 && ipw > 4) {
        go(mbj_int<6>{}, mbj_int<8>{}, reg);
    } else if (p <= 512) {
        if (ipw == 1) go(mbj_int<8>{}, mbj_int<1>{}, reg); else if (ipw == 2) go(mbj_int<8>{}, mbj_int<2>{}, reg);
        else go(mbj_int<8>{}, mbj_int<4>{}, reg);
    } else {
        if constexpr (WIDE2) {
            if (ipw == 1) go(mbj_int<16>{}, mbj_int<1>{}, reg); else go(mbj_int<16>{}, mbj_int<2>{}, reg);
        } else {
            go(mbj_int<16>{}, mbj_int<1>{}, reg);                           // (in_registers implied K <= 8)
        }
    }
}

}  // namespace ggl
