// Refit of neighbourhood selection on its graph: with the graph held fixed, every node is regressed on its
// neighbours by ordinary least squares -- the relaxed lasso (Meinshausen 2007), the regression-based precision estimator of
// Yuan (2010) and Zhou, Ruetimann, Xu, Buehlmann (2011).
//
// A unit of work is (slot s, node j); slot s is a (p,p) matrix of the stack W and reads matrix (s / sdiv) % smod of S (and T).
//     A      = { i != j : |W[s,j,i]| >= t }              row j; a NaN is no edge; ascending
//     beta   = S_AA^-1 s_A,  s_A = S[A, j]                Cholesky S_AA = L L', L y = s_A, L' beta = y
//     tau^2  = q(S; beta),  r = q(T; beta)                q(M; b) = M_jj - 2 m_A' b + b' M_AA b, one function for both
// d = |A| = 0 leaves beta = 0, tau^2 = S_jj, r = T_jj through the same code (every loop is empty).
//
// k_mb_refit<NT, UPB, CAP>: NT threads per unit, UPB units per workgroup, degrees up to CAP.  Two instantiations:
//     <64, 4, 32>    a WAVE per unit, no barrier in the kernel, 4.6 KiB of LDS per unit: every unit of the stack goes through
//                    it; a unit with CAP < d <= MBR_MAX_DEG leaves status -1 (pending) and writes nothing else
//     <128, 1, 128>  a WORKGROUP per unit, 67 KiB of LDS: the pending units only, from a list the host made from info
// so the low degrees, which are nearly all of them, do not pay for the cap.  d > MBR_MAX_DEG is status 3.
//
// One body.  Thread i < d owns row i of the packed lower triangle (element (i,k) at i (i + 1) / 2 + k) in LDS:
//     gather      row i of the d x d block S[A, A] is read whole and tested for non-finite values; k <= i is stored
//     factor      left-looking, column k:  a_i = S_ik - sum_{q<k} L_iq L_kq  (q ascending, fused multiply-adds),
//                 pivot a_k through LDS, L_kk = sqrt(a_k), L_ik = a_i / L_kk
//     solve       column-oriented forward and backward substitution, the running value of row i in thread i's register, the
//                 finished component through LDS
//     q(M; beta)  thread i: x_i = fma(-2, M[A_i, j], sum_k M[A_i, A_k] beta_k) (k ascending); then every thread the same
//                 chain q = M_jj, q = fma(beta_i, x_i, q) (i ascending)
// Every sum has one fixed order, there is no atomic and no inline assembly: two calls give the same bits; a unit reads its
// own slot and matrix and writes its own row, so its bits depend neither on the other slots nor on the bin's other units.
// Every loop's trip count is bounded by d <= CAP or by p.
//
// Status (info[..,1]; info[..,0] = d):  0 solved / 1 a pivot not positive and finite / 2 a non-finite value among the gathered
// entries of S or, once the factor exists, of T / 3 d > MBR_MAX_DEG.  For 1, 2, 3 the node's tau^2, r and row of coef are
// NaN (the diagonal 0, as k_mb_path leaves a dead node).  Order of the tests: 3, 2 on S, 1, 2 on T.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

static constexpr int MBR_WAVE_DEG = 32;

template <int NT>
__device__ __forceinline__ void mbr_sync()
{
    if constexpr (NT == 64) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <int CAP>
struct MbrLds {
    static constexpr int TRI = CAP * (CAP + 1) / 2;
    // packed factor, beta, x, two broadcast doubles, the neighbour list, two flags (+ 2 ints of padding: a multiple of 16)
    static constexpr size_t BYTES = (size_t)(TRI + 2 * CAP + 2) * sizeof(double) + (size_t)(CAP + 4) * sizeof(int);
};

// q(M; beta) as described above; nf collects a non-finite entry of what it reads
template <int NT>
__device__ __forceinline__ double mbr_quad(const double* __restrict__ Mm, int p, int j, int d, const int* lst,
                                           const double* beta, double* x, int tid, bool& nf)
{
    if (tid < d) {
        const double* row = Mm + (size_t)lst[tid] * p;
        double w = 0.0;
        for (int k = 0; k < d; ++k) {
            const double v = row[lst[k]];
            nf |= not_finite(v);
            w = fma(v, beta[k], w);
        }
        const double mj = row[j];
        nf |= not_finite(mj);
        x[tid] = fma(-2.0, mj, w);
    }
    mbr_sync<NT>();
    double q = Mm[(size_t)j * p + j];
    nf |= not_finite(q);
    for (int i = 0; i < d; ++i) q = fma(beta[i], x[i], q);
    mbr_sync<NT>();
    return q;
}

template <int NT, int UPB, int CAP>
__global__ __launch_bounds__(NT * UPB) void k_mb_refit(const double* __restrict__ S, const double* __restrict__ T,
                                                       const double* __restrict__ W, double t, int p, long long nunits,
                                                       int sdiv, int smod, const int* __restrict__ list,
                                                       double* __restrict__ coef, double* __restrict__ resvar,
                                                       double* __restrict__ heldout, int* __restrict__ info)
{
    static_assert(NT % CAP == 0 && NT >= 64 && CAP <= NT, "a thread per row, whole rows per gather step");
    extern __shared__ __attribute__((aligned(16))) char mbr_smem[];
    const int tid = threadIdx.x % NT, w = threadIdx.x / NT;
    const long long at = (long long)blockIdx.x * UPB + w;
    if (at >= nunits) return;                                               // the whole group of a unit; no barrier is pending
    const long long unit = list ? (long long)list[at] : at;
    const size_t slot = (size_t)(unit / p);
    const int j = (int)(unit % p);
    const size_t pp = (size_t)p * p;
    const size_t mat = (slot / (size_t)sdiv) % (size_t)smod;
    const double* Sm = S + mat * pp;

    char* base = mbr_smem + (size_t)w * MbrLds<CAP>::BYTES;
    double* Lp = reinterpret_cast<double*>(base);
    double* beta = Lp + MbrLds<CAP>::TRI;
    double* x = beta + CAP;
    double* bc = x + CAP;                                                   // bc[0]: the pivot of the column
    int* lst = reinterpret_cast<int*>(bc + 2);
    int* flag = lst + CAP;                                                  // flag[0]: d, flag[1]: a non-finite value was read

    // the neighbour list: the first wave of the group, 64 entries of row j per step
    if (tid < 64) {
        const double* wr = W + slot * pp + (size_t)j * p;
        const unsigned long long below = (1ull << tid) - 1ull;
        int cnt = 0;
        for (int v0 = 0; v0 < p; v0 += 64) {
            const int idx = v0 + tid;
            const bool e = idx < p && idx != j && fabs(wr[idx]) >= t;
            const unsigned long long bal = __ballot(e);
            const int pos = cnt + __popcll(bal & below);
            if (e && pos < CAP) lst[pos] = idx;
            cnt += __popcll(bal);
        }
        if (tid == 0) {
            flag[0] = cnt;
            flag[1] = 0;
        }
    }
    mbr_sync<NT>();
    const int d = flag[0];
    double* crow = coef + slot * pp + (size_t)j * p;
    const size_t o = slot * (size_t)p + j;
    const double qnan = __builtin_nan("");

    auto finish_bad = [&](int status) {
        for (int i = tid; i < p; i += NT) crow[i] = i == j ? 0.0 : qnan;
        if (tid == 0) {
            resvar[o] = qnan;
            if (heldout) heldout[o] = qnan;
            info[o * 2] = d;
            info[o * 2 + 1] = status;
        }
    };
    auto any_nf = [&](bool nf) -> bool {
        if (nf) flag[1] = 1;
        mbr_sync<NT>();
        return flag[1] != 0;
    };

    if (d > CAP) {                                                          // uniform over the group
        if (d > MBR_MAX_DEG) {
            finish_bad(3);
        } else if (tid == 0) {
            info[o * 2] = d;
            info[o * 2 + 1] = -1;
        }
        return;
    }

    // gather: NT / CAP rows of the block per step
    bool nf = false;
    {
        const int gc = tid % CAP, gr = tid / CAP;
        for (int i0 = 0; i0 < d; i0 += NT / CAP) {
            const int i = i0 + gr;
            if (i < d && gc < d) {
                const double v = Sm[(size_t)lst[i] * p + lst[gc]];
                nf |= not_finite(v);
                if (gc <= i) Lp[i * (i + 1) / 2 + gc] = v;
            }
        }
    }
    double yi = 0.0;
    if (tid < d) {
        yi = Sm[(size_t)lst[tid] * p + j];
        nf |= not_finite(yi);
    }
    nf |= not_finite(Sm[(size_t)j * p + j]);
    if (any_nf(nf)) {
        finish_bad(2);
        return;
    }

    // factor
    const int ri = tid * (tid + 1) / 2;
    for (int k = 0; k < d; ++k) {
        const int rk = k * (k + 1) / 2;
        double a = 0.0;
        if (tid >= k && tid < d) {
            a = Lp[ri + k];
            for (int q = 0; q < k; ++q) a = fma(-Lp[ri + q], Lp[rk + q], a);
            if (tid == k) bc[0] = a;
        }
        mbr_sync<NT>();
        const double piv = bc[0];
        if (!(piv > 0.0) || not_finite(piv)) {                          // the same value in every thread
            finish_bad(1);
            return;
        }
        const double lkk = sqrt(piv);
        if (tid == k) Lp[ri + k] = lkk;
        else if (tid > k && tid < d) Lp[ri + k] = a / lkk;
        mbr_sync<NT>();
    }
    // L y = s_A: y_k to beta[k]
    for (int k = 0; k < d; ++k) {
        if (tid == k) beta[k] = yi / Lp[ri + k];
        mbr_sync<NT>();
        if (tid > k && tid < d) yi = fma(-Lp[ri + k], beta[k], yi);
    }
    // L' beta = y
    if (tid < d) yi = beta[tid];
    for (int k = d - 1; k >= 0; --k) {
        if (tid == k) beta[k] = yi / Lp[ri + k];
        mbr_sync<NT>();
        if (tid < k) yi = fma(-Lp[k * (k + 1) / 2 + tid], beta[k], yi);
    }
    mbr_sync<NT>();

    bool nfq = false;
    const double tau = mbr_quad<NT>(Sm, p, j, d, lst, beta, x, tid, nfq);
    double r = 0.0;
    if (heldout) {
        r = mbr_quad<NT>(T + mat * pp, p, j, d, lst, beta, x, tid, nfq);
        if (any_nf(nfq)) {
            finish_bad(2);
            return;
        }
    }
    if (tid < d) crow[lst[tid]] = beta[tid];
    if (tid == 0) {
        resvar[o] = tau;
        if (heldout) heldout[o] = r;
        info[o * 2] = d;
        info[o * 2 + 1] = 0;
    }
}

// q(T; beta) of coefficients that exist already: beta^(j) = ROW j of slot s of C (as k_mb_path leaves it), over its non-zero
// entries in ascending order, a wave per unit.  The sums and their order are those of mbr_quad for
// the support as the list; nothing is gathered into LDS, so there is no degree cap.  A NaN in the row or a non-finite
// entry of T that it reaches gives NaN.
__global__ __launch_bounds__(256) void k_mb_heldout(const double* __restrict__ T, const double* __restrict__ C, int p,
                                                    long long nunits, int sdiv, int smod, double* __restrict__ heldout)
{
    const int lane = threadIdx.x & 63;
    const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= nunits) return;
    const size_t slot = (size_t)(unit / p);
    const int j = (int)(unit % p);
    const size_t pp = (size_t)p * p;
    const double* Tm = T + ((slot / (size_t)sdiv) % (size_t)smod) * pp;
    const double* Cm = C + slot * pp;
    // lane l takes the rows i = l, l + 64, ... with beta_i != 0; x_i = fma(-2, T_ij, sum_k T_ik beta_k), k ascending
    double q = Tm[(size_t)j * p + j];
    for (int i0 = 0; i0 < p; i0 += 64) {
        const int i = i0 + lane;
        const double bi = i < p ? Cm[(size_t)j * p + i] : 0.0;
        double xi = 0.0;
        if (bi != 0.0) {                                                    // (a NaN is non-zero)
            double wsum = 0.0;
            for (int k = 0; k < p; ++k) {
                const double bk = Cm[(size_t)j * p + k];
                if (bk != 0.0) wsum = fma(Tm[(size_t)i * p + k], bk, wsum);
            }
            xi = fma(-2.0, Tm[(size_t)i * p + j], wsum);
        }
        // the chain over i ascending: the lanes of this step in order
        unsigned long long live = __ballot(bi != 0.0);
        while (live) {
            const int l = __builtin_ctzll(live);
            live &= live - 1;
            const double bl = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(bi), l),
                                               __builtin_amdgcn_readlane(__double2loint(bi), l));
            const double xl = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xi), l),
                                               __builtin_amdgcn_readlane(__double2loint(xi), l));
            q = fma(bl, xl, q);
        }
    }
    if (lane == 0) heldout[slot * (size_t)p + j] = q;
}

template <int NT, int UPB, int CAP>
static void mbr_launch(hipStream_t st, const double* S, const double* T, const double* W, double t, int p, long long nunits,
                       int sdiv, int smod, const int* list, double* coef, double* resvar, double* heldout, int* info)
{
    const size_t lds = (size_t)UPB * MbrLds<CAP>::BYTES;
    static_assert(MbrLds<CAP>::BYTES % 16 == 0, "every unit's LDS starts 16-byte aligned");
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void*)k_mb_refit<NT, UPB, CAP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_mb_refit<NT, UPB, CAP>), dim3((unsigned)((nunits + UPB - 1) / UPB)), dim3(NT * UPB), lds, st, S, T, W, t,
                       p, nunits, sdiv, smod, list, coef, resvar, heldout, info);
}

void launch_mb_refit(hipStream_t st, const double* S, const double* T, const double* W, double t, int p, size_t nslot, int sdiv,
                     int smod, double* coef, double* resvar, double* heldout, int* info)
{
    mbr_launch<64, 4, MBR_WAVE_DEG>(st, S, T, W, t, p, (long long)nslot * p, sdiv, smod, nullptr, coef, resvar, heldout, info);
}

void launch_mb_refit_listed(hipStream_t st, const double* S, const double* T, const double* W, double t, int p, const int* list,
                            int nlist, int sdiv, int smod, double* coef, double* resvar, double* heldout, int* info)
{
    if (nlist < 1) return;
    mbr_launch<128, 1, MBR_MAX_DEG>(st, S, T, W, t, p, nlist, sdiv, smod, list, coef, resvar, heldout, info);
}

void launch_mb_heldout(hipStream_t st, const double* T, const double* C, int p, size_t nslot, int sdiv, int smod, double* heldout)
{
    const long long nunits = (long long)nslot * p;
    hipLaunchKernelGGL(k_mb_heldout, dim3((unsigned)((nunits + 3) / 4)), dim3(256), 0, st, T, C, p, nunits, sdiv, smod, heldout);
}

}  // namespace ggl
