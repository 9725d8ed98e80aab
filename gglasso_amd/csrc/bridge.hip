// Latent correlation of mixed binary / continuous data: the Gaussian copula model of Fan, Liu, Ning, Zou (2017, JRSS-B), the
// estimator of R's mixedCCA / latentcor, behind the exact counts G of kendall.hip.
//
//     tau          = G_ij / (n (n - 1) / 2)                                Kendall's tau-a over the n samples of a subset
//     Delta_i      = the normal quantile of n0_i / n                       binary i: n0_i samples of rank 0      k_bridge_zero_counts
//     F(r)         = c int_0^{A(r)} g(t; h, k) dt = tau,   g(t; h, k) = exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t))    k_bridge_invert
//       binary, binary:      c = 1/pi,  A = asin r,           h = Delta_i, k = Delta_j
//       binary, continuous:  c = 2/pi,  A = asin(r / sqrt 2), h = Delta,   k = 0
//       continuous pair:     r = sin(pi/2 tau), no root to find
//
// (Plackett's identity d Phi_2(h,k;r) / dr = phi_2(h,k;r) turns both bridges into this one integral; the Phi(Delta) terms
// cancel, so the kernel needs no normal distribution function.)
//
// The root is found in the angle: H(x) = c x sum_n v_n g(x u_n) = tau for x in [-A(clip), A(clip)], with (u_n, v_n) the 64-node
// Gauss-Legendre rule on [0, 1], and r = sin x (sqrt 2 sin x).  H' = c g(x) > 0: H is increasing, and H(x) has the sign of x,
// so the bracket is [0, A(clip)] or its mirror image.  Safeguarded Newton: a step that leaves the bracket is replaced by its
// midpoint.
//
// Thread mapping: ONE PAIR PER WAVE, ONE NODE PER LANE.  Lane n holds (u_n, v_n) in registers, evaluates the integrand at x u_n
// and the 64 terms meet in a butterfly (wave_sum: six steps, every lane ends with the same bits).  Everything that steers the
// iteration -- tau, the bracket, the iterate -- is then the same in all 64 lanes: the loop's trip count is uniform across the
// wave whatever the neighbouring pairs need, pairs of different types never share a wave, and a small matrix still fills the
// device (p = 33 has 528 pairs: 528 waves here, 9 with a pair per lane).  The price is the scalar part (the derivative, the
// quantiles), which all lanes repeat.  The sum has one fixed order, nothing is accumulated through atomics: two calls give the
// same bits.  Every unordered pair is solved once and written to (i,j) and (j,i).
#include "common.hpp"
#include "kernels.hpp"

namespace ggl {

// the 64-node Gauss-Legendre rule on [0, 1]: u = (1 + x) / 2, v = w / 2 (nodes by Newton on P_64 in extended precision, rounded)
__device__ static const double BR_U[64] = {
    0.0003474791321139303, 0.0018299416140223604, 0.00449331426162784, 0.008331873057687022,
    0.013336586105044517, 0.01949560017397314, 0.026794312570798593, 0.035215413934030215,
    0.044738931460748595, 0.055342277002442944, 0.06700030092295359, 0.07968535187370981,
    0.09336734243860122, 0.1080138205283293, 0.12359004636973406, 0.1400590749141946,
    0.15738184347288336, 0.17551726437267132, 0.19442232241380336, 0.21405217689868297,
    0.23436026799005272, 0.2552984271464735, 0.27681699137326793, 0.2988649210180042,
    0.32138992083116596, 0.34433856400489454, 0.3676564188956163, 0.39128817812999644,
    0.41517778978800357, 0.4392685903519397, 0.4635034391061005, 0.48782485366828776,
    0.5121751463317122, 0.5364965608938995, 0.5607314096480602, 0.5848222102119964,
    0.6087118218700035, 0.6323435811043837, 0.6556614359951055, 0.6786100791688341,
    0.7011350789819958, 0.723183008626732, 0.7447015728535265, 0.7656397320099473,
    0.7859478231013171, 0.8055776775861966, 0.8244827356273287, 0.8426181565271166,
    0.8599409250858054, 0.876409953630266, 0.8919861794716707, 0.9066326575613988,
    0.9203146481262902, 0.9329996990770464, 0.944657722997557, 0.9552610685392514,
    0.9647845860659698, 0.9732056874292014, 0.9805043998260269, 0.9866634138949555,
    0.991668126942313, 0.9955066857383722, 0.9981700583859776, 0.999652520867886};
__device__ static const double BR_V[64] = {
    0.0008916403608482165, 0.002073516630281234, 0.0032522289844891814, 0.0044233799131819735,
    0.005584069730065564, 0.006731523948359321, 0.007863015238012359, 0.008975857887848672,
    0.010067411576765104, 0.011135086904191627, 0.012176351284355437, 0.01318873485752733,
    0.014169836307129742, 0.015117328536201239, 0.016028964177425775, 0.016902580918570803,
    0.017736106628441193, 0.018527564270120023, 0.019275076589307813, 0.01997687056636017,
    0.020631281621311764, 0.021236757561826795, 0.021791862264661725, 0.022295279081878283,
    0.02274581396370907, 0.023142398290657208, 0.02348409140810501, 0.023770082857415154,
    0.023999694298229155, 0.024172381117401477, 0.024287733720751714, 0.024345478504569862,
    0.024345478504569862, 0.024287733720751714, 0.024172381117401477, 0.023999694298229155,
    0.023770082857415154, 0.02348409140810501, 0.023142398290657208, 0.02274581396370907,
    0.022295279081878283, 0.021791862264661725, 0.021236757561826795, 0.020631281621311764,
    0.01997687056636017, 0.019275076589307813, 0.018527564270120023, 0.017736106628441193,
    0.016902580918570803, 0.016028964177425775, 0.015117328536201239, 0.014169836307129742,
    0.01318873485752733, 0.012176351284355437, 0.011135086904191627, 0.010067411576765104,
    0.008975857887848672, 0.007863015238012359, 0.006731523948359321, 0.005584069730065564,
    0.0044233799131819735, 0.0032522289844891814, 0.002073516630281234, 0.0008916403608482165};

static constexpr int BR_MAXIT = 64;                       // (Newton takes 3 .. 7 steps; a bisection step halves the bracket)
static constexpr double BR_FTOL = 4.440892098500626e-16;  // 2^-51: |H - tau| at which the iteration ends (H, tau are below 1)

// one wave per (subset, variable): the samples of rank 0, and whether the variable varies over the subset at all
__global__ __launch_bounds__(256) void k_bridge_zero_counts(const int* __restrict__ Rg, int* __restrict__ n0, int* __restrict__ err,
                                                            int p, int b)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), r = blockIdx.y;
    if (i >= p) return;                                   // (the whole wave)
    const int* row = Rg + ((size_t)r * p + i) * b;
    int cnt = 0, mn = 0x7fffffff, mx = -1;
    for (int c = lane; c < b; c += 64) {
        const int v = row[c];
        cnt += (v == 0);
        mn = min(mn, v);
        mx = max(mx, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        mn = min(mn, __shfl_xor(mn, off, 64));
        mx = max(mx, __shfl_xor(mx, off, 64));
    }
    if (lane == 0) {
        n0[(size_t)r * p + i] = cnt;
        if (mn == mx) atomicMin(err, r * p + i);
    }
}

// Delta = the normal quantile of n0 / b, 0 < n0 < b; taken from the lower tail, whose argument is an exactly rounded quotient
__device__ __forceinline__ double br_delta(int n0, int b)
{
    return 2 * (long long)n0 <= b ? normcdfinv((double)n0 / (double)b) : -normcdfinv((double)(b - n0) / (double)b);
}

// lane 0's value in every lane, as a scalar
__device__ __forceinline__ double br_first(double v)
{
    const unsigned long long w = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(w >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// H(x) = c x sum_n v_n g(x u_n; h, k) with h2k2 = h^2 + k^2, hk2 = 2 h k; the same bits in every lane.  The butterfly alone
// does not give that: the compiler contracts a lane's product v g with the first addition into one fma, so lane l adds the
// partner's ROUNDED term to its own unrounded one, lane l ^ 32 the other way round, and the two differ in the last bit.  An
// iteration that ends within that bit of BR_FTOL then ended in some lanes only, and the rest went on summing over a part of
// the wave (one pair in 10^5 at p = 500, found by the residual of tools/bench_mixed.py).  Lane 0's sum is the wave's.
__device__ __forceinline__ double br_H(double x, double h2k2, double hk2, double c, double u, double v)
{
    double s, co;
    sincos(x * u, &s, &co);
    return c * x * br_first(wave_sum(v * exp(-(h2k2 - hk2 * s) / (2.0 * co * co))));
}

__global__ __launch_bounds__(256) void k_bridge_invert(const long long* __restrict__ G, const int* __restrict__ n0,
                                                       const int* __restrict__ types, double* __restrict__ S,
                                                       int* __restrict__ clipped, const int* __restrict__ err, int p, int b,
                                                       long long npairs, double nn, double clip)
{
    if (*err != GGL_DIAG_OK) return;
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the wave's pair
    const int r = blockIdx.y;
    const size_t pp = (size_t)p * p;
    double* Sr = S + r * pp;
    if (q >= npairs) {
        // the waves behind the pairs write the diagonal, 64 entries each
        const long long d = (q - npairs) * 64 + lane;
        if (d < p) Sr[(size_t)d * p + d] = 1.0;
        return;
    }
    // q = i (2 p - i - 1) / 2 + (j - i - 1), i < j: the upper triangle row by row
    const double tp = 2.0 * p - 1.0;
    int i = (int)(0.5 * (tp - sqrt(tp * tp - 8.0 * (double)q)));
    i = max(0, min(i, p - 2));
    while ((long long)i * (2ll * p - i - 1) / 2 > q) --i;
    while ((long long)(i + 1) * (2ll * p - i - 2) / 2 <= q) ++i;
    const int j = (int)(q - (long long)i * (2ll * p - i - 1) / 2) + i + 1;

    const double tau = (double)G[r * pp + (size_t)i * p + j] / nn;
    const int ti = types[i], tj = types[j];
    double res;
    bool hit = false;
    if (!ti && !tj) {
        res = sin(1.5707963267948966 * tau);
    } else {
        const bool bb = ti && tj;
        const double h = br_delta(n0[(size_t)r * p + (ti ? i : j)], b);
        const double k = bb ? br_delta(n0[(size_t)r * p + j], b) : 0.0;
        const double h2k2 = h * h + k * k, hk2 = 2.0 * h * k;
        const double c = bb ? 0.3183098861837907 : 0.6366197723675814;           // 1 / pi, 2 / pi
        const double amp = bb ? 1.0 : 1.4142135623730951;
        const double u = BR_U[lane], v = BR_V[lane];
        const double xc = asin(clip / amp);
        const double xe = tau >= 0.0 ? xc : -xc;                                  // the end on tau's side
        const double Fe = br_H(xe, h2k2, hk2, c, u, v);
        if (tau >= 0.0 ? tau >= Fe : tau <= Fe) {
            res = tau >= 0.0 ? clip : -clip;
            hit = true;
        } else {
            double lo = fmin(0.0, xe), hi = fmax(0.0, xe);
            double x = tau / (c * exp(-0.5 * h2k2));                              // H is c g(0) x to first order
            if (!(x > lo && x < hi)) x = 0.5 * (lo + hi);
            for (int it = 0; it < BR_MAXIT; ++it) {
                const double f = br_H(x, h2k2, hk2, c, u, v) - tau;
                if (fabs(f) <= BR_FTOL) break;
                if (f > 0.0) hi = x; else lo = x;
                double s, co;
                sincos(x, &s, &co);
                const double d = c * exp(-(h2k2 - hk2 * s) / (2.0 * co * co));    // H'(x); 0 where exp underflows: then bisect
                double xn = x - f / d;
                if (!(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
                if (xn == x) break;
                x = xn;
            }
            res = fmin(fmax(amp * sin(x), -clip), clip);
        }
    }
    if (lane == 0) {
        Sr[(size_t)i * p + j] = res;
        Sr[(size_t)j * p + i] = res;
        if (hit) atomicAdd(clipped + r, 1);                                       // (an integer count: order does not matter)
    }
}

void launch_bridge_zero_counts(hipStream_t st, const int* Rg, int* n0, int* err, int B, int p, int b)
{
    hipLaunchKernelGGL(k_bridge_zero_counts, dim3((p + 3) / 4, B), dim3(256), 0, st, Rg, n0, err, p, b);
}

void launch_bridge_invert(hipStream_t st, const long long* G, const int* n0, const int* types, double* S, int* clipped,
                          const int* err, int B, int p, int b, double clip)
{
    (void)hipMemsetAsync(clipped, 0, (size_t)B * sizeof(int), st);
    const long long npairs = (long long)p * (p - 1) / 2;
    const long long waves = npairs + (p + 63) / 64;                              // (p <= 23104: kendall_counts_fit)
    const double nn = (double)((long long)b * (b - 1) / 2);
    hipLaunchKernelGGL(k_bridge_invert, dim3((unsigned)((waves + 3) / 4), B), dim3(256), 0, st, G, n0, types, S, clipped, err, p,
                       b, npairs, nn, clip);
}

}  // namespace ggl
