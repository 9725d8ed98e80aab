// Tile geometry and XCD-aware work decoding shared by the register-staged FP64 matrix-core kernels: the symmetric
// products of gemm_sym.hip and the Gram tile body of gram_nt_tile.hpp (covariance.hip, covariance_missing.hip,
// covariance_weighted.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ggl {

typedef double v4d __attribute__((ext_vector_type(4)));

template <int BM, int BK, int WM, int WN, bool LM>
struct SymCfg {
    static constexpr int NWR = BM / WM, NWC = BM / WN, NW = NWR * NWC, NT = NW * 64;
    static constexpr int TI = WM / 16, TJ = WN / 16;
    static constexpr int LDS_LD = BM + 16;           // consecutive rows start on opposite bank halves
    static constexpr int SLAB = BK * LDS_LD;          // doubles per operand slab
    static constexpr int CLD = BM + 1;
    static constexpr int LDS_DOUBLES = (!LM || 2 * SLAB > BM * CLD) ? 2 * SLAB : BM * CLD;   // LM: mirror via LDS
    static constexpr int LPT = (BK * BM) / NT;       // elements per thread per operand slab
    static_assert((BK * BM) % NT == 0, "slab must divide evenly over the threads");
    static_assert(NT % BM == 0, "a row of the slab must be covered by whole thread rows");
};

constexpr int sym_nt(int BM, int WM, int WN) { return (BM / WM) * (BM / WN) * 64; }

// XCD-aware work decode.  The 8 XCDs have private 4 MiB L2s and the dispatcher deals consecutive
// workgroup ids round-robin over them (id % 8, observed; only speed depends on it).  A 1-D grid of
// 8 * ceil(K/8) * ntiles ids is decoded so that all tiles of instance k run on XCD k % 8 and
// follow each other in dispatch order: the two operand matrices of an instance (2 x 8 p^2 bytes)
// are then fetched into ONE L2 once and reused by all of its tiles, instead of being streamed
// into all eight.  Batches smaller than 8 keep the plain (tile, k) order so that every XCD has work.
static constexpr int NXCD = 8;
// batches of 1, 2 or 4 instances: 8 / K XCDs share one instance (its tiles interleaved over them), so an XCD's L2 still
// holds the operands of ONE instance only instead of slices of all of them
__host__ __device__ inline int xcd_share(int K) { return (K == 1 || K == 2 || K == 4) ? NXCD / K : 0; }
// K >= 8: whole rounds of eight instances as above; the K % 8 instances that are left over are dealt like a small batch
// of their own (8 / r XCDs per instance for r = 1, 2, 4, else plain tile order) -- as a "ninth, tenth, ..." instance of the
// first XCDs they would leave the other XCDs idle for a whole instance (K = 20: 3 against 2 instances per XCD; measured
// with an uneven split of the headline: 18 instead of 16 per launch costs 8 %).
__host__ __device__ inline int xcd_grid_small(int ntiles, int K)
{
    const int g = xcd_share(K);
    return g ? NXCD * ((ntiles + g - 1) / g) : NXCD * ((ntiles * K + NXCD - 1) / NXCD);
}
__host__ __device__ inline int xcd_grid(int ntiles, int K)
{
    if (K < NXCD) return xcd_grid_small(ntiles, K);
    const int r = K % NXCD;
    return NXCD * (K / NXCD) * ntiles + (r ? xcd_grid_small(ntiles, r) : 0);
}
__device__ __forceinline__ bool decode_block_small(int ntiles, int K, int& k, int& tile, int L)
{
    const int g = xcd_share(K);
    if (g) {
        const int xcd = L % NXCD, slot = L / NXCD;
        k = xcd / g;
        tile = slot * g + xcd % g;
        return tile < ntiles;
    }
    k = L / ntiles;
    tile = L % ntiles;
    return k < K;
}
__device__ __forceinline__ bool decode_block_xcd(int ntiles, int K, int& k, int& tile, int L)
{
    if (K < NXCD) return decode_block_small(ntiles, K, k, tile, L);
    const int nfull = NXCD * (K / NXCD) * ntiles;          // a multiple of 8: L % 8 is still the XCD behind it
    if (L < nfull) {
        const int xcd = L % NXCD, slot = L / NXCD;
        k = (slot / ntiles) * NXCD + xcd;
        tile = slot % ntiles;
        return true;
    }
    const bool ok = decode_block_small(ntiles, K % NXCD, k, tile, L - nfull);
    k += (K / NXCD) * NXCD;
    return ok;
}
__device__ __forceinline__ bool decode_block_xcd(int ntiles, int K, int& k, int& tile)
{
    return decode_block_xcd(ntiles, K, k, tile, (int)blockIdx.x);
}

}  // namespace ggl
