// What the metric kernels on float32 feature rows (kid.hip, prdc.hip) share: one 64 x 64 tile of inner products <p_i, q_j> on the fp64 matrix
// cores (v_mfma_f64_16x16x4_f64) and the wave-level sum in a fixed order.  Nothing here multiplies and adds outside the MFMAs, so the
// including file's `#pragma clang fp contract(off)` has nothing to act on in this header.
#pragma once
#include "wu_common.h"

namespace {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int kGramTile = 64;         // rows / columns of a workgroup's tile
constexpr int kGramKC = 32;           // features per staged chunk
constexpr int kGramLd = kGramKC + 1;  // LDS row stride of a staged chunk in doubles: rows 8 bytes apart in bank space

// wave-level sum in a fixed order (lane l takes lane l + off, off = 32 .. 1); the total lands in lane 0
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// <p_i, q_j> of one 64 x 64 tile, computed by a workgroup of 256 threads (four waves) into the calling wave's acc[2][2].
//
// Rows.  prow(r) / qrow(r), r = 0..63, give the `const float*` of the feature row behind tile row / tile column r.  They must return a
// readable row of at least D floats for EVERY r: a position past the end of the data is clamped to a valid row by the callable and its
// entries are masked by the caller's epilogue, so nothing reads out of bounds.
//
// Staging.  Thread -> feature k = tid & 31 of rows (tid >> 5) + 8 e, e = 0..7, of the tile rows and of the tile columns, widened to fp64 on
// the way into sP / sQ (kGramTile * kGramLd doubles each, [row][k]); the tail of the last chunk is zero-filled; the next chunk's global
// loads fly under this chunk's MFMAs.
//
// Fragments.  Each wave owns a 32 x 32 sub-tile at rows wr = 32 (wave >> 1), columns wc = 32 (wave & 1): 2 x 2 accumulators of 16 x 16.
// A = P[i = lane & 15][k], B = Q[j = lane & 15][k], one f64 per lane, lane group g = lane >> 4 taking one k of every four.  WHICH k a group
// takes only has to agree between A and B: group g reads k = 16 (g & 1) + 8 (g >> 1) + step, so the two groups of a half-wave sit 128 bytes
// apart in LDS and do not share banks.  f64 C/D map, which the callers' epilogues rely on: acc[a][b][reg] is the entry at
// row wr + 16 a + (lane >> 4) + 4 reg, column wc + 16 b + (lane & 15) of the tile.
//
// Barriers.  Every chunk starts with a barrier, so the caller may have used sP / sQ for something else before the call; it must place a
// barrier of its own before it reuses them after it.  All 256 threads must make the call (D is uniform over the workgroup).
template <class PRow, class QRow>
__device__ __forceinline__ void gram_tile_f64(PRow prow, QRow qrow, int D, double* sP, double* sQ, f64x4_t (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sk = tid & 31, sr = tid >> 5;
    const float* pr[8];
    const float* qr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        pr[e] = prow(sr + 8 * e);
        qr[e] = qrow(sr + 8 * e);
    }
    float pv[8], qv[8];
    auto fetch = [&](int k0) {
        const int k = k0 + sk;
        const bool ok = k < D;                     // zero-filled tail of the last chunk
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            pv[e] = ok ? pr[e][k] : 0.f;
            qv[e] = ok ? qr[e][k] : 0.f;
        }
    };
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int kg = 16 * (g & 1) + 8 * (g >> 1);
    const double* aP = sP + (wr + l15) * kGramLd + kg;
    const double* bQ = sQ + (wc + l15) * kGramLd + kg;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4_t{0.0, 0.0, 0.0, 0.0};

    fetch(0);
    for (int k0 = 0; k0 < D; k0 += kGramKC) {
        __syncthreads();                           // the previous chunk (or the caller's use of the buffers) has been consumed
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sP[(sr + 8 * e) * kGramLd + sk] = (double)pv[e];
            sQ[(sr + 8 * e) * kGramLd + sk] = (double)qv[e];
        }
        __syncthreads();
        if (k0 + kGramKC < D) fetch(k0 + kGramKC); // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            const double a0 = aP[st], a1 = aP[16 * kGramLd + st];
            const double b0 = bQ[st], b1 = bQ[16 * kGramLd + st];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

}  // namespace
