// Azimuthally averaged power spectrum of image luma (wu/spectrum.py; tests/_spectrum_ref.py states the arithmetic).  A DFT of any side up to
// 1024 as two matrix products against twiddle tables on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), every sum in an order that depends
// on the sizes alone:
//   * spectrum_luma_kernel      one thread per pixel: value mapping, luma, window -> fp64 plane (the two-step path and the tests);
//   * spectrum_order_kernel     a workgroup per 64 x 64 tile of the (H, Wh) half spectrum: the integer radial bin of every entry, then a
//                               counting sort of the tile's entries by bin (entries of one bin in row-major order) and the mirror-weighted
//                               count per bin.  Static per (H, W); rebuilt in the workspace by every call (its time was not measured);
//   * spectrum_rows_kernel      row stage: 64 rows (of the N H rows of a chunk) x 64 frequencies v per workgroup, [Tr | Ti] = Y . [C_W | -S_W].
//                               The Y tile is staged in LDS 32 columns at a time -- from an fp64 plane, or from the strided source with
//                               luma and window applied on the way (the production path: no fp64 plane exists in memory); the twiddle
//                               operand is read from the 1-D tables in LDS at (v j) mod W;
//   * spectrum_cols_kernel      column stage: 64 u x 64 v per workgroup and image, Xr = C_H Tr + S_H Ti, Xi = C_H Ti - S_H Tr (2 H terms each);
//                               Tr / Ti tiles staged 32 rows at a time, the twiddle operand from the tables at (u i) mod H.  Epilogue:
//                               P = Xr Xr + Xi Xi (times the mirror weight) to LDS, one thread per bin of the tile adds its entries in the
//                               order kernel's order -> per-tile partials.  P reaches memory only when the spectrum sum was asked for:
//                               the stage is then launched image by image, n ascending, and every entry's thread adds its P to the
//                               caller's sum (one owner per entry and launch, launches in stream order: a fixed order, no plane);
//   * spectrum_fold_kernel      prof[n][k] = (sum over tiles ascending of the partials) / count[k] / (H W)^2.
// No floating-point atomics; two runs give the same bits, and an image's profile does not depend on which images share its call.
#include <math.h>

#include <type_traits>

#include "wu_common.h"

// products and sums outside the MFMAs are rounded on their own, as the numpy restatement does
#pragma clang fp contract(off)

namespace {

typedef double f64x4_t __attribute__((ext_vector_type(4)));

constexpr int kSpMaxSide = 1024;
constexpr int kSpMaxN = 65535;             // images per call: the column stage puts the image in grid.y
constexpr int kSpTile = 64;                // rows / columns of a workgroup's tile
constexpr int kSpKC = 32;                  // inner-product terms per staged chunk
constexpr int kSpLd = kSpKC + 1;           // LDS row stride of a staged chunk in doubles
constexpr int kSpTileBins = 128;           // a 64 x 64 tile spans fewer than 64 sqrt(2) + 2 radial bins
constexpr int kSpF64 = 3;                  // a plane in memory (after WU_F32 / WU_BF16 / WU_SSIM_U8)

// what the order kernel leaves per tile
struct SpTileOrder {
    int kmin, nb;                          // the tile's entries fall in bins kmin .. kmin + nb - 1
    int seg[kSpTileBins + 1];              // perm[seg[b] .. seg[b + 1]) are the entries of bin kmin + b
    int wcount[kSpTileBins];               // their mirror weights, summed
    unsigned short perm[kSpTile * kSpTile];   // row * 64 + col of the tile's valid entries, sorted by bin, row-major inside a bin
};

// floor(sqrt(x)) for 0 <= x < 2^62
__host__ __device__ __forceinline__ long long sp_isqrt(long long x) {
    long long r = (long long)sqrt((double)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

// radial bin of the entry (u, v) of the half spectrum: integers only
__host__ __device__ __forceinline__ int sp_bin(int u, int v, int H, int W) {
    const long long fu = u <= H / 2 ? u : u - H, fv = v, M = H < W ? H : W;
    const long long q = fu * fu * W * W + fv * fv * H * H;
    return (int)(sp_isqrt(q * M * M) / ((long long)H * W));
}

// the bin index is monotone in |fu| and fv: the largest one sits at (H / 2, W / 2)
int sp_bins(int H, int W) { return sp_bin(H / 2, W / 2, H, W) + 1; }

__host__ __device__ __forceinline__ int sp_weight(int v, int W) { return v > 0 && 2 * v < W ? 2 : 1; }

struct SpSource {
    const void* x;               // element strides (n, c, h, w); a plane: (H W, 0, W, 1)
    long long xs[4];
    int C, H, W;
    double scale, shift, L;
    const double* wh;            // window tables of H and W doubles, or NULL
    const double* ww;
};

// the windowed luma of pixel (i, j) of image n
template <int DT> __device__ __forceinline__ double sp_value(const SpSource& a, long long n, int i, int j) {
    const long long at = n * a.xs[0] + i * a.xs[2] + j * a.xs[3];
    if (DT == kSpF64) return ((const double*)a.x)[at];
    double s[3];
    for (int c = 0; c < a.C; ++c) {
        const long long e = at + c * a.xs[1];
        double v;
        if (DT == WU_BF16) v = (double)bf16_to_f32(((const bf16_t*)a.x)[e]);
        else if (DT == WU_SSIM_U8) v = (double)((const unsigned char*)a.x)[e];
        else v = (double)((const float*)a.x)[e];
        v = v * a.scale;
        v = v + a.shift;
        s[c] = v / a.L;
    }
    double y = s[0];
    if (a.C == 3) {
        const double r = 0.299 * s[0], g = 0.587 * s[1], b = 0.114 * s[2];
        y = r + g;
        y = y + b;
    }
    if (a.wh) {
        y = y * a.wh[i];
        y = y * a.ww[j];
    }
    return y;
}

template <int DT> __global__ __launch_bounds__(256) void spectrum_luma_kernel(const SpSource a, long long total, double* out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % a.W), i = (int)((idx / a.W) % a.H);
    out[idx] = sp_value<DT>(a, idx / ((long long)a.H * a.W), i, j);
}

// grid (tiles): tile t covers u in [64 (t / tv), ..), v in [64 (t % tv), ..)
__global__ __launch_bounds__(256) void spectrum_order_kernel(int H, int W, int Wh, int tv, SpTileOrder* order) {
    __shared__ int sBin[kSpTile * kSpTile];
    __shared__ int sSeg[kSpTileBins + 1];
    __shared__ int sRange[2];
    const int tid = threadIdx.x;
    const int u0 = (blockIdx.x / tv) * kSpTile, v0 = (blockIdx.x % tv) * kSpTile;
    SpTileOrder* o = order + blockIdx.x;
    if (tid == 0) sRange[0] = 0x7fffffff, sRange[1] = -1;
    __syncthreads();
    for (int e = tid; e < kSpTile * kSpTile; e += 256) {
        const int u = u0 + (e >> 6), v = v0 + (e & 63);
        int k = -1;
        if (u < H && v < Wh) {
            k = sp_bin(u, v, H, W);
            atomicMin(&sRange[0], k);      // integers: any order gives the same result
            atomicMax(&sRange[1], k);
        }
        sBin[e] = k;
    }
    __syncthreads();
    const int kmin = sRange[0];
    const int nb = min(sRange[1] - kmin + 1, kSpTileBins);
    int cnt = 0, wc = 0;
    if (tid < nb) {
        for (int e = 0; e < kSpTile * kSpTile; ++e)
            if (sBin[e] == kmin + tid) {
                ++cnt;
                wc += sp_weight(v0 + (e & 63), W);
            }
        sSeg[tid + 1] = cnt;
        o->wcount[tid] = wc;
    }
    __syncthreads();
    if (tid == 0) {
        sSeg[0] = 0;
        for (int b = 0; b < nb; ++b) sSeg[b + 1] += sSeg[b];
        o->kmin = kmin;
        o->nb = nb;
    }
    __syncthreads();
    if (tid <= nb) o->seg[tid] = sSeg[tid];
    if (tid < nb) {
        int at = sSeg[tid];
        for (int e = 0; e < kSpTile * kSpTile; ++e)
            if (sBin[e] == kmin + tid) o->perm[at++] = (unsigned short)e;
    }
}

// One k-chunk of MFMAs.  The staged operand sits in LDS as [row][k] at stride kSpLd; lane group g = lane >> 4 takes k = kg + st of the
// chunk, kg = 16 (g & 1) + 8 (g >> 1), st = 0..7 (the k order of csrc/gram_f64.h).  The twiddle operand of row / column r at term k is
// tab[(r k) mod n]: a lane starts the chunk at (r (k0 + kg)) mod n and steps by r mod n.
struct SpTwiddle {
    int at[2], step[2];
    __device__ __forceinline__ void start(int r0, int r1, int k, int n) {
        step[0] = r0 % n, step[1] = r1 % n;
        at[0] = (int)(((long long)step[0] * k) % n);
        at[1] = (int)(((long long)step[1] * k) % n);
    }
    __device__ __forceinline__ void next(int n) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            at[b] += step[b];
            if (at[b] >= n) at[b] -= n;
        }
    }
};

struct SpRowsArgs {
    SpSource src;
    long long rows;              // N H
    int Wh;
    const double* cw;            // cos / sin of 2 pi k / W, k < W
    const double* sw;
    double* T;                   // (N H, 2 Wh): [Tr | Ti]
};

// grid (row tiles, v tiles)
template <int DT> __global__ __launch_bounds__(256) void spectrum_rows_kernel(const SpRowsArgs a) {
    __shared__ double sY[kSpTile * kSpLd];
    __shared__ double sC[kSpMaxSide], sS[kSpMaxSide];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.src.W, H = a.src.H, Wh = a.Wh;
    const long long r0 = (long long)blockIdx.x * kSpTile;
    const int v0 = blockIdx.y * kSpTile;
    for (int k = tid; k < W; k += 256) {
        sC[k] = a.cw[k];
        sS[k] = -a.sw[k];        // Ti = -sum y s: the negation is exact
    }
    // staging: thread -> column sk of rows sr + 8 e of the tile
    const int sk = tid & 31, sr = tid >> 5;
    long long img[8];
    int row[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const long long r = r0 + sr + 8 * e;
        img[e] = r < a.rows ? r / H : -1;
        row[e] = (int)(r % H);
    }
    double yv[8];
    auto fetch = [&](int k0) {
        const int j = k0 + sk;
#pragma unroll
        for (int e = 0; e < 8; ++e) yv[e] = (j < W && img[e] >= 0) ? sp_value<DT>(a.src, img[e], row[e], j) : 0.0;
    };
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int kg = 16 * (g & 1) + 8 * (g >> 1);
    const double* aY = sY + (wr + l15) * kSpLd + kg;
    f64x4_t accR[2][2], accI[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) accR[p][q] = accI[p][q] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    SpTwiddle tw;
    fetch(0);
    for (int k0 = 0; k0 < W; k0 += kSpKC) {
        __syncthreads();         // the previous chunk has been consumed (first pass: nothing yet)
#pragma unroll
        for (int e = 0; e < 8; ++e) sY[(sr + 8 * e) * kSpLd + sk] = yv[e];
        __syncthreads();         // also publishes the tables on the first pass
        if (k0 + kSpKC < W) fetch(k0 + kSpKC);
        tw.start(v0 + wc + l15, v0 + wc + 16 + l15, k0 + kg, W);
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            const double a0 = aY[st], a1 = aY[16 * kSpLd + st];
            const double c0 = sC[tw.at[0]], c1 = sC[tw.at[1]], s0 = sS[tw.at[0]], s1 = sS[tw.at[1]];
            tw.next(W);
            accR[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c0, accR[0][0], 0, 0, 0);
            accR[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c1, accR[0][1], 0, 0, 0);
            accR[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c0, accR[1][0], 0, 0, 0);
            accR[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c1, accR[1][1], 0, 0, 0);
            accI[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, s0, accI[0][0], 0, 0, 0);
            accI[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, s1, accI[0][1], 0, 0, 0);
            accI[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, s0, accI[1][0], 0, 0, 0);
            accI[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, s1, accI[1][1], 0, 0, 0);
        }
    }
    // C/D map: acc[p][q][reg] is row wr + 16 p + (lane >> 4) + 4 reg, column wc + 16 q + (lane & 15) of the tile
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const long long r = r0 + wr + 16 * p + g + 4 * reg;
                const int v = v0 + wc + 16 * q + l15;
                if (r < a.rows && v < Wh) {
                    a.T[r * (2 * Wh) + v] = accR[p][q][reg];
                    a.T[r * (2 * Wh) + Wh + v] = accI[p][q][reg];
                }
            }
}

struct SpColsArgs {
    const double* T;             // (N, H, 2 Wh)
    int H, W, Wh, tv, tiles;
    const double* ch;            // cos / sin of 2 pi k / H, k < H
    const double* sh;
    const SpTileOrder* order;
    double* partial;             // (N, tiles, kSpTileBins)
    double* sum2d;               // (H, Wh) running sum of P, or NULL
    int n0;                      // first image of the launch
};

// grid (tiles, images of the launch); with sum2d one image per launch, so that every entry of the sum has one writer at a time
__global__ __launch_bounds__(256) void spectrum_cols_kernel(const SpColsArgs a) {
    __shared__ double sT[2 * kSpTile * kSpLd];          // Tr and Ti chunks as [v][i]; then the tile's weighted P at row stride 65
    __shared__ double sC[kSpMaxSide], sS[kSpMaxSide];
    static_assert(2 * kSpTile * kSpLd >= kSpTile * (kSpTile + 1), "the P tile must fit the staging buffers");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, Wh = a.Wh;
    const int u0 = (blockIdx.x / a.tv) * kSpTile, v0 = (blockIdx.x % a.tv) * kSpTile;
    const long long n = a.n0 + blockIdx.y;
    const double* T = a.T + n * H * 2 * Wh;
    for (int k = tid; k < H; k += 256) {
        sC[k] = a.ch[k];
        sS[k] = a.sh[k];
    }
    // staging: thread -> frequency sv of rows i = k0 + si + 4 e of T
    const int sv = tid & 63, si = tid >> 6;
    const bool vok = v0 + sv < Wh;
    double tr[8], ti[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = k0 + si + 4 * e;
            const bool ok = vok && i < H;
            tr[e] = ok ? T[(long long)i * 2 * Wh + v0 + sv] : 0.0;
            ti[e] = ok ? T[(long long)i * 2 * Wh + Wh + v0 + sv] : 0.0;
        }
    };
    double* sTr = sT;
    double* sTi = sT + kSpTile * kSpLd;
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int kg = 16 * (g & 1) + 8 * (g >> 1);
    const double* bTr = sTr + (wc + l15) * kSpLd + kg;
    const double* bTi = sTi + (wc + l15) * kSpLd + kg;
    f64x4_t accR[2][2], accI[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) accR[p][q] = accI[p][q] = f64x4_t{0.0, 0.0, 0.0, 0.0};
    SpTwiddle tw;
    fetch(0);
    for (int k0 = 0; k0 < H; k0 += kSpKC) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sTr[sv * kSpLd + si + 4 * e] = tr[e];
            sTi[sv * kSpLd + si + 4 * e] = ti[e];
        }
        __syncthreads();
        if (k0 + kSpKC < H) fetch(k0 + kSpKC);
        tw.start(u0 + wr + l15, u0 + wr + 16 + l15, k0 + kg, H);
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            const double c0 = sC[tw.at[0]], c1 = sC[tw.at[1]], s0 = sS[tw.at[0]], s1 = sS[tw.at[1]];
            tw.next(H);
            const double r0 = bTr[st], r1 = bTr[16 * kSpLd + st];
            const double i0 = bTi[st], i1 = bTi[16 * kSpLd + st];
            // Xr += c Tr + s Ti
            accR[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, r0, accR[0][0], 0, 0, 0);
            accR[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, r1, accR[0][1], 0, 0, 0);
            accR[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, r0, accR[1][0], 0, 0, 0);
            accR[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, r1, accR[1][1], 0, 0, 0);
            accR[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s0, i0, accR[0][0], 0, 0, 0);
            accR[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s0, i1, accR[0][1], 0, 0, 0);
            accR[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(s1, i0, accR[1][0], 0, 0, 0);
            accR[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(s1, i1, accR[1][1], 0, 0, 0);
            // Xi += c Ti - s Tr
            const double m0 = -s0, m1 = -s1;
            accI[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, i0, accI[0][0], 0, 0, 0);
            accI[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, i1, accI[0][1], 0, 0, 0);
            accI[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, i0, accI[1][0], 0, 0, 0);
            accI[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, i1, accI[1][1], 0, 0, 0);
            accI[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(m0, r0, accI[0][0], 0, 0, 0);
            accI[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(m0, r1, accI[0][1], 0, 0, 0);
            accI[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(m1, r0, accI[1][0], 0, 0, 0);
            accI[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(m1, r1, accI[1][1], 0, 0, 0);
        }
    }
    __syncthreads();             // every wave is done with the staged chunks: sT becomes the P tile
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wr + 16 * p + g + 4 * reg, col = wc + 16 * q + l15;
                const double xr = accR[p][q][reg], xi = accI[p][q][reg];
                const double rr = xr * xr, ii = xi * xi;
                const double pw = rr + ii;
                const int u = u0 + row, v = v0 + col;
                sT[row * (kSpTile + 1) + col] = (double)sp_weight(v, a.W) * pw;      // times 1 or 2: exact
                if (a.sum2d && u < H && v < Wh) a.sum2d[(long long)u * Wh + v] = a.sum2d[(long long)u * Wh + v] + pw;
            }
    __syncthreads();
    const SpTileOrder* o = a.order + blockIdx.x;
    if (tid < o->nb) {
        double s = 0.0;
        const int hi = o->seg[tid + 1];
        for (int e = o->seg[tid]; e < hi; ++e) {
            const int at = o->perm[e];
            s = s + sT[(at >> 6) * (kSpTile + 1) + (at & 63)];
        }
        a.partial[(n * a.tiles + blockIdx.x) * kSpTileBins + tid] = s;
    }
}

// grid (N): thread t takes bins t, t + 256, ..; tiles ascending
__global__ __launch_bounds__(256) void spectrum_fold_kernel(const double* partial, const SpTileOrder* order, int tiles, int K, double hw2,
                                                            double* prof) {
    const long long n = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += 256) {
        double s = 0.0;
        long long cnt = 0;
        for (int t = 0; t < tiles; ++t) {
            const int b = k - order[t].kmin;
            if (b >= 0 && b < order[t].nb) {
                s = s + partial[(n * tiles + t) * kSpTileBins + b];
                cnt += order[t].wcount[b];
            }
        }
        s = s / (double)cnt;
        prof[n * K + k] = s / hw2;
    }
}

// offsets in bytes of the pieces of the workspace; false for anything out of range
struct SpPlan {
    int Wh, tu, tv, tiles, K;
    size_t offT, offPartial, offOrder, bytes;
};

size_t sp_align(size_t v) { return (v + 255) & ~(size_t)255; }

bool sp_plan(int N, int H, int W, SpPlan* p) {
    if (N < 1 || N > kSpMaxN || H < 1 || W < 1 || H > kSpMaxSide || W > kSpMaxSide) return false;
    p->Wh = W / 2 + 1;
    p->tu = cdiv(H, kSpTile), p->tv = cdiv(p->Wh, kSpTile), p->tiles = p->tu * p->tv;
    p->K = sp_bins(H, W);
    size_t at = 0;
    p->offT = at, at = sp_align(at + (size_t)N * H * 2 * p->Wh * sizeof(double));
    p->offPartial = at, at = sp_align(at + (size_t)N * p->tiles * kSpTileBins * sizeof(double));
    p->offOrder = at, at = sp_align(at + (size_t)p->tiles * sizeof(SpTileOrder));
    p->bytes = at;
    return true;
}

bool sp_dtype(int dtype) { return dtype == WU_F32 || dtype == WU_BF16 || dtype == WU_SSIM_U8; }

template <class F> void sp_by_dtype(int dt, F f) {
    if (dt == WU_F32) f(std::integral_constant<int, WU_F32>());
    else if (dt == WU_BF16) f(std::integral_constant<int, WU_BF16>());
    else if (dt == WU_SSIM_U8) f(std::integral_constant<int, WU_SSIM_U8>());
    else f(std::integral_constant<int, kSpF64>());
}

// order tables, row stage, column stage (image by image when the running spectrum sum is wanted) and fold, all on stream s
int sp_launch(const SpSource& src, int dt, int N, const SpPlan& p, const double* cw, const double* sw, const double* ch, const double* sh,
              void* workspace, double* prof, double* sum2d, hipStream_t s) {
    char* ws = (char*)workspace;
    double* T = (double*)(ws + p.offT);
    double* partial = (double*)(ws + p.offPartial);
    SpTileOrder* order = (SpTileOrder*)(ws + p.offOrder);
    const int H = src.H, W = src.W;
    hipLaunchKernelGGL(spectrum_order_kernel, dim3(p.tiles), dim3(256), 0, s, H, W, p.Wh, p.tv, order);
    WU_LAUNCH_CHECK("spectrum_order_kernel");
    SpRowsArgs ra;
    ra.src = src;
    ra.rows = (long long)N * H;
    ra.Wh = p.Wh, ra.cw = cw, ra.sw = sw, ra.T = T;
    const dim3 rgrid((unsigned)((ra.rows + kSpTile - 1) / kSpTile), p.tv);
    sp_by_dtype(dt, [&](auto tag) {
        hipLaunchKernelGGL(spectrum_rows_kernel<decltype(tag)::value>, rgrid, dim3(256), 0, s, ra);
    });
    WU_LAUNCH_CHECK("spectrum_rows_kernel");
    SpColsArgs ca;
    ca.T = T, ca.H = H, ca.W = W, ca.Wh = p.Wh, ca.tv = p.tv, ca.tiles = p.tiles, ca.ch = ch, ca.sh = sh;
    ca.order = order, ca.partial = partial, ca.sum2d = sum2d, ca.n0 = 0;
    if (!sum2d) {
        hipLaunchKernelGGL(spectrum_cols_kernel, dim3(p.tiles, N), dim3(256), 0, s, ca);
        WU_LAUNCH_CHECK("spectrum_cols_kernel");
    } else {
        for (ca.n0 = 0; ca.n0 < N; ++ca.n0) {
            hipLaunchKernelGGL(spectrum_cols_kernel, dim3(p.tiles, 1), dim3(256), 0, s, ca);
            WU_LAUNCH_CHECK("spectrum_cols_kernel");
        }
    }
    const double hw = (double)((long long)H * W);
    hipLaunchKernelGGL(spectrum_fold_kernel, dim3(N), dim3(256), 0, s, (const double*)partial, (const SpTileOrder*)order, p.tiles, p.K,
                       hw * hw, prof);
    WU_LAUNCH_CHECK("spectrum_fold_kernel");
    return 0;
}

}  // namespace

extern "C" int wu_spectrum_bins(int H, int W) {
    return H >= 1 && W >= 1 && H <= kSpMaxSide && W <= kSpMaxSide ? sp_bins(H, W) : 0;
}

extern "C" size_t wu_spectrum_workspace_bytes(int N, int H, int W) {
    SpPlan p;
    return sp_plan(N, H, W, &p) ? p.bytes : 0;
}

extern "C" int wu_spectrum_luma(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int N, int C, int H,
                                int W, double scale, double shift, double L, const double* wh, const double* ww, double* planes,
                                void* stream) {
    SpPlan p;
    WU_REQUIRE(sp_plan(N, H, W, &p), "wu_spectrum_luma: N %d H %d W %d out of range (1 <= N <= %d, 1 <= H, W <= %d)", N, H, W, kSpMaxN,
               kSpMaxSide);
    WU_REQUIRE(C == 1 || C == 3, "wu_spectrum_luma: C %d must be 1 or 3", C);
    WU_REQUIRE(sp_dtype(dtype), "wu_spectrum_luma: unknown dtype %d", dtype);
    WU_REQUIRE(x && planes, "wu_spectrum_luma: NULL pointer");
    WU_REQUIRE(!wh == !ww, "wu_spectrum_luma: the window needs both tables or neither");
    SpSource src;
    src.x = x;
    src.xs[0] = xs_n, src.xs[1] = xs_c, src.xs[2] = xs_h, src.xs[3] = xs_w;
    src.C = C, src.H = H, src.W = W, src.scale = scale, src.shift = shift, src.L = L, src.wh = wh, src.ww = ww;
    const long long total = (long long)N * H * W;
    const dim3 grid((unsigned)((total + 255) / 256));
    sp_by_dtype(dtype, [&](auto tag) {
        hipLaunchKernelGGL(spectrum_luma_kernel<decltype(tag)::value>, grid, dim3(256), 0, (hipStream_t)stream, src, total, planes);
    });
    WU_LAUNCH_CHECK("spectrum_luma_kernel");
    return 0;
}

extern "C" int wu_spectrum_profiles_planes(const double* planes, int N, int H, int W, const double* cw, const double* sw, const double* ch,
                                           const double* sh, int K, void* workspace, double* prof, double* spectrum_sum, void* stream) {
    SpPlan p;
    WU_REQUIRE(sp_plan(N, H, W, &p), "wu_spectrum_profiles_planes: N %d H %d W %d out of range (1 <= N <= %d, 1 <= H, W <= %d)", N, H, W,
               kSpMaxN, kSpMaxSide);
    WU_REQUIRE(K == p.K, "wu_spectrum_profiles_planes: K %d, but %d x %d has %d radial bins", K, H, W, p.K);
    WU_REQUIRE(planes && cw && sw && ch && sh && workspace && prof, "wu_spectrum_profiles_planes: NULL pointer");
    SpSource src;
    src.x = planes;
    src.xs[0] = (long long)H * W, src.xs[1] = 0, src.xs[2] = W, src.xs[3] = 1;
    src.C = 1, src.H = H, src.W = W, src.scale = 1.0, src.shift = 0.0, src.L = 1.0, src.wh = nullptr, src.ww = nullptr;
    return sp_launch(src, kSpF64, N, p, cw, sw, ch, sh, workspace, prof, spectrum_sum, (hipStream_t)stream);
}

extern "C" int wu_spectrum_profiles(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int N, int C,
                                    int H, int W, double scale, double shift, double L, const double* wh, const double* ww,
                                    const double* cw, const double* sw, const double* ch, const double* sh, int K, void* workspace,
                                    double* prof, double* spectrum_sum, void* stream) {
    SpPlan p;
    WU_REQUIRE(sp_plan(N, H, W, &p), "wu_spectrum_profiles: N %d H %d W %d out of range (1 <= N <= %d, 1 <= H, W <= %d)", N, H, W, kSpMaxN,
               kSpMaxSide);
    WU_REQUIRE(C == 1 || C == 3, "wu_spectrum_profiles: C %d must be 1 or 3", C);
    WU_REQUIRE(sp_dtype(dtype), "wu_spectrum_profiles: unknown dtype %d", dtype);
    WU_REQUIRE(K == p.K, "wu_spectrum_profiles: K %d, but %d x %d has %d radial bins", K, H, W, p.K);
    WU_REQUIRE(x && cw && sw && ch && sh && workspace && prof, "wu_spectrum_profiles: NULL pointer");
    WU_REQUIRE(!wh == !ww, "wu_spectrum_profiles: the window needs both tables or neither");
    SpSource src;
    src.x = x;
    src.xs[0] = xs_n, src.xs[1] = xs_c, src.xs[2] = xs_h, src.xs[3] = xs_w;
    src.C = C, src.H = H, src.W = W, src.scale = scale, src.shift = shift, src.L = L, src.wh = wh, src.ww = ww;
    return sp_launch(src, dtype, N, p, cw, sw, ch, sh, workspace, prof, spectrum_sum, (hipStream_t)stream);
}
