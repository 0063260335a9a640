// Fast colour guided filter (He, Sun, Tang 2013; He, Sun 2015) as a joint upsampler: a local affine model q = A I + b from the network's
// low-resolution input I (N, 3, hl, wl) to its R low-resolution outputs p (R, N, 3, hl, wl), applied to the full-resolution photograph.
// All arithmetic in fp64, every operation rounded on its own, in the order tests/_guided_ref.py restates; no atomics, no reductions across
// threads: the same inputs give the same bits, and a row's numbers do not depend on R.
//   Stage A, wu_guided_coeffs: SIX launches whatever N and R (FIVE for r <= 8, where 5 and 6 are one tiled launch).  box() is separable in the stated order (row sums left to right,
//   then the rows of row sums top to bottom, then ONE division by count_y * count_x), every output value formed by one thread:
//     1 guided_hsum_guide   row sums of I_k (3) and I_j I_k (6, j <= k)                                   -> workspace H1 (N, 9, hl, wl)
//     2 guided_vsum_guide   their column sums, mI, Sigma + eps, the inverse by cofactors                  -> workspace G  (N, 9, hl, wl)
//     3 guided_hsum_rows    row sums of p_c (3) and I_k p_c (9)                                           -> workspace H2 (R, N, 12, hl, wl)
//     4 guided_vsum_rows    their column sums, cov, a = Sigma^-1 cov, b                                   -> the OUTPUT buffer (a, b unsmoothed)
//     5 guided_hsum_maps    row sums of the 12 a / b maps                                                 -> H2 again
//     6 guided_vsum_maps    column sums and the division                                                  -> the output (R, N, 12, hl, wl)
//     5 + 6 for r <= 8: guided_box_tile_kernel, a 32 x 32 tile of one map with its halo in LDS (the buffers of 3 and 4 then trade places)
//   The guide's moments and the inverse (1, 2) are formed once per image and read by all R rows.
//   Stage B, wu_guided_apply: ONE launch.  A workgroup owns an 8 x 64 tile of one photograph: each thread reads its two pixels once and forms
//   their tap positions and weights once, then the R rows are walked: the rows' 12 x (patch) low-resolution coefficients go to LDS, every pixel
//   interpolates its 12 coefficients from there and writes its three bytes (or floats).  No full-resolution coefficient map reaches memory.
//   A small patch (at most 341 entries: upscaling by 5 / 3 or more) is requested a row ahead and waits in registers while the current row is
//   computed -- in launches whose patches have at least kGuidedPreMin entries; below that the launcher takes the kernel without those
//   registers.  A patch larger than kGuidedPatch entries (strong downscaling, h << hl) is read from global memory instead of LDS: same
//   arithmetic, same bits.
#include "wu_common.h"

// every product, sum and quotient is rounded on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kGuidedTH = 8, kGuidedTW = 64;         // apply tile: 256 threads, two pixels each (rows t and t + 4 of one column)
constexpr int kGuidedPatch = 640;                    // low-resolution entries per map in LDS: 12 x 640 x 8 B = 60 KiB, two workgroups per CU;
                                                     // a tile at ratio hl / h <= 1 needs at most 9 x 65 = 585
constexpr int kGuidedPre = 16;                       // coefficients a thread holds in flight for the next row (see the kernel)
constexpr int kGuidedPreMin = 32;                    // ... in launches whose largest tile patch has at least this many entries
constexpr int kGuidedMaxDim = 1 << 15;
constexpr int kGuidedBoxT = 32, kGuidedBoxR = 8;     // the tiled smoothing of the coefficient maps: 32 x 32 outputs, radius up to 8
constexpr int kGuidedBoxHalo = kGuidedBoxT + 2 * kGuidedBoxR;       // 48: 18 KiB of halo + 12 KiB of row sums
constexpr int kGuidedFillGroups = 1024;              // workgroups that fill the device (see ssim.hip)

template <int DT> __device__ __forceinline__ double guided_load(const void* p, long long at, double scale, double shift) {
    double v = DT == WU_BF16 ? (double)bf16_to_f32(((const bf16_t*)p)[at]) : (double)((const float*)p)[at];
    v = v * scale;
    return v + shift;
}

struct GuidedCoefArgs {
    const float* guide;          // element strides (n, c, h, w)
    const void* targets;         // element strides (r, n, c, h, w)
    long long gs[4], ts[5];
    int N, R, hl, wl, r;
    double g_scale, g_shift, t_scale, t_shift, eps;
    double* H1;                  // (N, 9, hl, wl)
    double* G;                   // (N, 9, hl, wl): mI (3), inverse (00, 01, 02, 11, 12, 22)
    double* H2;                  // (R, N, 12, hl, wl)
    double* out;                 // (R, N, 12, hl, wl)
};

// 1: one thread per (n, y, x)
__global__ __launch_bounds__(256) void guided_hsum_guide(const GuidedCoefArgs a) {
    const long long hw = (long long)a.hl * a.wl, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.N * hw) return;
    const int n = (int)(idx / hw), y = (int)((idx % hw) / a.wl), x = (int)(idx % a.wl);
    const int x0 = max(0, x - a.r), x1 = min(a.wl - 1, x + a.r);
    const long long base = n * a.gs[0] + y * a.gs[2];
    double s[9];
    for (int t = x0; t <= x1; ++t) {
        double I[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) I[k] = guided_load<WU_F32>(a.guide, base + k * a.gs[1] + t * a.gs[3], a.g_scale, a.g_shift);
        const double v[9] = {I[0], I[1], I[2], I[0] * I[0], I[0] * I[1], I[0] * I[2], I[1] * I[1], I[1] * I[2], I[2] * I[2]};
#pragma unroll
        for (int m = 0; m < 9; ++m) s[m] = t == x0 ? v[m] : s[m] + v[m];
    }
    double* o = a.H1 + (long long)n * 9 * hw + (long long)y * a.wl + x;
#pragma unroll
    for (int m = 0; m < 9; ++m) o[m * hw] = s[m];
}

// 2: one thread per (n, y, x)
__global__ __launch_bounds__(256) void guided_vsum_guide(const GuidedCoefArgs a) {
    const long long hw = (long long)a.hl * a.wl, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.N * hw) return;
    const int n = (int)(idx / hw), y = (int)((idx % hw) / a.wl), x = (int)(idx % a.wl);
    const int x0 = max(0, x - a.r), x1 = min(a.wl - 1, x + a.r);
    const int y0 = max(0, y - a.r), y1 = min(a.hl - 1, y + a.r);
    const double cnt = (double)((long long)(y1 - y0 + 1) * (x1 - x0 + 1));
    const double* in = a.H1 + (long long)n * 9 * hw + x;
    double s[9];
    for (int t = y0; t <= y1; ++t) {
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            const double v = in[m * hw + (long long)t * a.wl];
            s[m] = t == y0 ? v : s[m] + v;
        }
    }
#pragma unroll
    for (int m = 0; m < 9; ++m) s[m] = s[m] / cnt;
    const double m0 = s[0], m1 = s[1], m2 = s[2];
    const double A = (s[3] - m0 * m0) + a.eps, B = s[4] - m0 * m1, C = s[5] - m0 * m2;
    const double D = (s[6] - m1 * m1) + a.eps, E = s[7] - m1 * m2, F = (s[8] - m2 * m2) + a.eps;
    const double c00 = D * F - E * E, c01 = C * E - B * F, c02 = B * E - C * D;
    const double c11 = A * F - C * C, c12 = B * C - A * E, c22 = A * D - B * B;
    const double det = (A * c00 + B * c01) + C * c02;
    double* o = a.G + (long long)n * 9 * hw + (long long)y * a.wl + x;
    o[0] = m0, o[hw] = m1, o[2 * hw] = m2;
    o[3 * hw] = c00 / det, o[4 * hw] = c01 / det, o[5 * hw] = c02 / det;
    o[6 * hw] = c11 / det, o[7 * hw] = c12 / det, o[8 * hw] = c22 / det;
}

// 3: one thread per (r, n, y, x): p_c at map c, I_k p_c at map 3 + 3 c + k
template <int DT> __global__ __launch_bounds__(256) void guided_hsum_rows(const GuidedCoefArgs a) {
    const long long hw = (long long)a.hl * a.wl, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.R * a.N * hw) return;
    const long long rn = idx / hw;
    const int n = (int)(rn % a.N), r = (int)(rn / a.N), y = (int)((idx % hw) / a.wl), x = (int)(idx % a.wl);
    const int x0 = max(0, x - a.r), x1 = min(a.wl - 1, x + a.r);
    const long long gbase = n * a.gs[0] + y * a.gs[2], tbase = r * a.ts[0] + n * a.ts[1] + y * a.ts[3];
    double s[12];
    for (int t = x0; t <= x1; ++t) {
        double I[3], p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            I[k] = guided_load<WU_F32>(a.guide, gbase + k * a.gs[1] + t * a.gs[3], a.g_scale, a.g_shift);
            p[k] = guided_load<DT>(a.targets, tbase + k * a.ts[2] + t * a.ts[4], a.t_scale, a.t_shift);
        }
        double v[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = p[c];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[3 + 3 * c + k] = I[k] * p[c];
        }
#pragma unroll
        for (int m = 0; m < 12; ++m) s[m] = t == x0 ? v[m] : s[m] + v[m];
    }
    double* o = a.H2 + rn * 12 * hw + (long long)y * a.wl + x;
#pragma unroll
    for (int m = 0; m < 12; ++m) o[m * hw] = s[m];
}

// 4: one thread per (r, n, y, x): a_ck at map 3 c + k, b_c at map 9 + c
__global__ __launch_bounds__(256) void guided_vsum_rows(const GuidedCoefArgs a) {
    const long long hw = (long long)a.hl * a.wl, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.R * a.N * hw) return;
    const long long rn = idx / hw;
    const int n = (int)(rn % a.N), y = (int)((idx % hw) / a.wl), x = (int)(idx % a.wl);
    const int x0 = max(0, x - a.r), x1 = min(a.wl - 1, x + a.r);
    const int y0 = max(0, y - a.r), y1 = min(a.hl - 1, y + a.r);
    const double cnt = (double)((long long)(y1 - y0 + 1) * (x1 - x0 + 1));
    const double* in = a.H2 + rn * 12 * hw + x;
    double s[12];
    for (int t = y0; t <= y1; ++t) {
#pragma unroll
        for (int m = 0; m < 12; ++m) {
            const double v = in[m * hw + (long long)t * a.wl];
            s[m] = t == y0 ? v : s[m] + v;
        }
    }
#pragma unroll
    for (int m = 0; m < 12; ++m) s[m] = s[m] / cnt;
    const double* g = a.G + (long long)n * 9 * hw + (long long)y * a.wl + x;
    const double mI[3] = {g[0], g[hw], g[2 * hw]};
    const double i00 = g[3 * hw], i01 = g[4 * hw], i02 = g[5 * hw], i11 = g[6 * hw], i12 = g[7 * hw], i22 = g[8 * hw];
    const double inv[3][3] = {{i00, i01, i02}, {i01, i11, i12}, {i02, i12, i22}};
    double* o = a.out + rn * 12 * hw + (long long)y * a.wl + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double bp = s[c];
        double cov[3], ac[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cov[k] = s[3 + 3 * c + k] - mI[k] * bp;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ac[k] = (inv[k][0] * cov[0] + inv[k][1] * cov[1]) + inv[k][2] * cov[2];
            o[(3 * c + k) * hw] = ac[k];
        }
        o[(9 + c) * hw] = bp - ((ac[0] * mI[0] + ac[1] * mI[1]) + ac[2] * mI[2]);
    }
}

// 5: one thread per value of `maps` hl x wl maps
__global__ __launch_bounds__(256) void guided_hsum_maps(const double* in, double* out, long long maps, int hl, int wl, int r) {
    const long long hw = (long long)hl * wl, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= maps * hw) return;
    const int x = (int)(idx % wl);
    const int x0 = max(0, x - r), x1 = min(wl - 1, x + r);
    const double* p = in + (idx - x);
    double s = p[x0];
    for (int t = x0 + 1; t <= x1; ++t) s = s + p[t];
    out[idx] = s;
}
// 6: one thread per value
__global__ __launch_bounds__(256) void guided_vsum_maps(const double* in, double* out, long long maps, int hl, int wl, int r) {
    const long long hw = (long long)hl * wl, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= maps * hw) return;
    const int x = (int)(idx % wl), y = (int)((idx % hw) / wl);
    const int y0 = max(0, y - r), y1 = min(hl - 1, y + r);
    const int x0 = max(0, x - r), x1 = min(wl - 1, x + r);
    const double cnt = (double)((long long)(y1 - y0 + 1) * (x1 - x0 + 1));
    const double* p = in + (idx - (long long)y * wl);
    double s = p[(long long)y0 * wl];
    for (int t = y0 + 1; t <= y1; ++t) s = s + p[(long long)t * wl];
    out[idx] = s / cnt;
}

// 5 + 6 in one launch for r <= kGuidedBoxR: a workgroup owns a 32 x 32 tile of one map.  Its (32 + 2r)^2 halo goes to LDS, the row pass
// leaves (32 + 2r) x 32 row sums in LDS, the column pass writes the means -- every value from its own in-range taps in the stated order, so
// the bits are those of the two kernels above; what is saved is their round trip through memory and the 2r + 1 reads per output from L2.
// grid (maps * tiles): the tile fastest.  A half-wave reads 32 consecutive doubles in both passes: no bank conflict.
__global__ __launch_bounds__(256) void guided_box_tile_kernel(const double* in, double* out, int tiles_x, int tiles_y, int hl, int wl, int r) {
    __shared__ double sIn[kGuidedBoxHalo * kGuidedBoxHalo];
    __shared__ double sH[kGuidedBoxHalo * kGuidedBoxT];
    const int tid = threadIdx.x;
    const int ntiles = tiles_x * tiles_y;
    const long long map = blockIdx.x / ntiles;
    const int tile = blockIdx.x % ntiles, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int oy0 = ty * kGuidedBoxT, ox0 = tx * kGuidedBoxT;
    const int WH = kGuidedBoxT + 2 * r;                             // halo rows and columns
    const double* p = in + map * hl * wl;
    for (int e = tid; e < WH * WH; e += 256) {
        const int i = e / WH, j = e - i * WH;
        const int gy = oy0 - r + i, gx = ox0 - r + j;
        sIn[e] = gy >= 0 && gy < hl && gx >= 0 && gx < wl ? p[(long long)gy * wl + gx] : 0.0;      // outside: never a tap
    }
    __syncthreads();
    for (int e = tid; e < WH * kGuidedBoxT; e += 256) {
        const int i = e >> 5, j = e & 31;
        const int x = ox0 + j;
        double sum = 0.0;
        if (x < wl) {
            const int x0 = max(0, x - r), x1 = min(wl - 1, x + r);
            const double* row = sIn + i * WH - (ox0 - r);          // row[gx]
            sum = row[x0];
            for (int t = x0 + 1; t <= x1; ++t) sum = sum + row[t];
        }
        sH[e] = sum;
    }
    __syncthreads();
    const int j = tid & 31, x = ox0 + j;
    if (x >= wl) return;
    const int x0 = max(0, x - r), x1 = min(wl - 1, x + r);
    for (int i = tid >> 5; i < kGuidedBoxT; i += 8) {
        const int y = oy0 + i;
        if (y >= hl) break;
        const int y0 = max(0, y - r), y1 = min(hl - 1, y + r);
        const double cnt = (double)((long long)(y1 - y0 + 1) * (x1 - x0 + 1));
        const double* col = sH + j - (oy0 - r) * kGuidedBoxT;      // col[gy * 32]
        double sum = col[y0 * kGuidedBoxT];
        for (int t = y0 + 1; t <= y1; ++t) sum = sum + col[t * kGuidedBoxT];
        out[map * hl * wl + (long long)y * wl + x] = sum / cnt;
    }
}

// ---- stage B ---------------------------------------------------------------------------------------------------------------------------------
struct GuidedApplyArgs {
    const double* coeffs;        // (R, N, 12, hl, wl)
    const unsigned char* photos; // (N, Hmax, Wmax, 3)
    const int* sizes;            // (N, 2) on the device: h, w
    unsigned char* out_u8;       // (R, N, Hmax, Wmax, 3) or NULL
    float* out_f32;              // (R, N, 3, Hmax, Wmax) or NULL
    int N, R, hl, wl, Hmax, Wmax;
    int tiles_x, tiles_y, rows_per_group;
};

// the two taps and the weight of full-resolution coordinate P on a low-resolution axis of nl samples: v = (P + 0.5) ratio - 0.5 clamped
__device__ __forceinline__ void guided_tap(int P, double ratio, int nl, int& i0, int& i1, double& f) {
    double v = ((double)P + 0.5) * ratio;
    v = v - 0.5;
    const double top = (double)(nl - 1);
    v = v < 0.0 ? 0.0 : v;
    v = v > top ? top : v;
    i0 = (int)floor(v);
    i1 = min(i0 + 1, nl - 1);
    f = v - (double)i0;
}

// one pixel of one row from maps at `c` (map stride ms, row stride rs), the taps as offsets into a map
template <bool U8> __device__ __forceinline__ void guided_pixel(const double* c, long long ms, long long o00, long long o01, long long o10,
                                                                long long o11, double fx, double fy, const double* I, const GuidedApplyArgs& a,
                                                                long long rn, int Y, int X) {
    double q[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) {
        const double* p = c + m * ms;
        const double v00 = p[o00], v01 = p[o01], v10 = p[o10], v11 = p[o11];
        const double top = v00 + (v01 - v00) * fx, bot = v10 + (v11 - v10) * fx;
        q[m] = top + (bot - top) * fy;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double v = ((q[3 * ch] * I[0] + q[3 * ch + 1] * I[1]) + q[3 * ch + 2] * I[2]) + q[9 + ch];
        if (U8) {
            double t = v * 255.0;
            t = t > 0.0 ? t : 0.0;              // NaN -> 0 as well
            t = t < 255.0 ? t : 255.0;
            a.out_u8[((rn * a.Hmax + Y) * a.Wmax + X) * 3 + ch] = (unsigned char)(int)t;
        } else {
            a.out_f32[((rn * 3 + ch) * a.Hmax + Y) * a.Wmax + X] = (float)v;
        }
    }
}

// grid (tiles_x * tiles_y * N, row groups): the tile fastest
template <bool U8, int PRE> __global__ __launch_bounds__(256) void guided_apply_kernel(const GuidedApplyArgs a) {
    __shared__ double sC[12 * kGuidedPatch];
    const int tid = threadIdx.x;
    const int ntiles = a.tiles_x * a.tiles_y;
    const int tile = blockIdx.x % ntiles, n = blockIdx.x / ntiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int Y0 = ty * kGuidedTH, X0 = tx * kGuidedTW;
    const int h = a.sizes[2 * n], w = a.sizes[2 * n + 1];
    if (Y0 >= h || X0 >= w) return;                                  // the whole workgroup: padding is not written
    const int r_lo = blockIdx.y * a.rows_per_group, r_hi = min(a.R, r_lo + a.rows_per_group);
    const double ry = (double)a.hl / (double)h, rx = (double)a.wl / (double)w;

    // the low-resolution patch of the tile: first tap of its first pixel .. second tap of its last pixel inside the image (taps are monotone)
    int py0, py1, px0, px1, dummy;
    double fdummy;
    guided_tap(Y0, ry, a.hl, py0, dummy, fdummy);
    guided_tap(min(Y0 + kGuidedTH, h) - 1, ry, a.hl, dummy, py1, fdummy);
    guided_tap(X0, rx, a.wl, px0, dummy, fdummy);
    guided_tap(min(X0 + kGuidedTW, w) - 1, rx, a.wl, dummy, px1, fdummy);
    const int ph = py1 - py0 + 1, pw = px1 - px0 + 1;
    const long long npatch = (long long)ph * pw;
    const bool lds = npatch <= kGuidedPatch;

    // the thread's two pixels: column X, rows Ya and Ya + 4
    const int X = X0 + (tid & 63), Ya = Y0 + (tid >> 6);
    const bool in_x = X < w;
    bool live[2];
    double I[2][3], fy[2], fx = 0.0;
    int x0 = 0, x1 = 0, y0[2], y1[2];
    if (in_x) guided_tap(X, rx, a.wl, x0, x1, fx);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int Y = Ya + 4 * u;
        live[u] = in_x && Y < h;
        y0[u] = y1[u] = 0;
        fy[u] = 0.0;
        if (live[u]) {
            guided_tap(Y, ry, a.hl, y0[u], y1[u], fy[u]);
            const unsigned char* px = a.photos + (((long long)n * a.Hmax + Y) * a.Wmax + X) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) I[u][k] = (double)px[k] / 255.0;
        }
    }
    const long long hw = (long long)a.hl * a.wl;
    // PRE > 0: a patch of at most 256 PRE / 12 entries (341: every upscaling by 5 / 3 or more) is requested one row AHEAD and waits in
    // registers while the current row is computed, so the loads' latency is not on the path between two barriers; the element offsets
    // are formed once.  PRE = 0 is the kernel without those registers: the launcher takes it where the patches are a few entries only.
    constexpr int kPre = PRE > 0 ? PRE : 1;
    const bool ahead = PRE > 0 && 12 * npatch <= 256 * PRE;
    const int nper = (12 * (int)(ahead ? npatch : 0) + 255) / 256;   // elements per thread, at most: the same for the whole workgroup
    long long off[kPre];
    double pre[kPre];
    if (ahead) {
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const int e = tid + 256 * u;
            off[u] = -1;
            if (u < nper && e < 12 * (int)npatch) {
                const int m = e / (int)npatch, rem = e - m * (int)npatch;
                const int iy = rem / pw, ix = rem - iy * pw;
                off[u] = m * hw + (long long)(py0 + iy) * a.wl + (px0 + ix);
            }
        }
        const double* c0 = a.coeffs + ((long long)r_lo * a.N + n) * 12 * hw;
#pragma unroll
        for (int u = 0; u < kPre; ++u)
            if (u < nper && off[u] >= 0) pre[u] = c0[off[u]];
    }
    for (int r = r_lo; r < r_hi; ++r) {
        const long long rn = (long long)r * a.N + n;
        const double* c = a.coeffs + rn * 12 * hw;
        if (lds) {
            __syncthreads();                                         // the row before is read
            if (ahead) {
#pragma unroll
                for (int u = 0; u < kPre; ++u)
                    if (u < nper && off[u] >= 0) sC[tid + 256 * u] = pre[u];
                if (r + 1 < r_hi) {
                    const double* cn = c + (long long)a.N * 12 * hw;
#pragma unroll
                    for (int u = 0; u < kPre; ++u)
                        if (u < nper && off[u] >= 0) pre[u] = cn[off[u]];
                }
            } else {
                for (int e = tid; e < 12 * (int)npatch; e += 256) {
                    const int m = e / (int)npatch, rem = e - m * (int)npatch;
                    const int iy = rem / pw, ix = rem - iy * pw;
                    sC[e] = c[m * hw + (long long)(py0 + iy) * a.wl + (px0 + ix)];
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (live[u]) {
                    const int ra = (y0[u] - py0) * pw, rb = (y1[u] - py0) * pw, ca = x0 - px0, cb = x1 - px0;
                    guided_pixel<U8>(sC, npatch, ra + ca, ra + cb, rb + ca, rb + cb, fx, fy[u], I[u], a, rn, Ya + 4 * u, X);
                }
        } else {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (live[u]) {
                    const long long ra = (long long)y0[u] * a.wl, rb = (long long)y1[u] * a.wl;
                    guided_pixel<U8>(c, hw, ra + x0, ra + x1, rb + x0, rb + x1, fx, fy[u], I[u], a, rn, Ya + 4 * u, X);
                }
        }
    }
}

bool guided_coef_range(int N, int R, int hl, int wl) {
    if (N < 1 || R < 1 || hl < 1 || wl < 1 || hl > kGuidedMaxDim || wl > kGuidedMaxDim) return false;
    if ((long long)N * R > (1 << 24)) return false;
    // the largest grid: one thread per value of the R N 12 maps
    return ((long long)R * N * 12 * hl * wl + 255) / 256 < (1ll << 31);
}

}  // namespace

extern "C" int wu_guided_tile_h(void) { return kGuidedTH; }
extern "C" int wu_guided_tile_w(void) { return kGuidedTW; }

extern "C" size_t wu_guided_workspace_bytes(int N, int R, int hl, int wl) {
    if (!guided_coef_range(N, R, hl, wl)) return 0;
    return ((size_t)N * 18 + (size_t)R * N * 12) * hl * wl * sizeof(double);
}

extern "C" int wu_guided_coeffs(const float* guide, long long gs_n, long long gs_c, long long gs_h, long long gs_w, double g_scale,
                                double g_shift, const void* targets, long long ts_r, long long ts_n, long long ts_c, long long ts_h,
                                long long ts_w, int t_dtype, double t_scale, double t_shift, int N, int R, int hl, int wl, int r, double eps,
                                void* workspace, double* coeffs, void* stream) {
    WU_REQUIRE(r >= 0, "wu_guided_coeffs: radius r %d must not be negative", r);
    WU_REQUIRE(eps > 0.0, "wu_guided_coeffs: eps %g must be positive", eps);
    WU_REQUIRE(N >= 1 && R >= 1 && hl >= 1 && wl >= 1, "wu_guided_coeffs: N %d / R %d / hl %d / wl %d must be at least 1", N, R, hl, wl);
    WU_REQUIRE(t_dtype == WU_F32 || t_dtype == WU_BF16, "wu_guided_coeffs: unknown dtype %d", t_dtype);
    WU_REQUIRE(guide && targets && workspace && coeffs, "wu_guided_coeffs: NULL pointer");
    WU_REQUIRE(guided_coef_range(N, R, hl, wl), "wu_guided_coeffs: N %d R %d hl %d wl %d out of range", N, R, hl, wl);
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)hl * wl;
    GuidedCoefArgs a;
    a.guide = guide, a.targets = targets;
    a.gs[0] = gs_n, a.gs[1] = gs_c, a.gs[2] = gs_h, a.gs[3] = gs_w;
    a.ts[0] = ts_r, a.ts[1] = ts_n, a.ts[2] = ts_c, a.ts[3] = ts_h, a.ts[4] = ts_w;
    a.N = N, a.R = R, a.hl = hl, a.wl = wl;
    a.r = r < (hl > wl ? hl : wl) ? r : (hl > wl ? hl : wl);      // a window beyond the image is the whole image: the same taps
    a.g_scale = g_scale, a.g_shift = g_shift, a.t_scale = t_scale, a.t_shift = t_shift, a.eps = eps;
    a.H1 = (double*)workspace;
    a.G = a.H1 + (size_t)N * 9 * hw;
    // r <= kGuidedBoxR: passes 5 and 6 are one tiled launch, which cannot work in place: 3 then writes into the output buffer, 4 into the
    // workspace, and the tiled launch from there into the output.  Otherwise 3 -> workspace, 4 -> output, 5 -> workspace, 6 -> output.
    double* rows_ws = a.G + (size_t)N * 9 * hw;
    const long long box_tiles = (long long)cdiv(hl, kGuidedBoxT) * cdiv(wl, kGuidedBoxT);
    const bool tiled = a.r <= kGuidedBoxR && (long long)R * N * 12 * box_tiles < (1ll << 31);
    a.H2 = tiled ? coeffs : rows_ws;
    a.out = tiled ? rows_ws : coeffs;
    const unsigned g1 = (unsigned)(((size_t)N * hw + 255) / 256), g2 = (unsigned)(((size_t)R * N * hw + 255) / 256);
    const unsigned g3 = (unsigned)(((size_t)R * N * 12 * hw + 255) / 256);
    hipLaunchKernelGGL(guided_hsum_guide, dim3(g1), dim3(256), 0, s, a);
    WU_LAUNCH_CHECK("guided_hsum_guide");
    hipLaunchKernelGGL(guided_vsum_guide, dim3(g1), dim3(256), 0, s, a);
    WU_LAUNCH_CHECK("guided_vsum_guide");
    if (t_dtype == WU_F32) hipLaunchKernelGGL(guided_hsum_rows<WU_F32>, dim3(g2), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(guided_hsum_rows<WU_BF16>, dim3(g2), dim3(256), 0, s, a);
    WU_LAUNCH_CHECK("guided_hsum_rows");
    hipLaunchKernelGGL(guided_vsum_rows, dim3(g2), dim3(256), 0, s, a);
    WU_LAUNCH_CHECK("guided_vsum_rows");
    if (tiled) {
        hipLaunchKernelGGL(guided_box_tile_kernel, dim3((unsigned)((long long)R * N * 12 * box_tiles)), dim3(256), 0, s, (const double*)rows_ws,
                           coeffs, cdiv(wl, kGuidedBoxT), cdiv(hl, kGuidedBoxT), hl, wl, a.r);
        WU_LAUNCH_CHECK("guided_box_tile_kernel");
        return 0;
    }
    hipLaunchKernelGGL(guided_hsum_maps, dim3(g3), dim3(256), 0, s, (const double*)coeffs, rows_ws, (long long)R * N * 12, hl, wl, a.r);
    WU_LAUNCH_CHECK("guided_hsum_maps");
    hipLaunchKernelGGL(guided_vsum_maps, dim3(g3), dim3(256), 0, s, (const double*)rows_ws, coeffs, (long long)R * N * 12, hl, wl, a.r);
    WU_LAUNCH_CHECK("guided_vsum_maps");
    return 0;
}

extern "C" int wu_guided_apply(const double* coeffs, int N, int R, int hl, int wl, const unsigned char* photos, int Hmax, int Wmax,
                               const int* sizes_host, const int* sizes_dev, unsigned char* out_u8, float* out_f32, void* stream) {
    WU_REQUIRE(N >= 1 && R >= 1 && hl >= 1 && wl >= 1 && Hmax >= 1 && Wmax >= 1,
               "wu_guided_apply: N %d / R %d / hl %d / wl %d / Hmax %d / Wmax %d must be at least 1", N, R, hl, wl, Hmax, Wmax);
    WU_REQUIRE(coeffs && photos && sizes_host && sizes_dev, "wu_guided_apply: NULL pointer");
    WU_REQUIRE((out_u8 != nullptr) != (out_f32 != nullptr), "wu_guided_apply: exactly one of out_u8 and out_f32 (a NULL pointer for the other)");
    WU_REQUIRE(guided_coef_range(N, R, hl, wl) && Hmax <= kGuidedMaxDim && Wmax <= kGuidedMaxDim,
               "wu_guided_apply: N %d R %d hl %d wl %d Hmax %d Wmax %d out of range", N, R, hl, wl, Hmax, Wmax);
    for (int n = 0; n < N; ++n) {
        const int h = sizes_host[2 * n], w = sizes_host[2 * n + 1];
        WU_REQUIRE(h >= 1 && w >= 1, "wu_guided_apply: image %d has a zero size %d x %d", n, h, w);
        WU_REQUIRE(h <= Hmax && w <= Wmax, "wu_guided_apply: image %d is %d x %d, beyond the batch's Hmax %d x Wmax %d", n, h, w, Hmax, Wmax);
    }
    GuidedApplyArgs a;
    a.coeffs = coeffs, a.photos = photos, a.sizes = sizes_dev, a.out_u8 = out_u8, a.out_f32 = out_f32;
    a.N = N, a.R = R, a.hl = hl, a.wl = wl, a.Hmax = Hmax, a.Wmax = Wmax;
    a.tiles_x = cdiv(Wmax, kGuidedTW), a.tiles_y = cdiv(Hmax, kGuidedTH);
    const long long per_group = (long long)a.tiles_x * a.tiles_y * N;
    WU_REQUIRE(per_group < (1ll << 31), "wu_guided_apply: %lld tiles exceed the grid", per_group);
    // too few tiles to fill the device: split the rows over workgroups (a row's numbers do not depend on the split)
    const int want = per_group < kGuidedFillGroups ? (int)((kGuidedFillGroups + per_group - 1) / per_group) : 1;
    a.rows_per_group = cdiv(R, want < R ? want : R);
    const dim3 grid((unsigned)per_group, (unsigned)cdiv(R, a.rows_per_group));
    WU_REQUIRE(grid.y <= 65535u, "wu_guided_apply: R %d rows exceed the grid", R);
    // The low-resolution patch of a full tile, at most, over the batch.  Measured (profiles/guided_bench.md): requesting a row ahead halves
    // the time at 64 and 180 entries and costs 7 - 27 % at 18, where its registers are taken from the batching of the LDS reads.
    int patch = 0;
    for (int n = 0; n < N; ++n) {
        const long long ph = (long long)kGuidedTH * hl / sizes_host[2 * n] + 2, pw = (long long)kGuidedTW * wl / sizes_host[2 * n + 1] + 2;
        const int e = (int)(ph < hl ? ph : hl) * (int)(pw < wl ? pw : wl);
        patch = e > patch ? e : patch;
    }
    hipStream_t s = (hipStream_t)stream;
    if (patch >= kGuidedPreMin) {
        if (out_u8) hipLaunchKernelGGL((guided_apply_kernel<true, kGuidedPre>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((guided_apply_kernel<false, kGuidedPre>), grid, dim3(256), 0, s, a);
    } else {
        if (out_u8) hipLaunchKernelGGL((guided_apply_kernel<true, 0>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((guided_apply_kernel<false, 0>), grid, dim3(256), 0, s, a);
    }
    WU_LAUNCH_CHECK("guided_apply_kernel");
    return 0;
}
