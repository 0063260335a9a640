// Paired content preservation: SSIM / MS-SSIM means and squared / absolute error sums of an input batch x (B, C, H, W) against R conditioned
// outputs y (R, B, C, H, W), all in fp64 (tests/_ssim_ref.py states the arithmetic), at most 2 * levels launches per call.
//   * ssim_pool_kernel    one level's x (per n) and y (per r, n) images -> the next level's, a 2 x 2 mean with a zero row / column in front of
//                         an odd dimension; the pooled fp64 pyramids live in the workspace;
//   * ssim_tile_kernel    a workgroup owns a 32 x 32 output tile of one (n, c): the halo tile of x, mu_x and F(x x) are formed ONCE, then the
//                         R rows are walked: halo of y, column pass of y / y y / x y, row pass, the ssim and cs entries, their sums over the
//                         tile -- no filtered map reaches global memory (the optional level-0 ssim map does); level 0 also sums (x - y)^2 and
//                         |x - y| over the pixels the tile owns.  A row's y values are requested while the row before it is filtered; where
//                         B C tiles is too small to fill the device the rows are split over several workgroups instead of walked by one;
//   * ssim_finish_kernel  one wave per (r, n): the per-wave partial sums of the tiles in a fixed order, the means, the error sums over
//                         channels and tiles.
// LDS.  Halo tile and column-pass result share one row width WH = 32 + k - 1 and are stored without padding; a thread's element index e runs
// over rows, so the 32 lanes of a half-wave always read 32 CONSECUTIVE doubles (e + t WH): one 256-byte bank row, no conflict for ds_read_b64.
// No atomics, every reduction in a fixed order that does not depend on R: two runs, and one (R, B) call against R (B) calls, give the same bits.
#include "gram_f64.h"

// every product, sum and quotient is rounded on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kSsimTH = 32, kSsimTW = 32;            // output tile
constexpr int kSsimMaxK = 11, kSsimMaxLevels = 5;
constexpr int kSsimHalo = kSsimTH + kSsimMaxK - 1;   // 42
constexpr int kSsimWaves = 4;                        // waves of a tile's workgroup: one partial-sum slot each
constexpr int kSsimPerThread = (kSsimHalo * kSsimHalo + 255) / 256;      // halo elements per thread, at most
constexpr int kSsimFillGroups = 1024;                // workgroups that fill the device: 256 compute units x 2 resident x 2 rounds
constexpr int kSsimF64 = 3;                         // the pooled levels in the workspace (after WU_F32 / WU_BF16 / WU_SSIM_U8)
constexpr int kSsimMaxDim = 1 << 15;

// a stored value as it is loaded (kept raw while the load is in flight), and the mapped image's value made of it: widened to fp64, then
// v * scale + shift in two roundings; the pooled levels are mapped already
template <int DT> struct SsimRaw { typedef float type; };
template <> struct SsimRaw<WU_BF16> { typedef bf16_t type; };
template <> struct SsimRaw<WU_SSIM_U8> { typedef unsigned char type; };
template <> struct SsimRaw<kSsimF64> { typedef double type; };
template <int DT> __device__ __forceinline__ typename SsimRaw<DT>::type ssim_load_raw(const void* p, long long at) {
    return ((const typename SsimRaw<DT>::type*)p)[at];
}
template <int DT> __device__ __forceinline__ double ssim_value(typename SsimRaw<DT>::type raw, double scale, double shift) {
    if (DT == kSsimF64) return (double)raw;
    double v = DT == WU_BF16 ? (double)bf16_to_f32((bf16_t)raw) : (double)raw;
    v = v * scale;
    return v + shift;
}
template <int DT> __device__ __forceinline__ double ssim_load(const void* p, long long at, double scale, double shift) {
    return ssim_value<DT>(ssim_load_raw<DT>(p, at), scale, shift);
}

struct SsimTileArgs {
    const void* x;               // element strides (n, c, h, w)
    const void* y;               // element strides (r, n, c, h, w)
    long long xs[4], ys[5];
    int B, R, C, H, W, k;
    int tiles_x, tiles_y;
    int rows_per_group;          // a workgroup walks rows [g * rows_per_group, min(R, (g + 1) * rows_per_group)) of its (n, c, tile)
    double scale, shift, C1, C2;
    double g[kSsimMaxK];
    double* partial;             // (R, B, C, tiles, waves, 2): sum of ssim, sum of cs
    double* err_partial;         // (R, B, C, tiles, waves, 2): sse, sae; NULL above level 0
    double* map;                 // (R, B, C, H - k + 1, W - k + 1) or NULL
};

// grid (row groups * B * C * tiles): tile fastest, then c, then n, then the row group.  One group (all R rows behind one filtering of x) where
// the (n, c, tile) alone fill the device; the small pooled levels split the rows over more workgroups instead of walking them one by one.
template <int DT, int KT> __global__ __launch_bounds__(256) void ssim_tile_kernel(const SsimTileArgs a) {
    __shared__ double sX[kSsimHalo * kSsimHalo];
    __shared__ double sY[kSsimHalo * kSsimHalo];
    __shared__ double sT[3][kSsimTH * kSsimHalo];        // column-pass results: (mu, F(v v)) of x, then (mu_y, F(y y), F(x y)) per row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = KT ? KT : a.k;
    const int WH = kSsimTW + k - 1, HH = kSsimTH + k - 1;
    const int ntiles = a.tiles_x * a.tiles_y;
    const int tile = blockIdx.x % ntiles, ncg = blockIdx.x / ntiles;
    const int nc = ncg % (a.B * a.C), group = ncg / (a.B * a.C);
    const int c = nc % a.C, n = nc / a.C;
    const int r_lo = group * a.rows_per_group, r_hi = min(a.R, r_lo + a.rows_per_group);
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int oy0 = ty * kSsimTH, ox0 = tx * kSsimTW;
    const int Ho = a.H - k + 1, Wo = a.W - k + 1;
    // the pixels this tile owns for the error sums: its 32 x 32 block, the last tile of an axis also the k - 1 pixels behind it
    const int own_h = ty == a.tiles_y - 1 ? HH : kSsimTH, own_w = tx == a.tiles_x - 1 ? WH : kSsimTW;

    const long long xbase = n * a.xs[0] + c * a.xs[1];
    for (int e = tid; e < HH * WH; e += 256) {
        const int hi = e / WH, hj = e - hi * WH;
        const int gi = oy0 + hi, gj = ox0 + hj;
        sX[e] = gi < a.H && gj < a.W ? ssim_load<DT>(a.x, xbase + gi * a.xs[2] + gj * a.xs[3], a.scale, a.shift) : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < kSsimTH * WH; e += 256) {
        double v = sX[e];
        double m = a.g[0] * v, q = a.g[0] * (v * v);
        for (int t = 1; t < k; ++t) {
            v = sX[e + t * WH];
            m = m + a.g[t] * v;
            q = q + a.g[t] * (v * v);
        }
        sT[0][e] = m;
        sT[1][e] = q;
    }
    __syncthreads();
    // row pass: thread -> column j = tid & 31 of rows (tid >> 5) + 8 q
    const int j = tid & 31, i0 = tid >> 5;
    double mux[4], fxx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int at = (i0 + 8 * q) * WH + j;
        double m = a.g[0] * sT[0][at], s = a.g[0] * sT[1][at];
        for (int t = 1; t < k; ++t) {
            m = m + a.g[t] * sT[0][at + t];
            s = s + a.g[t] * sT[1][at + t];
        }
        mux[q] = m;
        fxx[q] = s;
    }
    __syncthreads();

    // The thread's halo elements e = tid + 256 u are the same for every row: their offsets into a y image and three bit masks (the element
    // exists, lies in the image, is owned for the error sums) are formed once.  A row's values are requested one row AHEAD and stay raw in
    // registers while the current row is filtered, so the loads' latency is not on the path between two barriers.
    long long yoff[kSsimPerThread];
    unsigned m_exists = 0, m_in = 0, m_own = 0;
#pragma unroll
    for (int u = 0; u < kSsimPerThread; ++u) {
        const int e = tid + 256 * u;
        const int hi = e / WH, hj = e - hi * WH;
        const int gi = oy0 + hi, gj = ox0 + hj;
        const bool in = e < HH * WH && gi < a.H && gj < a.W;
        yoff[u] = in ? gi * a.ys[3] + gj * a.ys[4] : 0;
        m_exists |= (e < HH * WH ? 1u : 0u) << u;
        m_in |= (in ? 1u : 0u) << u;
        m_own |= (in && hi < own_h && hj < own_w ? 1u : 0u) << u;
    }
    const long long ybase0 = n * a.ys[1] + c * a.ys[2];
    typename SsimRaw<DT>::type raw[kSsimPerThread];
#pragma unroll
    for (int u = 0; u < kSsimPerThread; ++u) raw[u] = (m_in >> u) & 1 ? ssim_load_raw<DT>(a.y, r_lo * a.ys[0] + ybase0 + yoff[u]) : 0;

    for (int r = r_lo; r < r_hi; ++r) {
        double sse = 0.0, sae = 0.0;
#pragma unroll
        for (int u = 0; u < kSsimPerThread; ++u) {
            const int e = tid + 256 * u;
            if ((m_exists >> u) & 1) {
                const double v = (m_in >> u) & 1 ? ssim_value<DT>(raw[u], a.scale, a.shift) : 0.0;
                sY[e] = v;
                if ((m_own >> u) & 1) {
                    const double d = sX[e] - v;
                    sse = sse + d * d;
                    sae = sae + fabs(d);
                }
            }
        }
        if (r + 1 < r_hi) {
            const long long ybase = (r + 1) * a.ys[0] + ybase0;
#pragma unroll
            for (int u = 0; u < kSsimPerThread; ++u)
                if ((m_in >> u) & 1) raw[u] = ssim_load_raw<DT>(a.y, ybase + yoff[u]);
        }
        __syncthreads();
        for (int e = tid; e < kSsimTH * WH; e += 256) {
            double v = sY[e], u = sX[e];
            double m = a.g[0] * v, q = a.g[0] * (v * v), p = a.g[0] * (u * v);
            for (int t = 1; t < k; ++t) {
                v = sY[e + t * WH];
                u = sX[e + t * WH];
                m = m + a.g[t] * v;
                q = q + a.g[t] * (v * v);
                p = p + a.g[t] * (u * v);
            }
            sT[0][e] = m;
            sT[1][e] = q;
            sT[2][e] = p;
        }
        __syncthreads();
        double sum_s = 0.0, sum_c = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 8 * q, at = i * WH + j;
            double muy = a.g[0] * sT[0][at], fyy = a.g[0] * sT[1][at], fxy = a.g[0] * sT[2][at];
            for (int t = 1; t < k; ++t) {
                muy = muy + a.g[t] * sT[0][at + t];
                fyy = fyy + a.g[t] * sT[1][at + t];
                fxy = fxy + a.g[t] * sT[2][at + t];
            }
            const double mxx = mux[q] * mux[q], myy = muy * muy, mxy = mux[q] * muy;
            const double sx = fxx[q] - mxx, sy = fyy - myy, sxy = fxy - mxy;
            const double cs = (2.0 * sxy + a.C2) / ((sx + sy) + a.C2);
            const double ss = ((2.0 * mxy + a.C1) / ((mxx + myy) + a.C1)) * cs;
            const int gi = oy0 + i, gj = ox0 + j;
            if (gi < Ho && gj < Wo) {
                sum_s = sum_s + ss;
                sum_c = sum_c + cs;
                if (a.map) a.map[((((long long)r * a.B + n) * a.C + c) * Ho + gi) * Wo + gj] = ss;
            }
        }
        sum_s = wave_sum_f64(sum_s);
        sum_c = wave_sum_f64(sum_c);
        sse = wave_sum_f64(sse);
        sae = wave_sum_f64(sae);
        // one slot per wave, folded by the finish kernel: no barrier here.  The next row's sY is written while other waves may still be
        // in this row pass (which reads sT only); its column pass, which rewrites sT, comes after the next barrier.
        if (lane == 0) {
            const long long slot = (((((long long)r * a.B + n) * a.C + c) * ntiles + tile) * kSsimWaves + wave) * 2;
            a.partial[slot] = sum_s;
            a.partial[slot + 1] = sum_c;
            if (a.err_partial) {
                a.err_partial[slot] = sse;
                a.err_partial[slot + 1] = sae;
            }
        }
    }
}

struct SsimPoolArgs {
    const void* x;
    const void* y;
    long long xs[4], ys[5];
    int B, R, C, H, W;           // the SOURCE level's size
    double scale, shift;
    double* xo;                  // (B, C, Ho, Wo)
    double* yo;                  // (R, B, C, Ho, Wo)
};

// one thread per output value of the x images and then of the y images; ((p00 + p01) + (p10 + p11)) * 0.25 with zeros in front of an odd axis
template <int DT> __global__ __launch_bounds__(256) void ssim_pool_kernel(const SsimPoolArgs a) {
    const int ph = a.H & 1, pw = a.W & 1;
    const int Ho = a.H / 2 + ph, Wo = a.W / 2 + pw;
    const long long per = (long long)Ho * Wo, nx = (long long)a.B * a.C * per, total = nx * (1 + a.R);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const bool isx = idx < nx;
    const long long id = isx ? idx : idx - nx;
    const int jo = (int)(id % Wo), io = (int)((id / Wo) % Ho);
    long long img = id / per;
    const int c = (int)(img % a.C);
    img /= a.C;
    const int n = (int)(img % a.B), r = (int)(img / a.B);      // r = 0 for x
    const void* src = isx ? a.x : a.y;
    const long long base = isx ? n * a.xs[0] + c * a.xs[1] : r * a.ys[0] + n * a.ys[1] + c * a.ys[2];
    const long long sh = isx ? a.xs[2] : a.ys[3], sw = isx ? a.xs[3] : a.ys[4];
    const int i1 = 2 * io + 1 - ph, j1 = 2 * jo + 1 - pw, i0 = i1 - 1, j0 = j1 - 1;      // i0 / j0 = -1: the padded zero
    const double p00 = i0 >= 0 && j0 >= 0 ? ssim_load<DT>(src, base + i0 * sh + j0 * sw, a.scale, a.shift) : 0.0;
    const double p01 = i0 >= 0 ? ssim_load<DT>(src, base + i0 * sh + j1 * sw, a.scale, a.shift) : 0.0;
    const double p10 = j0 >= 0 ? ssim_load<DT>(src, base + i1 * sh + j0 * sw, a.scale, a.shift) : 0.0;
    const double p11 = ssim_load<DT>(src, base + i1 * sh + j1 * sw, a.scale, a.shift);
    (isx ? a.xo : a.yo)[id] = ((p00 + p01) + (p10 + p11)) * 0.25;
}

struct SsimFinishArgs {
    const double* partial[kSsimMaxLevels];
    const double* err_partial;
    int slots[kSsimMaxLevels];           // tiles * kSsimWaves partial sums per (r, n, c)
    double count[kSsimMaxLevels];        // entries of a level's maps
    int C, levels;
    double* ssim_mean;                   // (R, B, C, levels)
    double* cs_mean;
    double* err;                         // (R, B, 2)
};

// one wave per (r, n): lane l adds slots l, l + 64, .. in that order, the lanes are then summed in wave_sum_f64's order
__global__ __launch_bounds__(64) void ssim_finish_kernel(const SsimFinishArgs a) {
    const long long rn = blockIdx.x;
    const int lane = threadIdx.x;
    for (int c = 0; c < a.C; ++c)
        for (int l = 0; l < a.levels; ++l) {
            const double* p = a.partial[l] + (rn * a.C + c) * a.slots[l] * 2;
            double s = 0.0, q = 0.0;
            for (int t = lane; t < a.slots[l]; t += 64) {
                s = s + p[2 * t];
                q = q + p[2 * t + 1];
            }
            s = wave_sum_f64(s);
            q = wave_sum_f64(q);
            if (lane == 0) {
                a.ssim_mean[(rn * a.C + c) * a.levels + l] = s / a.count[l];
                a.cs_mean[(rn * a.C + c) * a.levels + l] = q / a.count[l];
            }
        }
    const double* p = a.err_partial + rn * a.C * a.slots[0] * 2;
    double s = 0.0, q = 0.0;
    for (int t = lane; t < a.C * a.slots[0]; t += 64) {
        s = s + p[2 * t];
        q = q + p[2 * t + 1];
    }
    s = wave_sum_f64(s);
    q = wave_sum_f64(q);
    if (lane == 0) {
        a.err[rn * 2] = s;
        a.err[rn * 2 + 1] = q;
    }
}

struct SsimPlan {
    int h[kSsimMaxLevels], w[kSsimMaxLevels], tiles_x[kSsimMaxLevels], tiles_y[kSsimMaxLevels];
    size_t x_off[kSsimMaxLevels], y_off[kSsimMaxLevels], part_off[kSsimMaxLevels], err_off, doubles;   // offsets in doubles
};

// sizes, tiles and workspace offsets of every level; false for anything out of range
bool ssim_plan(int B, int R, int C, int H, int W, int k, int levels, SsimPlan* p) {
    if (B < 1 || R < 1 || C < 1 || k < 3 || k > kSsimMaxK || !(k & 1) || H < k || W < k || H > kSsimMaxDim || W > kSsimMaxDim) return false;
    if (levels != 1 && levels != kSsimMaxLevels) return false;
    if (levels > 1 && (H < W ? H : W) <= (k - 1) * 16) return false;
    if ((long long)B * C > (1 << 24) || (long long)R * B > (1 << 24)) return false;
    size_t at = 0;
    int h = H, w = W;
    for (int l = 0; l < levels; ++l) {
        p->h[l] = h;
        p->w[l] = w;
        p->tiles_y[l] = cdiv(h - k + 1, kSsimTH);
        p->tiles_x[l] = cdiv(w - k + 1, kSsimTW);
        const long long tiles = (long long)p->tiles_x[l] * p->tiles_y[l];
        if ((long long)B * C * tiles >= (1ll << 31)) return false;
        p->x_off[l] = p->y_off[l] = 0;
        if (l > 0) {
            p->x_off[l] = at;
            at += (size_t)B * C * h * w;
            p->y_off[l] = at;
            at += (size_t)R * B * C * h * w;
        }
        p->part_off[l] = at;
        at += (size_t)R * B * C * tiles * kSsimWaves * 2;
        if (l == 0) {
            p->err_off = at;
            at += (size_t)R * B * C * tiles * kSsimWaves * 2;
        }
        if (l + 1 < levels && ((size_t)B * C * (1 + R) * (h / 2 + 1) * (w / 2 + 1) + 255) / 256 >= (1ull << 31)) return false;
        h = h / 2 + (h & 1);
        w = w / 2 + (w & 1);
    }
    p->doubles = at;
    return true;
}

template <int DT> void ssim_launch_tile(const SsimTileArgs& a, unsigned grid, hipStream_t s) {
    if (a.k == kSsimMaxK) hipLaunchKernelGGL((ssim_tile_kernel<DT, kSsimMaxK>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((ssim_tile_kernel<DT, 0>), dim3(grid), dim3(256), 0, s, a);
}

}  // namespace

extern "C" int wu_ssim_tile_h(void) { return kSsimTH; }
extern "C" int wu_ssim_tile_w(void) { return kSsimTW; }

extern "C" size_t wu_ssim_workspace_bytes(int B, int R, int C, int H, int W, int k, int levels) {
    SsimPlan p;
    return ssim_plan(B, R, C, H, W, k, levels, &p) ? p.doubles * sizeof(double) : 0;
}

extern "C" int wu_ssim_pairs(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, const void* y, long long ys_r,
                             long long ys_n, long long ys_c, long long ys_h, long long ys_w, int dtype, int B, int R, int C, int H, int W,
                             double scale, double shift, double L, double K1, double K2, const double* window, int k, int levels,
                             void* workspace, double* ssim_mean, double* cs_mean, double* err, double* ssim_map, void* stream) {
    WU_REQUIRE(k >= 3 && k <= kSsimMaxK && (k & 1), "wu_ssim_pairs: window size k %d must be odd and in 3..%d", k, kSsimMaxK);
    WU_REQUIRE(B >= 1 && R >= 1 && C >= 1, "wu_ssim_pairs: B %d / R %d / C %d must be at least 1", B, R, C);
    WU_REQUIRE(H >= k && W >= k, "wu_ssim_pairs: image %d x %d is smaller than the window k %d", H, W, k);
    WU_REQUIRE(levels == 1 || levels == kSsimMaxLevels, "wu_ssim_pairs: levels %d must be 1 or %d", levels, kSsimMaxLevels);
    WU_REQUIRE(levels == 1 || (H < W ? H : W) > (k - 1) * 16,
               "wu_ssim_pairs: MS-SSIM over %d levels with k %d needs min(H, W) > %d, got %d x %d", levels, k, (k - 1) * 16, H, W);
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16 || dtype == WU_SSIM_U8, "wu_ssim_pairs: unknown dtype %d", dtype);
    WU_REQUIRE(x && y && window && workspace && ssim_mean && cs_mean && err, "wu_ssim_pairs: NULL pointer");
    SsimPlan p;
    WU_REQUIRE(ssim_plan(B, R, C, H, W, k, levels, &p), "wu_ssim_pairs: B %d R %d C %d H %d W %d out of range", B, R, C, H, W);
    hipStream_t s = (hipStream_t)stream;
    double* ws = (double*)workspace;

    SsimFinishArgs f;
    memset(&f, 0, sizeof(f));
    const void* lx = x;
    const void* ly = y;
    long long lxs[4] = {xs_n, xs_c, xs_h, xs_w}, lys[5] = {ys_r, ys_n, ys_c, ys_h, ys_w};
    int dt = dtype;
    for (int l = 0; l < levels; ++l) {
        const int h = p.h[l], w = p.w[l];
        if (l + 1 < levels) {      // the next level first: it reads what this level's tiles read
            SsimPoolArgs pa;
            pa.x = lx;
            pa.y = ly;
            memcpy(pa.xs, lxs, sizeof(lxs));
            memcpy(pa.ys, lys, sizeof(lys));
            pa.B = B, pa.R = R, pa.C = C, pa.H = h, pa.W = w;
            pa.scale = scale, pa.shift = shift;
            pa.xo = ws + p.x_off[l + 1];
            pa.yo = ws + p.y_off[l + 1];
            const unsigned grid = (unsigned)(((size_t)B * C * (1 + R) * p.h[l + 1] * p.w[l + 1] + 255) / 256);
            if (dt == WU_F32) hipLaunchKernelGGL(ssim_pool_kernel<WU_F32>, dim3(grid), dim3(256), 0, s, pa);
            else if (dt == WU_BF16) hipLaunchKernelGGL(ssim_pool_kernel<WU_BF16>, dim3(grid), dim3(256), 0, s, pa);
            else if (dt == WU_SSIM_U8) hipLaunchKernelGGL(ssim_pool_kernel<WU_SSIM_U8>, dim3(grid), dim3(256), 0, s, pa);
            else hipLaunchKernelGGL(ssim_pool_kernel<kSsimF64>, dim3(grid), dim3(256), 0, s, pa);
            WU_LAUNCH_CHECK("ssim_pool_kernel");
        }
        SsimTileArgs ta;
        ta.x = lx;
        ta.y = ly;
        memcpy(ta.xs, lxs, sizeof(lxs));
        memcpy(ta.ys, lys, sizeof(lys));
        ta.B = B, ta.R = R, ta.C = C, ta.H = h, ta.W = w, ta.k = k;
        ta.tiles_x = p.tiles_x[l], ta.tiles_y = p.tiles_y[l];
        ta.scale = scale, ta.shift = shift;
        ta.C1 = (K1 * L) * (K1 * L);
        ta.C2 = (K2 * L) * (K2 * L);
        for (int t = 0; t < kSsimMaxK; ++t) ta.g[t] = t < k ? window[t] : 0.0;
        ta.partial = ws + p.part_off[l];
        ta.err_partial = l == 0 ? ws + p.err_off : nullptr;
        ta.map = l == 0 ? ssim_map : nullptr;
        const int tiles = p.tiles_x[l] * p.tiles_y[l];
        // fewer than kSsimFillGroups workgroups of (n, c, tile): split the rows until there are about that many (at most one per row)
        const long long per_group = (long long)B * C * tiles;
        const int want = per_group < kSsimFillGroups ? (int)((kSsimFillGroups + per_group - 1) / per_group) : 1;
        ta.rows_per_group = cdiv(R, want < R ? want : R);
        const unsigned grid = (unsigned)(per_group * cdiv(R, ta.rows_per_group));
        if (dt == WU_F32) ssim_launch_tile<WU_F32>(ta, grid, s);
        else if (dt == WU_BF16) ssim_launch_tile<WU_BF16>(ta, grid, s);
        else if (dt == WU_SSIM_U8) ssim_launch_tile<WU_SSIM_U8>(ta, grid, s);
        else ssim_launch_tile<kSsimF64>(ta, grid, s);
        WU_LAUNCH_CHECK("ssim_tile_kernel");
        f.partial[l] = ta.partial;
        f.slots[l] = tiles * kSsimWaves;
        f.count[l] = (double)(h - k + 1) * (double)(w - k + 1);
        if (l + 1 < levels) {      // the pooled levels: contiguous fp64 in the workspace, mapped already
            lx = ws + p.x_off[l + 1];
            ly = ws + p.y_off[l + 1];
            const long long hw = (long long)p.h[l + 1] * p.w[l + 1];
            lxs[0] = C * hw, lxs[1] = hw, lxs[2] = p.w[l + 1], lxs[3] = 1;
            lys[0] = (long long)B * C * hw, lys[1] = C * hw, lys[2] = hw, lys[3] = p.w[l + 1], lys[4] = 1;
            dt = kSsimF64;
        }
    }
    f.err_partial = ws + p.err_off;
    f.C = C, f.levels = levels;
    f.ssim_mean = ssim_mean, f.cs_mean = cs_mean, f.err = err;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)((long long)R * B)), dim3(64), 0, s, f);
    WU_LAUNCH_CHECK("ssim_finish_kernel");
    return 0;
}
