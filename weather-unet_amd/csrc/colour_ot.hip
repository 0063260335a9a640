// Colour-transfer baselines: per-channel histogram matching and its N-dimensional form, the iterative distribution transfer of Pitie,
// Kokaram and Dahyot (sliced optimal transport) -- wu/colour.py; tests/_colour_ref.py states the arithmetic.
//   * colour_load_kernel     one thread per pixel of a virtual image: the three channels are read through the input's strides, widened and
//                            mapped to [0, 1] units, and written as the fp64 state (nimg, 3, n).  Virtual image g = r B + b reads input
//                            image g % B: the R targets of an image share the input by index, never by a copy;
//   * colour_palette_kernel  one thread per palette point: its three keys under the iteration's rotation, axis-major (C * 3, P) -- sorted by
//                            the segmented sort of swd.hip (wu_swd_sort_columns), once per iteration whatever the number of images;
//   * colour_project_kernel  one thread per pixel: the three keys of the state, axis-major (nimg * 3, n), for the same sort;
//   * colour_match_kernel    the fused match and update.  A workgroup owns kColPerBlock consecutive pixels of one virtual image.  It stages
//                            every stride-th key of the image's three sorted columns in LDS (at most kColSamples per column), so the first
//                            ten steps of every search touch no memory; the rest of a search runs over the `stride` keys between two
//                            samples, in L2.  Per pixel and axis: the key again (the same operations, hence the same bits as the sorted
//                            copy), lo = #{key' < key}, hi = #{key' <= key} (one probe when the key is unique), t = ((lo + hi) P) / (2 n),
//                            delta = q[t] - key; then the rotation back and the update of the three channels.  Thread t takes pixels
//                            t, t + 256, ..: the 64 lanes of a wave read and write 512 contiguous bytes per channel.  All workgroups of an
//                            image run on one XCD, so its columns stay in that XCD's L2 (0.55 ms against 1.01 ms per iteration of 80
//                            images of 224 x 224 with the images spread over all eight);
//   * colour_store_kernel    clip to [0, 1], the inverse mapping, rounding, and the write through the output's strides.
// No atomics, no reduction across threads at all: the same inputs give the same bits, however the images are chunked.
#include <math.h>

#include "wu_common.h"

// every product, sum and quotient is rounded on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kColMaxN = 1 << 21;              // pixels of an image, points of a palette: the range of the sort
constexpr int kColSortCols = 4096;             // columns wu_swd_sort_columns takes at once
constexpr int kColSamples = 1024;              // keys of one sorted column in LDS: 3 x 8 KiB per workgroup
constexpr int kColPer = 4;                     // pixels per thread
constexpr int kColPerBlock = 256 * kColPer;
constexpr size_t kColChunkBytes = 256ull << 20;   // the keys of at most this many bytes are in flight (and as much again for the sort)

struct ColRot {
    double r[9];                               // row a = axis a
};

__device__ __forceinline__ double col_key(const ColRot& R, int a, double s0, double s1, double s2) {
    return (R.r[3 * a] * s0 + R.r[3 * a + 1] * s1) + R.r[3 * a + 2] * s2;
}

template <int DT> __device__ __forceinline__ double col_widen(const void* p, long long at) {
    if (DT == WU_BF16) return (double)bf16_to_f32(((const bf16_t*)p)[at]);
    if (DT == WU_SSIM_U8) return (double)((const unsigned char*)p)[at];
    return (double)((const float*)p)[at];
}

struct ColLoadArgs {
    const void* x;               // element strides (n, c, h, w)
    long long xs[4];
    int B, W, n;
    long long first;             // the global index of virtual image 0 of this call
    long long total;             // nimg * n
    double scale, shift, L;
    double* state;               // (nimg, 3, n)
};

template <int DT> __global__ __launch_bounds__(256) void colour_load_kernel(const ColLoadArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const long long v = idx / a.n;
    const int p = (int)(idx % a.n);
    const long long b = (a.first + v) % a.B;
    const long long at = b * a.xs[0] + (long long)(p / a.W) * a.xs[2] + (long long)(p % a.W) * a.xs[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double s = col_widen<DT>(a.x, at + c * a.xs[1]) * a.scale;
        s = s + a.shift;
        a.state[(v * 3 + c) * a.n + p] = s / a.L;
    }
}

__global__ __launch_bounds__(256) void colour_palette_kernel(const double* pal, long long total, int P, const ColRot R, double* keys) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long c = idx / P;
    const int p = (int)(idx % P);
    const double s0 = pal[idx * 3], s1 = pal[idx * 3 + 1], s2 = pal[idx * 3 + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) keys[(c * 3 + a) * P + p] = col_key(R, a, s0, s1, s2);
}

__global__ __launch_bounds__(256) void colour_project_kernel(const double* state, long long total, int n, const ColRot R, double* keys) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long v = idx / n;
    const int p = (int)(idx % n);
    const double* s = state + v * 3 * n + p;
    const double s0 = s[0], s1 = s[n], s2 = s[2 * (long long)n];
#pragma unroll
    for (int a = 0; a < 3; ++a) keys[(v * 3 + a) * n + p] = col_key(R, a, s0, s1, s2);
}

// #{i < n : col[i] < key} (UPPER = false) or #{i < n : col[i] <= key} (UPPER = true): bisection over the LDS samples smp[j] = col[j stride],
// j < ns, then over the keys strictly between two samples in global memory
template <bool UPPER> __device__ __forceinline__ int col_count(const double* smp, int ns, const double* col, int n, int stride, double key) {
    int a = 0, b = ns;
    while (a < b) {
        const int mid = (a + b) >> 1;
        const double v = smp[mid];
        if (UPPER ? v <= key : v < key) a = mid + 1;
        else b = mid;
    }
    if (a == 0) return 0;
    // sample a - 1 counts, sample a (if there is one) does not: the answer is in ((a - 1) stride, min(a stride, n)]
    b = min(a * stride, n);
    a = (a - 1) * stride + 1;
    while (a < b) {
        const int mid = (a + b) >> 1;
        const double v = col[mid];
        if (UPPER ? v <= key : v < key) a = mid + 1;
        else b = mid;
    }
    return a;
}

struct ColMatchArgs {
    double* state;               // (nimg, 3, n), updated in place
    const double* sorted;        // (nimg * 3, n): the sorted keys of the state
    const double* pal;           // (npal * 3, P): the sorted keys of the palettes
    const int* cls;              // (nimg): the palette of every virtual image
    int n, P, npal, stride, ns;
    int nimg, nblk;              // images of the launch, workgroups per image
    double step;
    ColRot R;
};

// Workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own, and every search is a string of scattered 8-byte reads of
// one image's sorted columns (1.2 MB at 224 x 224).  All workgroups of an image therefore go to ONE XCD -- image v to XCD v % 8 -- so that
// an L2 holds the columns of the few images its own workgroups are on, not a slice of every image in flight.  The grid is padded to a
// multiple of 8 images; workgroups of the padding leave at once.
__global__ __launch_bounds__(256) void colour_match_kernel(const ColMatchArgs a) {
    __shared__ double smp[3][kColSamples];
    const int tid = threadIdx.x;
    const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
    const long long v = (long long)(seq / a.nblk) * 8 + xcd;
    const int blk = seq % a.nblk;
    if (v >= a.nimg) return;
    const int cl = a.cls[v];
    // the host has checked the targets; this only keeps a bad device array from reading outside the palettes (uniform over the workgroup)
    if (cl < 0 || cl >= a.npal) return;
    const double* sorted = a.sorted + v * 3 * a.n;
    for (int e = tid; e < 3 * a.ns; e += 256) {
        const int ax = e / a.ns, j = e % a.ns;
        smp[ax][j] = sorted[(long long)ax * a.n + (long long)j * a.stride];
    }
    __syncthreads();
    const double* pal = a.pal + (long long)cl * 3 * a.P;
    double* st = a.state + v * 3 * a.n;
    const int p0 = blk * kColPerBlock;
    for (int u = 0; u < kColPer; ++u) {
        const int p = p0 + u * 256 + tid;
        if (p >= a.n) break;
        const double s0 = st[p], s1 = st[a.n + p], s2 = st[2 * (long long)a.n + p];
        double d[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const double key = col_key(a.R, ax, s0, s1, s2);
            const double* col = sorted + (long long)ax * a.n;
            const int lo = col_count<false>(smp[ax], a.ns, col, a.n, a.stride, key);
            // col[lo] is this pixel's key or an equal one: where the next key is larger the pixel has no ties
            int hi = lo + 1;
            if (hi < a.n && col[hi] <= key) hi = col_count<true>(smp[ax], a.ns, col, a.n, a.stride, key);
            hi = min(hi, a.n);
            long long t = ((long long)(lo + hi) * a.P) / (2ll * a.n);
            t = t > a.P - 1 ? a.P - 1 : t;      // only reached with non-finite keys
            d[ax] = pal[(long long)ax * a.P + t] - key;
        }
        const double in[3] = {s0, s1, s2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double dc = (d[0] * a.R.r[c] + d[1] * a.R.r[3 + c]) + d[2] * a.R.r[6 + c];
            st[(long long)c * a.n + p] = in[c] + a.step * dc;
        }
    }
}

struct ColStoreArgs {
    const double* state;         // (nimg, 3, n)
    void* y;                     // (R, B, 3, H, W), element strides (r, n, c, h, w)
    long long ys[5];
    int B, W, n;
    long long first, total;
    double lo, span;
    int round_int;               // the "uint8" range on a floating output
};

template <int DT> __global__ __launch_bounds__(256) void colour_store_kernel(const ColStoreArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.total) return;
    const long long v = idx / a.n;
    const int p = (int)(idx % a.n);
    const long long g = a.first + v;
    const long long at = (g / a.B) * a.ys[0] + (g % a.B) * a.ys[1] + (long long)(p / a.W) * a.ys[3] + (long long)(p % a.W) * a.ys[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double s = a.state[(v * 3 + c) * a.n + p];
        const double u = fmin(fmax(s, 0.0), 1.0);
        double val = a.lo + u * a.span;
        const long long o = at + c * a.ys[2];
        if (DT == WU_SSIM_U8) {
            val = fmin(fmax(rint(val), 0.0), 255.0);
            ((unsigned char*)a.y)[o] = (unsigned char)val;
        } else {
            if (a.round_int) val = rint(val);
            const float f = (float)val;
            if (DT == WU_BF16) ((bf16_t*)a.y)[o] = f32_to_bf16(f);
            else ((float*)a.y)[o] = f;
        }
    }
}

bool col_range(long long nimg, int n, int npal, int P) {
    return nimg >= 1 && nimg <= (1ll << 24) && n >= 1 && n <= kColMaxN && npal >= 1 && npal <= (1 << 16) && P >= 1 && P <= kColMaxN;
}

// how many virtual images go through project / sort / match at once: the sort's column limit, and kColChunkBytes of keys
int col_chunk(long long nimg, int n) {
    long long k = (long long)(kColChunkBytes / ((size_t)3 * n * sizeof(double)));
    if (k > kColSortCols / 3) k = kColSortCols / 3;
    if (k > nimg) k = nimg;
    return k < 1 ? 1 : (int)k;
}

unsigned col_grid(long long total) { return (unsigned)((total + 255) / 256); }

bool col_dtype(int dt) { return dt == WU_F32 || dt == WU_BF16 || dt == WU_SSIM_U8; }

}  // namespace

extern "C" size_t wu_colour_ot_workspace_bytes(int nimg, int n, int npal, int P) {
    if (!col_range(nimg, n, npal, P)) return 0;
    // the keys of a chunk of images and the sort's temporary of the same size; or, for wu_colour_ot_palette_keys, the temporary of its sort
    const size_t img = 2 * (size_t)col_chunk(nimg, n) * 3 * n * sizeof(double);
    const size_t cols = (size_t)3 * npal < (size_t)kColSortCols ? (size_t)3 * npal : (size_t)kColSortCols;
    const size_t pal = cols * P * sizeof(double);
    return img > pal ? img : pal;
}

extern "C" int wu_colour_ot_load(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int B, int H, int W,
                                 double scale, double shift, double L, long long first, int nimg, double* state, void* stream) {
    WU_REQUIRE(col_dtype(dtype), "wu_colour_ot_load: unknown dtype %d", dtype);
    WU_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kColMaxN, "wu_colour_ot_load: B %d H %d W %d out of range (H W <= %d)", B, H,
               W, kColMaxN);
    WU_REQUIRE(col_range(nimg, H * W, 1, 1) && first >= 0, "wu_colour_ot_load: nimg %d / first %lld out of range", nimg, first);
    WU_REQUIRE(L > 0.0, "wu_colour_ot_load: the data range L must be positive");
    WU_REQUIRE(x && state, "wu_colour_ot_load: NULL pointer");
    ColLoadArgs a;
    a.x = x;
    a.xs[0] = xs_n, a.xs[1] = xs_c, a.xs[2] = xs_h, a.xs[3] = xs_w;
    a.B = B, a.W = W, a.n = H * W, a.first = first, a.total = (long long)nimg * a.n;
    a.scale = scale, a.shift = shift, a.L = L, a.state = state;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(col_grid(a.total));
    if (dtype == WU_F32) hipLaunchKernelGGL(colour_load_kernel<WU_F32>, grid, dim3(256), 0, s, a);
    else if (dtype == WU_BF16) hipLaunchKernelGGL(colour_load_kernel<WU_BF16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(colour_load_kernel<WU_SSIM_U8>, grid, dim3(256), 0, s, a);
    WU_LAUNCH_CHECK("colour_load_kernel");
    return 0;
}

extern "C" int wu_colour_ot_palette_keys(const double* palette, int npal, int P, const double* rotation, double* keys, void* workspace,
                                         void* stream) {
    WU_REQUIRE(col_range(1, 1, npal, P), "wu_colour_ot_palette_keys: npal %d (1..65536) or P %d (1..%d) out of range", npal, P, kColMaxN);
    WU_REQUIRE(palette && rotation && keys && workspace, "wu_colour_ot_palette_keys: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    ColRot R;
    memcpy(R.r, rotation, sizeof(R.r));
    const long long total = (long long)npal * P;
    hipLaunchKernelGGL(colour_palette_kernel, dim3(col_grid(total)), dim3(256), 0, s, palette, total, P, R, keys);
    WU_LAUNCH_CHECK("colour_palette_kernel");
    const int cols = 3 * npal;
    for (int c0 = 0; c0 < cols; c0 += kColSortCols) {
        const int k = cols - c0 < kColSortCols ? cols - c0 : kColSortCols;
        const int rc = wu_swd_sort_columns(keys + (long long)c0 * P, P, k, workspace, stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int wu_colour_ot_step(double* state, int nimg, int n, const double* palette_keys, int npal, int P, const int* classes,
                                 const double* rotation, double step, void* workspace, void* stream) {
    WU_REQUIRE(col_range(nimg, n, npal, P), "wu_colour_ot_step: nimg %d, n %d (1..%d), npal %d or P %d (1..%d) out of range", nimg, n,
               kColMaxN, npal, P, kColMaxN);
    WU_REQUIRE(state && palette_keys && classes && rotation && workspace, "wu_colour_ot_step: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    ColRot R;
    memcpy(R.r, rotation, sizeof(R.r));
    const int chunk = col_chunk(nimg, n);
    double* keys = (double*)workspace;
    double* tmp = keys + (size_t)chunk * 3 * n;
    const int stride = cdiv(n, kColSamples);
    for (int v0 = 0; v0 < nimg; v0 += chunk) {
        const int k = nimg - v0 < chunk ? nimg - v0 : chunk;
        double* st = state + (long long)v0 * 3 * n;
        const long long total = (long long)k * n;
        hipLaunchKernelGGL(colour_project_kernel, dim3(col_grid(total)), dim3(256), 0, s, (const double*)st, total, n, R, keys);
        WU_LAUNCH_CHECK("colour_project_kernel");
        const int rc = wu_swd_sort_columns(keys, n, 3 * k, tmp, stream);
        if (rc) return rc;
        ColMatchArgs a;
        a.state = st, a.sorted = keys, a.pal = palette_keys, a.cls = classes + v0;
        a.n = n, a.P = P, a.npal = npal, a.stride = stride, a.ns = cdiv(n, stride);
        a.nimg = k, a.nblk = cdiv(n, kColPerBlock);
        a.step = step, a.R = R;
        hipLaunchKernelGGL(colour_match_kernel, dim3((unsigned)(8 * cdiv(k, 8) * a.nblk)), dim3(256), 0, s, a);
        WU_LAUNCH_CHECK("colour_match_kernel");
    }
    return 0;
}

extern "C" int wu_colour_ot_store(const double* state, long long first, int nimg, void* y, long long ys_r, long long ys_n, long long ys_c,
                                  long long ys_h, long long ys_w, int dtype, int B, int H, int W, double lo, double span, int round_int,
                                  void* stream) {
    WU_REQUIRE(col_dtype(dtype), "wu_colour_ot_store: unknown dtype %d", dtype);
    WU_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= kColMaxN, "wu_colour_ot_store: B %d H %d W %d out of range (H W <= %d)", B,
               H, W, kColMaxN);
    WU_REQUIRE(col_range(nimg, H * W, 1, 1) && first >= 0, "wu_colour_ot_store: nimg %d / first %lld out of range", nimg, first);
    WU_REQUIRE(state && y, "wu_colour_ot_store: NULL pointer");
    ColStoreArgs a;
    a.state = state, a.y = y;
    a.ys[0] = ys_r, a.ys[1] = ys_n, a.ys[2] = ys_c, a.ys[3] = ys_h, a.ys[4] = ys_w;
    a.B = B, a.W = W, a.n = H * W, a.first = first, a.total = (long long)nimg * a.n;
    a.lo = lo, a.span = span, a.round_int = round_int;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(col_grid(a.total));
    if (dtype == WU_F32) hipLaunchKernelGGL(colour_store_kernel<WU_F32>, grid, dim3(256), 0, s, a);
    else if (dtype == WU_BF16) hipLaunchKernelGGL(colour_store_kernel<WU_BF16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(colour_store_kernel<WU_SSIM_U8>, grid, dim3(256), 0, s, a);
    WU_LAUNCH_CHECK("colour_store_kernel");
    return 0;
}
