// Antialiased resampling in front of the metrics (wu/resample.py): Pillow's ImagingResample (libImaging/Resample.c) for the box, bilinear,
// bicubic and Lanczos filters, in its 8-bit form (Image.resize of an RGB image) and in its float form (mode 'F' per channel: Parmar et
// al.'s "clean" resize), on ragged batches, as ONE launch with no intermediate image in global memory.
//
// Pillow resamples in two passes, horizontal first, and rounds the intermediate image (clip8 to uint8, or float64 -> float32).  A
// workgroup here owns a band of output rows of one image and walks the source rows that band needs in ascending order.  Per source row:
//   1. the row is staged in LDS on the 0..255 scale (bytes, or float32 for a float source in float mode), coalesced, converted once;
//   2. thread ox filters output column ox of that row from LDS -- one row of Pillow's intermediate image, rounded as Pillow rounds it;
//   3. the same thread adds the three values, times the row's vertical coefficient, into its accumulators of the band's output rows
//      that are live at this source row (int32 or float64, in registers).
// Ascending source rows are Pillow's summation order, so the streamed sums carry the same bits; there are no atomics, and a band's
// height changes which workgroup computes a row, never how.  Because the thread that filters a column also owns that column's
// accumulators, the horizontally filtered row never has to be exchanged: LDS holds the SOURCE row (what every thread reads at overlapping
// taps), not the filtered one.  A pass whose source and output size are equal is skipped as Pillow skips it (kx == 0 / ky == 0): the
// thread then reads its source pixel directly, or each source row is one output row.
//
// The coefficient tables are Pillow's precompute_coeffs (and normalize_coeffs_8bpc), built on the host by wu/resample.py in float64 --
// Lanczos needs the C library's sin -- and cached there by (in, out, filter); the horizontal table is stored tap-major, [kx][Wout], so that
// a wave's loads of one tap are contiguous.
//
// WU_RESAMPLE_EMU: scratch/resample_emu.cpp compiles the device functions below as host C++ and runs them thread by thread under the
// address and undefined-behaviour sanitizers against the bytes of tests/_resample_ref.py.
#ifdef WU_RESAMPLE_EMU
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#define WU_HD inline
typedef unsigned short bf16_t;
inline float bf16_to_f32(bf16_t v) { const uint32_t u = (uint32_t)v << 16; float f; memcpy(&f, &u, 4); return f; }
inline bf16_t f32_to_bf16(float f) {                       // round to nearest even (finite inputs only here)
    uint32_t u; memcpy(&u, &f, 4);
    return (bf16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
#else
#include "wu_common.h"
#define WU_HD __device__ __forceinline__
#endif

// Every floating-point operation below is one IEEE operation in the order written (csrc/image.hip says why): Resample.c rounds the
// product pixel * k and then the sum, and x * 127.5f + 127.5f is two roundings in torch.
#pragma clang fp contract(off)

namespace {

constexpr int kPrec = 22;            // Resample.c PRECISION_BITS = 32 - 8 - 2
constexpr int kBandMax = 8;          // output rows per workgroup: 3 x 8 float64 accumulators = 48 VGPRs per thread
constexpr int kMaxOut = 1024;        // one thread per output column, one workgroup per band
constexpr size_t kMaxLds = 64 * 1024;

enum { SRC_U8 = 0, SRC_F32 = 1, SRC_BF16 = 2 };
enum { MODE_F32 = 0, MODE_U8 = 1 };
enum { EPI_NHWC_U8 = 0, EPI_RAW = 1, EPI_UNIT = 2, EPI_NORM = 3, EPI_INCEPTION = 4 };

struct ResDesc {                     // one per image (host-prepared, wu/resample.py); 64 bytes
    long long src_off;               // element offset of pixel (0, 0), channel 0
    long long s_row, s_col, s_ch;    // element strides
    int src_h, src_w;
    int hb, hk;                      // byte offsets in the workspace: horizontal bounds int[Wout][2] = {xmin, count}, coefficients [kx][Wout]
    int vb, vk;                      // vertical bounds int[Hout][2] = {ymin, count}, coefficients [Hout][ky]
    int kx, ky;                      // taps per output coordinate (Resample.c ksize); 0 = the pass is skipped (equal sizes)
};

template <int MODE> struct Acc { typedef double type; typedef float mid; };
template <> struct Acc<MODE_U8> { typedef int type; typedef int mid; };
// what a staged source row holds: bytes, except for a float source in float mode
template <int MODE, int SRC> struct Staged { typedef uint8_t type; };
template <> struct Staged<MODE_F32, SRC_F32> { typedef float type; };
template <> struct Staged<MODE_F32, SRC_BF16> { typedef float type; };

WU_HD int clip8(int v) {
    v >>= kPrec;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
WU_HD float clipf(float v) { return v > 0.f ? (v < 255.f ? v : 255.f) : 0.f; }

// one source sample on the 0..255 scale: float32 with two roundings for (-1, 1); quantised as wu.infer_driver.to_uint8 (truncation) in
// 8-bit mode
template <int MODE, int SRC>
WU_HD typename Staged<MODE, SRC>::type sample(const void* src, long long i, int vr) {
    typedef typename Staged<MODE, SRC>::type ST;
    if constexpr (SRC == SRC_U8) {
        return ((const uint8_t*)src)[i];
    } else {
        float x;
        if constexpr (SRC == SRC_F32) x = ((const float*)src)[i];
        else x = bf16_to_f32(((const bf16_t*)src)[i]);
        const float t = vr ? x * 127.5f + 127.5f : x * 255.0f;
        if constexpr (MODE == MODE_U8) return (ST)(int)clipf(t);
        else return t;
    }
}

// step 1: source row sy of image d into `stage` ([src_w][3]); every thread of the workgroup takes part
template <int MODE, int SRC>
WU_HD void stage_row(typename Staged<MODE, SRC>::type* stage, const void* src, const ResDesc& d, int sy, int vr, int tid, int nthreads) {
    for (int c = 0; c < 3; ++c) {
        const long long base = d.src_off + (long long)sy * d.s_row + (long long)c * d.s_ch;
        for (int x = tid; x < d.src_w; x += nthreads) stage[x * 3 + c] = sample<MODE, SRC>(src, base + (long long)x * d.s_col, vr);
    }
}

// step 2: ImagingResampleHorizontal for one output column of one row.  hk points at this column's first tap; taps are `ld` apart
template <int MODE, typename ST>
WU_HD void filter_row(const ST* stage, const typename Acc<MODE>::type* hk, int ld, int xmin, int xn, typename Acc<MODE>::mid* v) {
    typedef typename Acc<MODE>::type A;
    A h0 = MODE == MODE_U8 ? (A)(1 << (kPrec - 1)) : (A)0, h1 = h0, h2 = h0;
    const ST* p = stage + (size_t)xmin * 3;
    for (int k = 0; k < xn; ++k) {
        const A w = hk[(size_t)k * ld];
        h0 += (A)p[3 * k] * w;
        h1 += (A)p[3 * k + 1] * w;
        h2 += (A)p[3 * k + 2] * w;
    }
    if (MODE == MODE_U8) { v[0] = clip8((int)h0); v[1] = clip8((int)h1); v[2] = clip8((int)h2); }
    else { v[0] = (typename Acc<MODE>::mid)h0; v[1] = (typename Acc<MODE>::mid)h1; v[2] = (typename Acc<MODE>::mid)h2; }     // float64 -> float32
}

// step 3: ImagingResampleVertical, streamed: source row sy into the accumulators of the band's rows that are live there
template <int MODE>
WU_HD void accumulate(typename Acc<MODE>::type (*acc)[kBandMax], const typename Acc<MODE>::mid* v, int sy, const int* ymin, const int* ycnt,
                      const typename Acc<MODE>::type* vk, int ky, int oy0) {
    typedef typename Acc<MODE>::type A;
#pragma unroll
    for (int j = 0; j < kBandMax; ++j) {
        const int r = sy - ymin[j];
        if (r < 0 || r >= ycnt[j]) continue;                   // the same for every thread of the workgroup
        if (ky > 0) {
            const A w = vk[(size_t)(oy0 + j) * ky + r];
            acc[0][j] += (A)v[0] * w; acc[1][j] += (A)v[1] * w; acc[2][j] += (A)v[2] * w;
        } else {                                               // no vertical pass: the row itself
            acc[0][j] = (A)v[0]; acc[1][j] = (A)v[1]; acc[2][j] = (A)v[2];
        }
    }
}

#ifdef WU_RESAMPLE_EMU
inline void store4(float* p, const float* q) { for (int e = 0; e < 4; ++e) p[e] = q[e]; }
inline void store4(bf16_t* p, const float* q) { for (int e = 0; e < 4; ++e) p[e] = f32_to_bf16(q[e]); }
#else
__device__ __forceinline__ void store4(float* p, const float* q) { *(float4*)p = make_float4(q[0], q[1], q[2], q[3]); }
__device__ __forceinline__ void store4(bf16_t* p, const float* q) { *(uint2*)p = make_uint2(pack_bf16x2(q[0], q[1]), pack_bf16x2(q[2], q[3])); }
#endif

struct Out {
    void* dst;
    int epi, normalize, ldy, cpad, bf16;
};

// one output pixel: `val` is Pillow's result (8-bit mode: 0..255; float mode: unclipped float32)
WU_HD void epilogue(const Out& o, const float* val, int n, int oy, int ox, int Hout, int Wout) {
    const size_t pix = ((size_t)n * Hout + oy) * Wout + ox;
    if (o.epi == EPI_NHWC_U8) {
        uint8_t* q = (uint8_t*)o.dst + pix * 3;
        q[0] = (uint8_t)val[0]; q[1] = (uint8_t)val[1]; q[2] = (uint8_t)val[2];
        return;
    }
    float u[3];
    for (int c = 0; c < 3; ++c) {
        u[c] = val[c];
        if (o.epi != EPI_RAW) u[c] = clipf(u[c]) / 255.0f;
        if (o.epi == EPI_NORM) u[c] = (u[c] - 0.5f) / 0.5f;
        if (o.epi == EPI_INCEPTION && o.normalize) u[c] = (float)(2.0 * (double)u[c] - 1.0);        // inception_input_kernel's 2x - 1
    }
    if (o.epi != EPI_INCEPTION) {
        const size_t plane = (size_t)Hout * Wout;
        float* q = (float*)o.dst + (size_t)n * 3 * plane + (size_t)oy * Wout + ox;
        q[0] = u[0]; q[plane] = u[1]; q[2 * plane] = u[2];
        return;
    }
    // the network input: cpad channels (a multiple of 4) per pixel, 3.. zero, four at a time
    for (int c0 = 0; c0 < o.cpad; c0 += 4) {
        const float q[4] = {c0 ? 0.f : u[0], c0 ? 0.f : u[1], c0 ? 0.f : u[2], 0.f};
        if (o.bf16) store4((bf16_t*)o.dst + pix * o.ldy + c0, q);
        else store4((float*)o.dst + pix * o.ldy + c0, q);
    }
}

// the rows of a band: ymin / ycnt of each of its output rows (ycnt 0 beyond the band) and the source rows [ylo, yhi) it walks.  The
// clamps keep every index inside the image whatever a table holds.
WU_HD void band_rows(const ResDesc& d, const int* vb, int oy0, int nrows, int* ymin, int* ycnt, int& ylo, int& yhi) {
    ylo = d.src_h;
    yhi = 0;
#pragma unroll
    for (int j = 0; j < kBandMax; ++j) {
        ymin[j] = 0;
        ycnt[j] = 0;
        if (j >= nrows) continue;
        int y0 = d.ky > 0 ? vb[(oy0 + j) * 2] : oy0 + j, cnt = d.ky > 0 ? vb[(oy0 + j) * 2 + 1] : 1;
        y0 = y0 < 0 ? 0 : (y0 > d.src_h - 1 ? d.src_h - 1 : y0);
        if (d.ky > 0 && cnt > d.ky) cnt = d.ky;
        if (cnt > d.src_h - y0) cnt = d.src_h - y0;
        if (cnt < 0) cnt = 0;
        ymin[j] = y0;
        ycnt[j] = cnt;
        if (y0 < ylo) ylo = y0;
        if (y0 + cnt > yhi) yhi = y0 + cnt;
    }
}

// a column's taps: {xmin, count} of output column ox, clamped into the row as above
WU_HD void column_taps(const ResDesc& d, const int* hb, int ox, int& xmin, int& xn) {
    xmin = hb[ox * 2];
    xn = hb[ox * 2 + 1];
    xmin = xmin < 0 ? 0 : (xmin > d.src_w - 1 ? d.src_w - 1 : xmin);
    if (xn > d.kx) xn = d.kx;
    if (xn > d.src_w - xmin) xn = d.src_w - xmin;
    if (xn < 0) xn = 0;
}

template <int MODE>
WU_HD void finish(const typename Acc<MODE>::type (*acc)[kBandMax], int j, int ky, float* val) {
    for (int c = 0; c < 3; ++c) {
        if (MODE == MODE_U8) val[c] = (float)(ky > 0 ? clip8((int)acc[c][j]) : (int)acc[c][j]);
        else val[c] = (float)acc[c][j];                        // float64 -> float32, once per pass
    }
}

#ifndef WU_RESAMPLE_EMU
template <int MODE, int SRC>
__global__ __launch_bounds__(kMaxOut) void resample_kernel(const void* __restrict__ src, const unsigned char* __restrict__ ws, int Hout, int Wout,
                                                           int band, int vr, int max_stage_w, Out out) {
    typedef typename Acc<MODE>::type A;
    typedef typename Acc<MODE>::mid M;
    typedef typename Staged<MODE, SRC>::type ST;
    extern __shared__ __align__(16) unsigned char lds[];
    ST* stage = (ST*)lds;
    const int n = blockIdx.y, oy0 = blockIdx.x * band, tid = threadIdx.x, nthreads = blockDim.x;
    if (oy0 >= Hout) return;
    const ResDesc d = ((const ResDesc*)ws)[n];
    if (d.kx > 0 && d.src_w > max_stage_w) return;             // the host checked it; LDS holds max_stage_w pixels
    const int nrows = Hout - oy0 < band ? Hout - oy0 : band;
    int ymin[kBandMax], ycnt[kBandMax], ylo, yhi;
    band_rows(d, (const int*)(ws + d.vb), oy0, nrows, ymin, ycnt, ylo, yhi);
    const bool live = tid < Wout;
    const int ox = live ? tid : 0;
    int xmin = 0, xn = 0;
    if (d.kx > 0) column_taps(d, (const int*)(ws + d.hb), ox, xmin, xn);
    const A* hk = (const A*)(ws + d.hk) + ox;
    const A* vk = (const A*)(ws + d.vk);
    A acc[3][kBandMax];
#pragma unroll
    for (int j = 0; j < kBandMax; ++j) acc[0][j] = acc[1][j] = acc[2][j] = MODE == MODE_U8 && d.ky > 0 ? (A)(1 << (kPrec - 1)) : (A)0;
    for (int sy = ylo; sy < yhi; ++sy) {
        M v[3] = {0, 0, 0};
        if (d.kx > 0) {
            __syncthreads();                                   // the row before this one has been read
            stage_row<MODE, SRC>(stage, src, d, sy, vr, tid, nthreads);
            __syncthreads();
            if (live) filter_row<MODE, ST>(stage, hk, Wout, xmin, xn, v);
        } else if (live) {
            const long long base = d.src_off + (long long)sy * d.s_row + (long long)ox * d.s_col;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (M)sample<MODE, SRC>(src, base + (long long)c * d.s_ch, vr);
        }
        if (live) accumulate<MODE>(acc, v, sy, ymin, ycnt, vk, d.ky, oy0);
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < kBandMax; ++j) {
        if (j >= nrows) continue;
        float val[3];
        finish<MODE>(acc, j, d.ky, val);
        epilogue(out, val, n, oy0 + j, ox, Hout, Wout);
    }
}
#endif  // WU_RESAMPLE_EMU

}  // namespace

#ifndef WU_RESAMPLE_EMU
extern "C" size_t wu_resample_desc_bytes(void) { return sizeof(ResDesc); }

extern "C" int wu_resample_max_band(void) { return kBandMax; }

extern "C" size_t wu_resample_workspace_bytes(int N, size_t table_bytes) {
    if (N <= 0) return 0;
    return (size_t)N * sizeof(ResDesc) + ((table_bytes + 15) & ~(size_t)15);
}

extern "C" int wu_resample(const void* src, int src_kind, const void* descs_host, const void* workspace, size_t workspace_bytes, int N, int Hout,
                           int Wout, void* dst, int ldy, int cpad, int dst_dtype, int flags, void* stream) {
    const int mode = flags & WU_RESAMPLE_MODE_U8 ? MODE_U8 : MODE_F32, epi = (flags >> 4) & 15, band_arg = (flags >> 8) & 255;
    const int normalize = (flags >> 16) & 1, vr = (flags >> 17) & 1;
    WU_REQUIRE(src && descs_host && workspace && dst, "wu_resample: null argument");
    WU_REQUIRE(src_kind == SRC_U8 || src_kind == SRC_F32 || src_kind == SRC_BF16, "wu_resample: source kind %d", src_kind);
    WU_REQUIRE(N > 0 && N <= 65535 && Hout > 0 && Wout > 0, "wu_resample: bad shape N=%d -> %d x %d", N, Hout, Wout);
    WU_REQUIRE(Hout <= kMaxOut && Wout <= kMaxOut, "wu_resample: the output side is at most %d (one thread per output column, one workgroup per "
               "band of rows), got %d x %d", kMaxOut, Hout, Wout);
    WU_REQUIRE((long long)N * Hout * Wout < (1ll << 31), "wu_resample: N*Hout*Wout must stay below 2^31");
    WU_REQUIRE(epi <= EPI_INCEPTION, "wu_resample: epilogue %d", epi);
    WU_REQUIRE(epi != EPI_NHWC_U8 || mode == MODE_U8, "wu_resample: the uint8 output needs the 8-bit mode");
    WU_REQUIRE(band_arg <= kBandMax, "wu_resample: band height %d (1..%d, 0 = default)", band_arg, kBandMax);
    const int band = band_arg ? band_arg : kBandMax;
    if (epi == EPI_INCEPTION) {
        WU_REQUIRE(dst_dtype == WU_F32 || dst_dtype == WU_BF16, "wu_resample: dtype %d", dst_dtype);
        WU_REQUIRE(cpad >= 4 && cpad % 4 == 0 && ldy >= cpad && ldy % 4 == 0, "wu_resample: cpad %d (>= 4, multiple of 4) / ldy %d", cpad, ldy);
        WU_REQUIRE(((uintptr_t)dst & 15) == 0, "wu_resample: unaligned network input");
    }
    WU_REQUIRE(workspace_bytes >= (size_t)N * sizeof(ResDesc), "wu_resample: workspace too small");
    // the descriptors, checked on the host before anything touches the device: sizes, and every table inside the workspace
    const ResDesc* dh = (const ResDesc*)descs_host;
    const size_t ksz = mode == MODE_U8 ? sizeof(int) : sizeof(double);
    int max_stage_w = 0;
    for (int n = 0; n < N; ++n) {
        const ResDesc& d = dh[n];
        WU_REQUIRE(d.src_h > 0 && d.src_w > 0 && d.kx >= 0 && d.ky >= 0, "wu_resample: image %d: size %d x %d, taps %d / %d", n, d.src_h, d.src_w, d.kx, d.ky);
        WU_REQUIRE(d.kx > 0 || d.src_w == Wout, "wu_resample: image %d: no horizontal pass, but width %d != %d", n, d.src_w, Wout);
        WU_REQUIRE(d.ky > 0 || d.src_h == Hout, "wu_resample: image %d: no vertical pass, but height %d != %d", n, d.src_h, Hout);
        if (d.kx > 0) {
            WU_REQUIRE(d.hb >= 0 && d.hb % 4 == 0 && (size_t)d.hb + (size_t)Wout * 8 <= workspace_bytes && d.hk >= 0 && d.hk % 8 == 0 &&
                       (size_t)d.hk + (size_t)d.kx * Wout * ksz <= workspace_bytes, "wu_resample: image %d: horizontal tables outside the workspace", n);
            if (d.src_w > max_stage_w) max_stage_w = d.src_w;
        }
        if (d.ky > 0)
            WU_REQUIRE(d.vb >= 0 && d.vb % 4 == 0 && (size_t)d.vb + (size_t)Hout * 8 <= workspace_bytes && d.vk >= 0 && d.vk % 8 == 0 &&
                       (size_t)d.vk + (size_t)d.ky * Hout * ksz <= workspace_bytes, "wu_resample: image %d: vertical tables outside the workspace", n);
    }
    const size_t stage_elem = (mode == MODE_F32 && src_kind != SRC_U8) ? sizeof(float) : 1;
    const size_t lds = (size_t)max_stage_w * 3 * stage_elem;
    WU_REQUIRE(lds <= kMaxLds, "wu_resample: a source row of %d pixels needs %zu bytes of LDS, at most %zu (%zu pixels)", max_stage_w, lds, kMaxLds,
               kMaxLds / (3 * stage_elem));
    Out o;
    o.dst = dst; o.epi = epi; o.normalize = normalize; o.ldy = ldy; o.cpad = cpad; o.bf16 = dst_dtype == WU_BF16;
    const dim3 grid((unsigned)cdiv(Hout, band), (unsigned)N), block((unsigned)(cdiv(Wout, 64) * 64));
    hipStream_t s = (hipStream_t)stream;
    const unsigned char* ws = (const unsigned char*)workspace;
#define WU_RS_LAUNCH(M, S) hipLaunchKernelGGL((resample_kernel<M, S>), grid, block, lds, s, src, ws, Hout, Wout, band, vr, max_stage_w, o)
    if (mode == MODE_U8) {
        if (src_kind == SRC_U8) WU_RS_LAUNCH(MODE_U8, SRC_U8);
        else if (src_kind == SRC_F32) WU_RS_LAUNCH(MODE_U8, SRC_F32);
        else WU_RS_LAUNCH(MODE_U8, SRC_BF16);
    } else {
        if (src_kind == SRC_U8) WU_RS_LAUNCH(MODE_F32, SRC_U8);
        else if (src_kind == SRC_F32) WU_RS_LAUNCH(MODE_F32, SRC_F32);
        else WU_RS_LAUNCH(MODE_F32, SRC_BF16);
    }
#undef WU_RS_LAUNCH
    WU_LAUNCH_CHECK("resample_kernel");
    return 0;
}
#endif  // WU_RESAMPLE_EMU
