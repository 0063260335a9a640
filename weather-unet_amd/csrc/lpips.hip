// LPIPS (Zhang et al. 2018, net = alex, version 0.1): the two ends around the AlexNet trunk, which runs on wu_conv_kxk_fwd / wu_pool3x3_fwd
// (tests/_lpips_ref.py states the arithmetic).
//   * lpips_input_kernel   one thread per pixel: the 3 source values through the source's strides (NCHW, channels-last, a crop, a row of the
//                          sweep's (R, B, ...) output, uint8 NHWC as a permuted view), the scaling layer in float32 with every operation rounded
//                          on its own, 16 channels of the NHWC network input stored (3 values, 13 zeros);
//   * lpips_dist_kernel    one layer's head.  16 lanes share a pixel, lane l of them owns channels 64 j + 4 l .. + 3 (one 16-byte load of fp32,
//                          8 bytes of bf16); a 256-thread workgroup owns kLpTile = 16 pixels of one image.  The x vector is read, widened to fp64
//                          and unit-normalised ONCE and stays in registers while the rows of y walk past: per row the y vector is normalised,
//                          sum_c w_c (xh_c - yh_c)^2 is formed per lane in channel order, folded over the 16 lanes, then over the wave's 4
//                          pixels; lane 0 of each wave stores that partial sum in its own workspace slot.  For the pair matrix the kept
//                          vectors are a block of 4 / 2 / 1 rows i of the same tensor (by C: what the registers hold) and the rows walked are
//                          the j behind them: a row j is normalised once per block and meets every kept i < j; pair (i, j) is formed exactly
//                          as the head forms (x = row i, y = row j), from direct differences, so it does not depend on the blocking;
//   * lpips_fold_kernel    one wave per output: lane l adds slots l, l + 64, .. in that order, the lanes are summed in wave_sum_f64's order,
//                          the sum is divided by h w; the pairs variant also writes the mirrored entry and the zero diagonal.
// No atomics, no LDS, every reduction in a fixed order that depends neither on B nor on R: two runs, and any split of the rows or images
// into several calls, give the same bits.
#include "gram_f64.h"

// every product, sum, quotient and square root is rounded on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kLpLanes = 16;                 // lanes that share a pixel
constexpr int kLpTile = 16;                  // pixels of a workgroup: 4 waves x 4 pixels
constexpr int kLpWaves = 4;                  // one partial-sum slot each
constexpr int kLpChunk = 4 * kLpLanes;       // channels the 16 lanes cover per step
constexpr int kLpMaxC = 512;
constexpr int kLpMaxRows = 64;               // pairs: R * R slots per (image, tile)

struct LpInputArgs {
    const void* src;
    long long s[4];              // element strides (n, c, h, w)
    int N, H, W;
    float scale, offset;
    void* dst;                   // (N, H, W, 16)
};

template <int SDT> __device__ __forceinline__ float lp_src(const void* p, long long at) {
    if (SDT == WU_BF16) return bf16_to_f32(((const bf16_t*)p)[at]);
    if (SDT == WU_LPIPS_U8) return (float)((const unsigned char*)p)[at];
    return ((const float*)p)[at];
}

template <int SDT, typename TO> __global__ __launch_bounds__(256) void lpips_input_kernel(const LpInputArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)a.H * a.W;
    if (idx >= per * a.N) return;
    const long long n = idx / per, hw = idx - n * per;
    const int i = (int)(hw / a.W), j = (int)(hw - (long long)i * a.W);
    const long long base = n * a.s[0] + i * a.s[2] + j * a.s[3];
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scl[3] = {0.458f, 0.448f, 0.450f};
    float u[16];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = lp_src<SDT>(a.src, base + c * a.s[1]) * a.scale;
        t = t + a.offset;
        t = t - shift[c];
        u[c] = t / scl[c];
    }
#pragma unroll
    for (int c = 3; c < 16; ++c) u[c] = 0.f;
    constexpr int per16 = ElemTraits<TO>::kPer16B;
    uint4* out = (uint4*)((TO*)a.dst + idx * 16);
#pragma unroll
    for (int q = 0; q < 16 / per16; ++q) out[q] = pack16<TO>(u + q * per16);
}

struct LpDistArgs {
    const void* x;               // (B, h, w, C) ld = ldx; with PAIRS: unused
    const void* y;               // (R, B, h, w, C) ld = ldy, rows row_stride elements apart
    const float* weight;
    long long row_stride;
    int ldx, ldy, B, R, hw, C, tiles;
    double* partial;             // head: (R, B, tiles, waves); pairs: (R, R, B, tiles, waves)
};

// 4 consecutive channels of a pixel, widened
template <typename T> __device__ __forceinline__ void lp_load4(const T* p, double* v);
template <> __device__ __forceinline__ void lp_load4<float>(const float* p, double* v) {
    const float4 f = *(const float4*)p;
    v[0] = (double)f.x, v[1] = (double)f.y, v[2] = (double)f.z, v[3] = (double)f.w;
}
template <> __device__ __forceinline__ void lp_load4<bf16_t>(const bf16_t* p, double* v) {
    const uint2 f = *(const uint2*)p;
    v[0] = (double)__uint_as_float(f.x << 16), v[1] = (double)__uint_as_float(f.x & 0xffff0000u);
    v[2] = (double)__uint_as_float(f.y << 16), v[3] = (double)__uint_as_float(f.y & 0xffff0000u);
}

// sum over the 16 lanes of a pixel; every lane ends with the same bits (both partners of a step add the same two numbers)
__device__ __forceinline__ double lp_sum16(double v) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// the lane's channels of one pixel's feature vector, divided by (the vector's norm + 1e-10); channels past C are zero
template <typename T, int NCH> __device__ __forceinline__ void lp_unit(const T* pix, int C, int l16, double (&v)[NCH * 4]) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = kLpChunk * j + 4 * l16;
        if (c < C) lp_load4<T>(pix + c, &v[4 * j]);
        else v[4 * j] = v[4 * j + 1] = v[4 * j + 2] = v[4 * j + 3] = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) s = s + v[4 * j + e] * v[4 * j + e];
    }
    const double den = sqrt(lp_sum16(s)) + 1e-10;
#pragma unroll
    for (int k = 0; k < NCH * 4; ++k) v[k] = v[k] / den;
}

// rows i a pairs workgroup keeps in registers, by the instance's channel steps: 4 up to C = 128, 2 up to C = 256, 1 above (register budget)
constexpr int lp_iblock(int nch) { return nch <= 2 ? 4 : nch <= 4 ? 2 : 1; }

// IB = 0: the head, grid (tiles, B, 1).  IB >= 1: pairs, grid (tiles, B, ceil((R - 1) / IB)): the workgroup keeps rows i0 .. i0 + IB - 1 in
// registers and walks the rows j > i0 past them; each row j is read and normalised once per workgroup and meets every kept row i < j.
template <typename T, int NCH, int IB> __global__ __launch_bounds__(256) void lpips_dist_kernel(const LpDistArgs a) {
    constexpr bool PAIRS = IB > 0;
    constexpr int NI = PAIRS ? IB : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15;
    const int tile = blockIdx.x, b = blockIdx.y, i0 = PAIRS ? (int)blockIdx.z * IB : 0;
    const int p = tile * kLpTile + (tid >> 4);
    const bool valid = p < a.hw;
    const int pc = valid ? p : a.hw - 1;         // a pixel past the end reads the last one and contributes nothing
    double wv[NCH * 4], xh[NI][NCH * 4], yh[NCH * 4];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = kLpChunk * j + 4 * l16;
        float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < a.C) f = *(const float4*)(a.weight + c);
        wv[4 * j] = (double)f.x, wv[4 * j + 1] = (double)f.y, wv[4 * j + 2] = (double)f.z, wv[4 * j + 3] = (double)f.w;
    }
    const long long ypix = ((long long)b * a.hw + pc) * a.ldy;
#pragma unroll
    for (int ii = 0; ii < NI; ++ii) {
        // a kept row past the last one that has a partner (i > R - 2) reads row R - 1 and is never used: every j <= R - 1 <= i
        const int row = min(i0 + ii, a.R - 1);
        const T* xp = PAIRS ? (const T*)a.y + row * a.row_stride + ypix : (const T*)a.x + ((long long)b * a.hw + pc) * a.ldx;
        lp_unit<T, NCH>(xp, a.C, l16, xh[ii]);
    }
    for (int r = PAIRS ? i0 + 1 : 0; r < a.R; ++r) {
        lp_unit<T, NCH>((const T*)a.y + r * a.row_stride + ypix, a.C, l16, yh);
#pragma unroll
        for (int ii = 0; ii < NI; ++ii) {
            const int i = i0 + ii;
            if (PAIRS && i >= r) continue;       // uniform over the workgroup
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NCH * 4; ++k) {
                const double d = xh[ii][k] - yh[k];
                s = s + wv[k] * (d * d);
            }
            s = lp_sum16(s);
            s = valid ? s : 0.0;
            s = s + __shfl_xor(s, 16, 64);       // the wave's 4 pixels
            s = s + __shfl_xor(s, 32, 64);
            if (lane == 0) {
                const long long rb = PAIRS ? ((long long)i * a.R + r) * a.B + b : (long long)r * a.B + b;
                a.partial[(rb * a.tiles + tile) * kLpWaves + wave] = s;
            }
        }
    }
}

struct LpFoldArgs {
    const double* partial;
    int B, R, slots, ldo;
    double hw;
    double* out;
};

// one wave per (r, b) [head] or (i, j, b) [pairs]
template <bool PAIRS> __global__ __launch_bounds__(64) void lpips_fold_kernel(const LpFoldArgs a) {
    const long long id = blockIdx.x;
    const int lane = threadIdx.x;
    const int b = (int)(id % a.B);
    const long long rr = id / a.B;
    int i = 0, j = 0;
    if (PAIRS) {
        i = (int)(rr / a.R), j = (int)(rr % a.R);
        if (i > j) return;                       // written by (j, i)
        if (i == j) {
            if (lane == 0) a.out[((long long)i * a.R + j) * a.ldo + b] = 0.0;
            return;
        }
    }
    const double* p = a.partial + id * a.slots;
    double s = 0.0;
    for (int t = lane; t < a.slots; t += 64) s = s + p[t];
    s = wave_sum_f64(s);
    if (lane == 0) {
        const double d = s / a.hw;
        if (PAIRS) {
            a.out[((long long)i * a.R + j) * a.ldo + b] = d;
            a.out[((long long)j * a.R + i) * a.ldo + b] = d;
        } else {
            a.out[rr * a.ldo + b] = d;
        }
    }
}

bool lp_shape_ok(int B, int R, int h, int w, int pairs) {
    if (B < 1 || B > 65535 || R < 1 || h < 1 || w < 1 || (long long)h * w > (1ll << 24)) return false;
    if (pairs && (R < 2 || R > kLpMaxRows)) return false;
    const long long outs = (long long)(pairs ? R : 1) * R * B;
    return outs < (1ll << 31) && outs * cdiv(h * w, kLpTile) * kLpWaves < (1ll << 40);
}

template <typename T, bool PAIRS> int lp_launch(const LpDistArgs& a, hipStream_t s) {
    const int nch = cdiv(a.C, kLpChunk);
    const dim3 grid((unsigned)a.tiles, (unsigned)a.B, PAIRS ? (unsigned)cdiv(a.R - 1, lp_iblock(nch)) : 1u);
    switch (nch) {
#define WU_LP_CASE(n) \
    case n: hipLaunchKernelGGL((lpips_dist_kernel<T, n, PAIRS ? lp_iblock(n) : 0>), grid, dim3(256), 0, s, a); break;
        WU_LP_CASE(1) WU_LP_CASE(2) WU_LP_CASE(3) WU_LP_CASE(4) WU_LP_CASE(5) WU_LP_CASE(6) WU_LP_CASE(7) WU_LP_CASE(8)
#undef WU_LP_CASE
    default: WU_FAIL(-1, "wu_lpips: C %d out of range", a.C);
    }
    WU_LAUNCH_CHECK("lpips_dist_kernel");
    return 0;
}

int lp_run(const void* fx, int ldx, const void* fy, int ldy, long long row_stride, const float* weight, int dtype, int B, int R, int h, int w,
           int C, void* workspace, double* out, int ldo, bool pairs, void* stream) {
    const char* who = pairs ? "wu_lpips_pairs" : "wu_lpips_head";
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "%s: dtype %d must be WU_F32 or WU_BF16", who, dtype);
    WU_REQUIRE(lp_shape_ok(B, R, h, w, pairs), "%s: B %d R %d h %d w %d out of range (B <= 65535, h w <= 2^24%s)", who, B, R, h, w,
               pairs ? ", 2 <= R <= 64" : "");
    WU_REQUIRE(C >= 16 && C <= kLpMaxC && C % 16 == 0, "%s: C %d must be a multiple of 16 in 16..%d", who, C, kLpMaxC);
    WU_REQUIRE(ldy >= C && ldy % 8 == 0 && (pairs || (ldx >= C && ldx % 8 == 0)), "%s: ld %d / %d must be multiples of 8, at least C %d", who,
               ldx, ldy, C);
    WU_REQUIRE(fy && weight && workspace && out && (pairs || fx), "%s: NULL pointer", who);
    WU_REQUIRE(((uintptr_t)fy % 16 == 0) && ((uintptr_t)fx % 16 == 0) && ((uintptr_t)weight % 16 == 0) && row_stride % 8 == 0,
               "%s: features and weight must be 16-byte aligned, the row stride a multiple of 8", who);
    WU_REQUIRE(ldo >= B, "%s: ldo %d must be at least B %d", who, ldo, B);
    hipStream_t s = (hipStream_t)stream;
    LpDistArgs a;
    a.x = fx, a.y = fy, a.weight = weight, a.row_stride = row_stride;
    a.ldx = ldx, a.ldy = ldy, a.B = B, a.R = R, a.hw = h * w, a.C = C;
    a.tiles = cdiv(h * w, kLpTile);
    a.partial = (double*)workspace;
    int rc;
    if (pairs) rc = dtype == WU_F32 ? lp_launch<float, true>(a, s) : lp_launch<bf16_t, true>(a, s);
    else rc = dtype == WU_F32 ? lp_launch<float, false>(a, s) : lp_launch<bf16_t, false>(a, s);
    if (rc) return rc;
    LpFoldArgs f;
    f.partial = a.partial, f.B = B, f.R = R, f.slots = a.tiles * kLpWaves, f.ldo = ldo, f.hw = (double)(h * w), f.out = out;
    const unsigned outs = (unsigned)((long long)(pairs ? R : 1) * R * B);
    if (pairs) hipLaunchKernelGGL(lpips_fold_kernel<true>, dim3(outs), dim3(64), 0, s, f);
    else hipLaunchKernelGGL(lpips_fold_kernel<false>, dim3(outs), dim3(64), 0, s, f);
    WU_LAUNCH_CHECK("lpips_fold_kernel");
    return 0;
}

template <int SDT> void lp_launch_input(const LpInputArgs& a, int dtype, unsigned grid, hipStream_t s) {
    if (dtype == WU_F32) hipLaunchKernelGGL((lpips_input_kernel<SDT, float>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((lpips_input_kernel<SDT, bf16_t>), dim3(grid), dim3(256), 0, s, a);
}

}  // namespace

extern "C" int wu_lpips_tile_pixels(void) { return kLpTile; }

extern "C" size_t wu_lpips_workspace_bytes(int B, int R, int h, int w, int pairs) {
    if (!lp_shape_ok(B, R, h, w, pairs)) return 0;
    return (size_t)(pairs ? R : 1) * R * B * cdiv(h * w, kLpTile) * kLpWaves * sizeof(double);
}

extern "C" int wu_lpips_input(const void* src, long long s_n, long long s_c, long long s_h, long long s_w, int src_dtype, int N, int H, int W,
                              float scale, float offset, void* dst, int dtype, void* stream) {
    WU_REQUIRE(src_dtype == WU_F32 || src_dtype == WU_BF16 || src_dtype == WU_LPIPS_U8, "wu_lpips_input: unknown source dtype %d", src_dtype);
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "wu_lpips_input: dtype %d must be WU_F32 or WU_BF16", dtype);
    WU_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (long long)N * H * W < (1ll << 38), "wu_lpips_input: N %d H %d W %d out of range", N, H, W);
    WU_REQUIRE(src && dst && (uintptr_t)dst % 16 == 0, "wu_lpips_input: NULL source or a destination that is not 16-byte aligned");
    LpInputArgs a;
    a.src = src, a.s[0] = s_n, a.s[1] = s_c, a.s[2] = s_h, a.s[3] = s_w;
    a.N = N, a.H = H, a.W = W, a.scale = scale, a.offset = offset, a.dst = dst;
    const unsigned grid = (unsigned)(((long long)N * H * W + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype == WU_F32) lp_launch_input<WU_F32>(a, dtype, grid, s);
    else if (src_dtype == WU_BF16) lp_launch_input<WU_BF16>(a, dtype, grid, s);
    else lp_launch_input<WU_LPIPS_U8>(a, dtype, grid, s);
    WU_LAUNCH_CHECK("lpips_input_kernel");
    return 0;
}

extern "C" int wu_lpips_head(const void* fx, int ldx, const void* fy, int ldy, long long fy_row_stride, const float* weight, int dtype, int B,
                             int R, int h, int w, int C, void* workspace, double* out, int ldo, void* stream) {
    return lp_run(fx, ldx, fy, ldy, fy_row_stride, weight, dtype, B, R, h, w, C, workspace, out, ldo, false, stream);
}

extern "C" int wu_lpips_pairs(const void* f, int ld, long long row_stride, const float* weight, int dtype, int B, int R, int h, int w, int C,
                              void* workspace, double* out, int ldo, void* stream) {
    return lp_run(nullptr, ld, f, ld, row_stride, weight, dtype, B, R, h, w, C, workspace, out, ldo, true, stream);
}
