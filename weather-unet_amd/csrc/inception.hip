// Kernels of the InceptionV3 forward behind FID / Inception-Score evaluation (the reference's eval/fid_score.py, eval/inception.py,
// eval/inception_score.py: pytorch-fid's FID InceptionV3 and torchvision's Inception3, eval mode, forward only):
//   * conv_kxk_kernel        every conv of the network -- 3x3 (s1 / s2, valid / pad 1), 1x1, 5x5, 1x7 / 7x1, 1x3 / 3x1 and the fc
//                            head as a 1x1 over N x 1 x 1 pixels -- as ONE implicit GEMM on the matrix cores: rows = output pixels,
//                            K = KH * KW * Cin in (tap, channel) order, padding = out-of-range buffer offsets (zeros); folded BatchNorm
//                            bias + ReLU in the register epilogue, stores of the channels < Cout only (Mixed-block concats are channel
//                            slices of one buffer);
//   * pool3x3_kernel         3x3 max / average pools (stride 1 or 2, pad 0 or 1, count_include_pad either way);
//   * global_avgpool_kernel  NHWC -> (N, C) fp32 mean in a fixed order (pool3 and the adaptive_avg_pool2d of fid_score.py);
//   * inception_input_kernel uint8 / fp32 images -> bilinear 299 x 299 (F.interpolate, align_corners=False) -> 2x - 1, NHWC padded;
//   * feature_stats_*        shifted first / second moments of feature rows into fp64 accumulators (mu and sigma of the FID).
// Nothing here uses atomics or a grid-dependent K split: every result is a function of the inputs alone.
#include <algorithm>
#include <type_traits>

#include "wu_common.h"

namespace {

// =================================================================================================
// KH x KW conv = implicit GEMM   y[m][co] = act(sum_k x[pix(m, k)][ci(k)] * w[co][k] + bias[co])
// =================================================================================================
constexpr int kKB = 128;        // bytes of K staged per step and row (64 bf16 / 32 fp32 elements)
constexpr int kTM = 128;        // output pixels per workgroup (4 waves x 32)
constexpr unsigned kOOB = 0x80000000u;

struct KxArgs {
    const void* x; const void* w; const float* bias; void* y;
    int ldx, ldy, H, W, Cin, Ho, Wo, Cout, KW, sh, sw, ph, pw, act;
    int M;                      // output pixels of this launch (images x Ho x Wo)
    int K, Kp;                  // KH * KW * Cin and the packed row length (K rounded up to a whole step)
    int n_ct;                   // cout tiles
    int x_bytes;                // bytes of x this launch may read (the descriptor's range)
};

template <typename T> struct KxMma;
template <> struct KxMma<bf16_t> {
    static __device__ __forceinline__ void run(f32x16_t& acc, const uint4& a, const uint4& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct KxMma<float> {      // exact fp32: four 32x32x2 steps per 16-byte fragment pair (same k permutation on both operands)
    static __device__ __forceinline__ void run(f32x16_t& acc, const uint4& a, const uint4& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
};

// LDS image of one step: 128-byte rows, the eight 16-byte slots XOR-swizzled with ((row >> 1) & 7) (resnet.hip, pw_off: conflict-free
// ds_read_b128 of 32-row fragments)
__device__ __forceinline__ int kx_off(int row, int slot) { return row * kKB + ((slot ^ ((row >> 1) & 7)) << 4); }

// NI = 32-cout blocks per workgroup (tile of 32 * NI couts); each of the 4 waves owns 32 pixels x all NI blocks
template <typename T, int NI>
__global__ __launch_bounds__(256, 2) void conv_kxk_kernel(const KxArgs a) {
    constexpr int TN = 32 * NI;
    constexpr int E16 = 16 / (int)sizeof(T);            // elements per 16-byte slot
    constexpr int KE = kKB / (int)sizeof(T);            // K elements per step
    constexpr int NA = kTM / 32;                        // activation slots per thread and step
    constexpr int kStage = (kTM + TN) * kKB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;

    // cout tile fastest: the workgroups that share one pixel tile are neighbours (same XCD after the remap)
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int ct = bid % a.n_ct;
    const int m0 = (bid / a.n_ct) * kTM;
    const int co0 = ct * TN;

    // ---- staging map: thread = (row srow + 32 k, 16-byte slot sslot) of the step's 128-byte rows ----
    const int srow = tid >> 3, sslot = tid & 7;
    const int HoWo = a.Ho * a.Wo;
    int ih0[NA], iw0[NA], pbase[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int m = m0 + srow + 32 * k;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        const int n = mm / HoWo, r = mm - n * HoWo;
        const int oh = r / a.Wo, ow = r - oh * a.Wo;
        ih0[k] = ok ? oh * a.sh - a.ph : -(1 << 24);     // rows past the GEMM: every tap falls outside the image
        iw0[k] = ow * a.sw - a.pw;
        pbase[k] = n * a.H * a.W;
    }
    // K position of this thread's slot: tap (kh, kw), channel ci -- a slot never straddles two taps (Cin % 16 == 0)
    int kpos = sslot * E16;
    int tap = kpos / a.Cin, ci = kpos - tap * a.Cin;
    int kh = tap / a.KW, kw = tap - kh * a.KW;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, a.x_bytes, 0x00020000);
    const T* wsrc = (const T*)a.w + (size_t)(co0 + srow) * a.Kp + sslot * E16;

    // the weight registers are named, not an array: hipcc parks a small array of uint4 in scratch (resnet.hip notes the same)
    uint4 areg[NA], wreg0, wreg1;
    auto load_step = [&](int step) __attribute__((always_inline)) {
        const bool kin = kpos < a.K;
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int ih = ih0[k] + kh, iw = iw0[k] + kw;
            const bool ok = kin && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
            const unsigned off = ((unsigned)(pbase[k] + ih * a.W + iw) * (unsigned)a.ldx + (unsigned)ci) * (unsigned)sizeof(T);
            areg[k] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)(ok ? off : kOOB), 0, 0));
        }
        wreg0 = *(const uint4*)(wsrc + (size_t)step * KE);
        if constexpr (NI == 2) wreg1 = *(const uint4*)(wsrc + (size_t)32 * a.Kp + (size_t)step * KE);
        // advance to the next step: KE elements further along K (may cross several taps when Cin < KE)
        ci += KE;
        kpos += KE;
        while (ci >= a.Cin) {
            ci -= a.Cin;
            if (++kw == a.KW) { kw = 0; ++kh; }
        }
    };
    auto store_step = [&](int stage) __attribute__((always_inline)) {
        char* a_lds = smem + stage * kStage;
        char* w_lds = a_lds + kTM * kKB;
#pragma unroll
        for (int k = 0; k < NA; ++k) *(uint4*)(a_lds + kx_off(srow + 32 * k, sslot)) = areg[k];
        *(uint4*)(w_lds + kx_off(srow, sslot)) = wreg0;
        if constexpr (NI == 2) *(uint4*)(w_lds + kx_off(srow + 32, sslot)) = wreg1;
    };

    // accumulators transposed (weights are the MFMA A operand): lane = pixel, register 4 g + e = cout 8 g + 4 lh + e of the block
    f32x16_t acc[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

    // two LDS stages, one register set: step s + 1 travels from memory while step s is multiplied
    const int nsteps = a.Kp / KE;
    load_step(0);
    store_step(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) load_step(s + 1);
        const char* a_lds = smem + (s & 1) * kStage;
        const char* w_lds = a_lds + kTM * kKB;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const uint4 xf = *(const uint4*)(a_lds + kx_off(32 * wave + l31, 2 * ks + lh));
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const uint4 wf = *(const uint4*)(w_lds + kx_off(32 * j + l31, 2 * ks + lh));
                KxMma<T>::run(acc[j], wf, xf);
            }
        }
        if (more) {
            // the other stage was last read in step s - 1, which every thread finished before the barrier that published stage s
            store_step((s + 1) & 1);
            __syncthreads();
        }
    }

    // ---- epilogue: fp32 bias, activation, one rounding, stores of the channels < Cout only ----
    const int m = m0 + 32 * wave + l31;
    if (m >= a.M) return;
    T* yp = (T*)a.y + (size_t)m * a.ldy;
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int co = co0 + 32 * j + 8 * g + 4 * lh;
            if (co >= a.Cout) continue;                  // Cout % 16 == 0: a 4-channel group is wholly inside or outside
            float o[4];
            const float4 bv = a.bias ? *(const float4*)(a.bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
            o[0] = acc[j][4 * g + 0] + bv.x; o[1] = acc[j][4 * g + 1] + bv.y;
            o[2] = acc[j][4 * g + 2] + bv.z; o[3] = acc[j][4 * g + 3] + bv.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = act_apply(o[e], a.act);
            if constexpr (std::is_same<T, float>::value) {
                *(float4*)(yp + co) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                *(uint2*)(yp + co) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
            }
        }
}

// packed weight: [roundup(Cout, 64)][Kp], element (co, k = (kh * KW + kw) * Cin + ci) = w_oihw[co][ci][kh][kw] (zero where co >= Cout,
// ci >= Cin_w or k >= K)
template <typename T>
__global__ void pack_kxk_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin_w, int Cin, int KH, int KW, int K, int Kp,
                                long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i / Kp), k = (int)(i - (long long)co * Kp);
    float v = 0.f;
    if (co < Cout && k < K) {
        const int tap = k / Cin, ci = k - tap * Cin;
        const int kh = tap / KW, kw = tap - kh * KW;
        if (ci < Cin_w) v = w[(((size_t)co * Cin_w + ci) * KH + kh) * KW + kw];
    }
    ElemTraits<T>::store(out + i, v);
}

// =================================================================================================
// pools
// =================================================================================================
template <typename T> __device__ __forceinline__ void load4e(const T* p, float* o);
template <> __device__ __forceinline__ void load4e<float>(const float* p, float* o) {
    const float4 v = *(const float4*)p;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <> __device__ __forceinline__ void load4e<bf16_t>(const bf16_t* p, float* o) {
    const uint2 v = *(const uint2*)p;
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void store4e(T* p, const float* o);
template <> __device__ __forceinline__ void store4e<float>(float* p, const float* o) { *(float4*)p = make_float4(o[0], o[1], o[2], o[3]); }
template <> __device__ __forceinline__ void store4e<bf16_t>(bf16_t* p, const float* o) {
    *(uint2*)p = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
}

// one thread = 4 channels of one output pixel; window taps in (kh, kw) row-major order; padding = -inf (max) / 0 (average)
template <typename T>
__global__ void pool3x3_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int H, int W, int Ho, int Wo, int C4,
                               int stride, int pad, int mode, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cg = (int)(i % C4);
    const long long p = i / C4;
    const int ow = (int)(p % Wo);
    const long long t = p / Wo;
    const int oh = (int)(t % Ho);
    const long long n = t / Ho;
    const int h0 = oh * stride - pad, w0 = ow * stride - pad;
    float r[4];
    const bool is_max = mode == WU_POOL_MAX;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = is_max ? -__builtin_huge_valf() : 0.f;
    int cnt = 0;
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = h0 + kh;
        if (ih < 0 || ih >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = w0 + kw;
            if (iw < 0 || iw >= W) continue;
            float v[4];
            load4e<T>(x + ((n * H + ih) * W + iw) * ldx + 4 * cg, v);
            ++cnt;
            if (is_max) {
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] += v[e];
            }
        }
    }
    if (!is_max) {
        const float div = mode == WU_POOL_AVG ? 9.f : (float)cnt;     // stride 1, pad 1: a padded window always spans 9 sites
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] /= div;
    }
    store4e<T>(y + p * ldy + 4 * cg, r);
}

// global average pool: block = (image n, 64 channels); thread (pixel lane pl < 16, channel group cg < 16) sums pixels pl, pl + 16, ...
// in fp64, the 16 lanes are folded in lane order: a fixed summation order for every launch geometry of the same shape
template <typename T>
__global__ __launch_bounds__(256) void global_avgpool_kernel(const T* __restrict__ x, int ldx, float* __restrict__ out, int ldo, int HW, int C) {
    __shared__ double part[16][64];
    const int tid = threadIdx.x, cg = tid & 15, pl = tid >> 4;
    const int n = blockIdx.y, c = blockIdx.x * 64 + 4 * cg;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < C) {
        const T* xp = x + (size_t)n * HW * ldx + c;
        for (int p = pl; p < HW; p += 16) {
            float v[4];
            load4e<T>(xp + (size_t)p * ldx, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) part[pl][4 * cg + e] = s[e];
    __syncthreads();
    if (tid < 64 && blockIdx.x * 64 + tid < C) {
        double t = 0.0;
        for (int l = 0; l < 16; ++l) t += part[l][tid];
        out[(size_t)n * ldo + blockIdx.x * 64 + tid] = (float)(t / (double)HW);
    }
}

// =================================================================================================
// input: images -> [affine] -> bilinear resize (align_corners=False) -> [2x - 1] -> NHWC, channels zero-padded to cpad
// =================================================================================================
// PyTorch's area_pixel_compute_source_index (linear, align_corners=False) in double: the source positions of the float64 F.interpolate
// exactly (an fp32 position near column 500 is off by up to 3e-5 of a pixel), one rounding of the blended value to fp32
__device__ __forceinline__ double src_index(double scale, int dst) {
    const double s = scale * ((double)dst + 0.5) - 0.5;
    return s < 0.0 ? 0.0 : s;
}

template <typename T>
__global__ void inception_input_kernel(const void* __restrict__ src, int src_u8, int Hin, int Win, float in_scale, float in_shift, int affine,
                                       int normalize, T* __restrict__ y, int ldy, int Ho, int Wo, int cpad, double sch, double scw, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ow = (int)(i % Wo);
    const long long t = i / Wo;
    const int oh = (int)(t % Ho);
    const long long n = t / Ho;
    const double fh = src_index(sch, oh), fw = src_index(scw, ow);
    const int h0 = (int)fh, w0 = (int)fw;
    const int h1 = h0 + (h0 < Hin - 1 ? 1 : 0), w1 = w0 + (w0 < Win - 1 ? 1 : 0);
    const double lh1 = fh - (double)h0, lh0 = 1.0 - lh1, lw1 = fw - (double)w0, lw0 = 1.0 - lw1;
    auto fetch = [&](int c, int h, int w) -> float {
        float v;
        if (src_u8) {
            // np.float32 division x / 255: the double quotient of an 8-bit integer by 255 is never within double rounding of a float
            // midpoint (its binary expansion repeats the 8 bits of x), so rounding it to float IS the correctly rounded fp32 quotient
            const uint8_t u = ((const uint8_t*)src)[((n * Hin + h) * Win + w) * 3 + c];
            v = (float)((double)u / 255.0);
        } else {
            v = ((const float*)src)[((n * 3 + c) * Hin + h) * (long long)Win + w];
        }
        return affine ? v * in_scale + in_shift : v;
    };
    float o[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) o[c] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v = lh0 * (lw0 * fetch(c, h0, w0) + lw1 * fetch(c, h0, w1)) + lh1 * (lw0 * fetch(c, h1, w0) + lw1 * fetch(c, h1, w1));
        o[c] = (float)(normalize ? 2.0 * v - 1.0 : v);
    }
    T* yp = y + i * ldy;
    for (int c0 = 0; c0 < cpad; c0 += 4) {
        float q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = c0 + e < 16 ? o[(c0 + e) & 15] : 0.f;
        store4e<T>(yp + c0, q);
    }
}

// =================================================================================================
// feature statistics: sum[d] += sum_b (x[b][d] - K[d]);  cross[i][j] += sum_b (x[b][i] - K[i]) (x[b][j] - K[j])
// =================================================================================================
__global__ void feature_colsum_kernel(const float* __restrict__ x, int ldx, int B, int D, float* __restrict__ shift, int init_shift,
                                      double* __restrict__ sum) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    if (init_shift) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += (double)x[(size_t)b * ldx + d];
        shift[d] = (float)(s / (double)B);
    }
    const float k = shift[d];
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)(x[(size_t)b * ldx + d] - k);
    sum[d] += s;
}

// 64 x 64 tile of the D x D product per workgroup, 32 x 32 per wave: exact fp32 MFMA over the batch (a k-ordered fma chain), fp64 add
// into the accumulator -- each element is owned by one lane: no atomics
__global__ __launch_bounds__(256) void feature_cross_kernel(const float* __restrict__ x, int ldx, int B, int D, const float* __restrict__ shift,
                                                            double* __restrict__ cross) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int i0 = blockIdx.x * 64 + 32 * (wave >> 1), j0 = blockIdx.y * 64 + 32 * (wave & 1);
    const int ia = i0 + l31, jb = j0 + l31;
    const bool iok = ia < D, jok = jb < D;
    const float ki = iok ? shift[ia] : 0.f, kj = jok ? shift[jb] : 0.f;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k = 0; k < B; k += 2) {
        const int b = k + lh;
        const float av = (b < B && iok) ? x[(size_t)b * ldx + ia] - ki : 0.f;     // A[i][k] = xc[k][i]
        const float bv = (b < B && jok) ? x[(size_t)b * ldx + jb] - kj : 0.f;     // B[k][j] = xc[k][j]
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    if (!jok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + 8 * (r >> 2) + 4 * lh + (r & 3);
        if (i < D) cross[(size_t)i * D + jb] += (double)acc[r];
    }
}

#define KX_DISPATCH_T(dtype, ...)                  \
    do {                                           \
        if ((dtype) == WU_BF16) {                  \
            using T = bf16_t;                      \
            __VA_ARGS__;                           \
        } else {                                   \
            using T = float;                       \
            __VA_ARGS__;                           \
        }                                          \
    } while (0)

int kx_kp(int K, int dtype) {
    const int ke = kKB / (dtype == WU_BF16 ? 2 : 4);
    return (K + ke - 1) / ke * ke;
}

}  // namespace

extern "C" size_t wu_conv_kxk_packed_bytes(int Cout, int Cin, int KH, int KW, int dtype) {
    if (Cout <= 0 || Cin <= 0 || KH <= 0 || KW <= 0 || (dtype != WU_F32 && dtype != WU_BF16)) return 0;
    return (size_t)cdiv(Cout, 64) * 64 * kx_kp(KH * KW * Cin, dtype) * (dtype == WU_BF16 ? 2 : 4);
}

extern "C" int wu_pack_conv_kxk(const float* w_oihw, void* w_packed, int Cout, int Cin_w, int Cin, int KH, int KW, int dtype, void* stream) {
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "wu_pack_conv_kxk: dtype %d", dtype);
    WU_REQUIRE(Cout > 0 && Cout % 16 == 0, "wu_pack_conv_kxk: Cout %d must be a positive multiple of 16", Cout);
    WU_REQUIRE(Cin > 0 && Cin % 16 == 0, "wu_pack_conv_kxk: Cin %d must be a positive multiple of 16", Cin);
    WU_REQUIRE(Cin_w > 0 && Cin_w <= Cin, "wu_pack_conv_kxk: weight channels %d outside 1..Cin (%d)", Cin_w, Cin);
    WU_REQUIRE(KH > 0 && KW > 0 && KH <= 15 && KW <= 15, "wu_pack_conv_kxk: kernel %d x %d", KH, KW);
    WU_REQUIRE(w_oihw && w_packed, "wu_pack_conv_kxk: NULL pointer");
    const int K = KH * KW * Cin, Kp = kx_kp(K, dtype);
    const long long total = (long long)cdiv(Cout, 64) * 64 * Kp;
    hipStream_t s = (hipStream_t)stream;
    KX_DISPATCH_T(dtype, hipLaunchKernelGGL(pack_kxk_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                                            w_oihw, (T*)w_packed, Cout, Cin_w, Cin, KH, KW, K, Kp, total));
    WU_LAUNCH_CHECK("pack_kxk_kernel");
    return 0;
}

extern "C" int wu_conv_kxk_fwd(const void* x, int ldx, const void* w_packed, const float* bias, void* y, int ldy,
                               int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w,
                               int act, int dtype, void* stream) {
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "wu_conv_kxk_fwd: dtype %d", dtype);
    WU_REQUIRE(Cin > 0 && Cin % 16 == 0, "wu_conv_kxk_fwd: Cin %d must be a positive multiple of 16", Cin);
    WU_REQUIRE(Cout > 0 && Cout % 16 == 0, "wu_conv_kxk_fwd: Cout %d must be a positive multiple of 16", Cout);
    WU_REQUIRE(KH > 0 && KW > 0 && KH <= 15 && KW <= 15, "wu_conv_kxk_fwd: kernel %d x %d", KH, KW);
    WU_REQUIRE(stride_h > 0 && stride_w > 0 && pad_h >= 0 && pad_w >= 0 && pad_h < KH && pad_w < KW,
               "wu_conv_kxk_fwd: stride %d x %d / pad %d x %d", stride_h, stride_w, pad_h, pad_w);
    WU_REQUIRE(N > 0 && H > 0 && W > 0, "wu_conv_kxk_fwd: empty input %d x %d x %d", N, H, W);
    WU_REQUIRE(act == WU_ACT_NONE || act == WU_ACT_RELU, "wu_conv_kxk_fwd: act %d", act);
    WU_REQUIRE(ldx >= Cin && ldy >= Cout && ldx % 8 == 0 && ldy % 8 == 0, "wu_conv_kxk_fwd: ldx %d / ldy %d (>= C, multiples of 8)", ldx, ldy);
    WU_REQUIRE(x && w_packed && y && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)w_packed & 15) == 0 &&
               ((uintptr_t)bias & 15) == 0, "wu_conv_kxk_fwd: x, y, w_packed and bias must be 16-byte aligned device pointers");
    const int Ho = (H + 2 * pad_h - KH) / stride_h + 1, Wo = (W + 2 * pad_w - KW) / stride_w + 1;
    WU_REQUIRE(H + 2 * pad_h >= KH && W + 2 * pad_w >= KW && Ho > 0 && Wo > 0, "wu_conv_kxk_fwd: %d x %d input smaller than the %d x %d kernel",
               H, W, KH, KW);
    const size_t esz = dtype == WU_BF16 ? 2 : 4;
    const size_t img_x = (size_t)H * W * ldx * esz;
    WU_REQUIRE(img_x < (1u << 30) && (size_t)Ho * Wo < (1u << 24), "wu_conv_kxk_fwd: image of %zu bytes too large", img_x);
    // the input descriptor addresses 32-bit byte offsets: batches whose input exceeds 1 GiB run as several launches
    const int nb = (int)std::min<size_t>((size_t)N, ((size_t)1 << 30) / img_x);
    const int Kp = kx_kp(KH * KW * Cin, dtype);
    const int cout32 = cdiv(Cout, 32) * 32;
    const int ni = cout32 % 64 == 0 ? 2 : 1;         // 64-cout tiles where they waste nothing over 32-cout tiles
    const int n_ct = cout32 / (32 * ni);
    hipStream_t s = (hipStream_t)stream;
    for (int n0 = 0; n0 < N; n0 += nb) {
        const int nn = std::min(nb, N - n0);
        KxArgs a;
        a.x = (const char*)x + (size_t)n0 * img_x;
        a.w = w_packed; a.bias = bias;
        a.y = (char*)y + (size_t)n0 * Ho * Wo * ldy * esz;
        a.ldx = ldx; a.ldy = ldy; a.H = H; a.W = W; a.Cin = Cin; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout; a.KW = KW;
        a.sh = stride_h; a.sw = stride_w; a.ph = pad_h; a.pw = pad_w; a.act = act;
        a.M = nn * Ho * Wo;
        a.K = KH * KW * Cin; a.Kp = Kp; a.n_ct = n_ct;
        a.x_bytes = (int)((((size_t)nn * H * W - 1) * ldx + Cin) * esz);
        const unsigned grid = (unsigned)(cdiv(a.M, kTM) * n_ct);
        if (ni == 2) KX_DISPATCH_T(dtype, hipLaunchKernelGGL((conv_kxk_kernel<T, 2>), dim3(grid), dim3(256), 2 * (kTM + 64) * kKB, s, a));
        else KX_DISPATCH_T(dtype, hipLaunchKernelGGL((conv_kxk_kernel<T, 1>), dim3(grid), dim3(256), 2 * (kTM + 32) * kKB, s, a));
        WU_LAUNCH_CHECK("conv_kxk_kernel");
    }
    return 0;
}

extern "C" int wu_pool3x3_fwd(const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int stride, int pad, int mode,
                              int dtype, void* stream) {
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "wu_pool3x3_fwd: dtype %d", dtype);
    WU_REQUIRE(mode == WU_POOL_MAX || mode == WU_POOL_AVG || mode == WU_POOL_AVG_EXCL_PAD, "wu_pool3x3_fwd: mode %d", mode);
    WU_REQUIRE((stride == 1 || stride == 2) && (pad == 0 || pad == 1), "wu_pool3x3_fwd: stride %d / pad %d", stride, pad);
    WU_REQUIRE(mode == WU_POOL_MAX || (stride == 1 && pad == 1), "wu_pool3x3_fwd: average pools are stride 1, pad 1");
    WU_REQUIRE(N > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0,
               "wu_pool3x3_fwd: C %d (multiple of 4) / ldx %d / ldy %d", C, ldx, ldy);
    WU_REQUIRE(H + 2 * pad >= 3 && W + 2 * pad >= 3, "wu_pool3x3_fwd: %d x %d input smaller than the window", H, W);
    WU_REQUIRE(x && y && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "wu_pool3x3_fwd: x, y must be 16-byte aligned");
    const int Ho = (H + 2 * pad - 3) / stride + 1, Wo = (W + 2 * pad - 3) / stride + 1;
    const long long total = (long long)N * Ho * Wo * (C / 4);
    hipStream_t s = (hipStream_t)stream;
    KX_DISPATCH_T(dtype, hipLaunchKernelGGL(pool3x3_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                                            (const T*)x, ldx, (T*)y, ldy, H, W, Ho, Wo, C / 4, stride, pad, mode, total));
    WU_LAUNCH_CHECK("pool3x3_kernel");
    return 0;
}

extern "C" int wu_global_avgpool_fwd(const void* x, int ldx, float* out, int ldo, int N, int H, int W, int C, int dtype, void* stream) {
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "wu_global_avgpool_fwd: dtype %d", dtype);
    WU_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0 && ldo >= C,
               "wu_global_avgpool_fwd: C %d (multiple of 4) / ldx %d / ldo %d", C, ldx, ldo);
    WU_REQUIRE(x && out && ((uintptr_t)x & 15) == 0, "wu_global_avgpool_fwd: x must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    KX_DISPATCH_T(dtype, hipLaunchKernelGGL(global_avgpool_kernel<T>, dim3((unsigned)cdiv(C, 64), (unsigned)N), dim3(256), 0, s,
                                            (const T*)x, ldx, out, ldo, H * W, C));
    WU_LAUNCH_CHECK("global_avgpool_kernel");
    return 0;
}

extern "C" int wu_inception_input(const void* src, int src_u8, int N, int Hin, int Win, float in_scale, float in_shift, int normalize,
                                  void* y, int ldy, int Ho, int Wo, int cpad, int dtype, void* stream) {
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "wu_inception_input: dtype %d", dtype);
    WU_REQUIRE(N > 0 && Hin > 0 && Win > 0 && Ho > 0 && Wo > 0, "wu_inception_input: sizes %d x %d -> %d x %d", Hin, Win, Ho, Wo);
    WU_REQUIRE(cpad >= 4 && cpad % 4 == 0 && ldy >= cpad && ldy % 4 == 0, "wu_inception_input: cpad %d (>= 4, multiple of 4) / ldy %d", cpad, ldy);
    WU_REQUIRE(src && y && ((uintptr_t)y & 15) == 0, "wu_inception_input: NULL or unaligned pointer");
    const long long total = (long long)N * Ho * Wo;
    const int affine = (in_scale != 1.f || in_shift != 0.f) ? 1 : 0;
    const double sch = (double)Hin / (double)Ho, scw = (double)Win / (double)Wo;
    hipStream_t s = (hipStream_t)stream;
    KX_DISPATCH_T(dtype, hipLaunchKernelGGL(inception_input_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                                            src, src_u8, Hin, Win, in_scale, in_shift, affine, normalize, (T*)y, ldy, Ho, Wo, cpad, sch, scw, total));
    WU_LAUNCH_CHECK("inception_input_kernel");
    return 0;
}

extern "C" int wu_feature_stats_update(const float* x, int ldx, int B, int D, float* shift, int init_shift, double* sum, double* cross,
                                       void* stream) {
    WU_REQUIRE(B > 0 && D > 0 && ldx >= D, "wu_feature_stats_update: B %d / D %d / ldx %d", B, D, ldx);
    WU_REQUIRE(x && shift && sum && cross, "wu_feature_stats_update: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(feature_colsum_kernel, dim3((unsigned)cdiv(D, 256)), dim3(256), 0, s, x, ldx, B, D, shift, init_shift, sum);
    WU_LAUNCH_CHECK("feature_colsum_kernel");
    hipLaunchKernelGGL(feature_cross_kernel, dim3((unsigned)cdiv(D, 64), (unsigned)cdiv(D, 64)), dim3(256), 0, s, x, ldx, B, D, shift, cross);
    WU_LAUNCH_CHECK("feature_cross_kernel");
    return 0;
}
