// Kernels of the TRAINABLE ResNet-101 (classifier.py:106 / estimator.py:143: torchvision.models.resnet101 trained from scratch in
// train-mode BatchNorm, sh/train_classifier.sh, sh/train_estimator.sh) that the frozen estimator (resnet.hip) does not need:
//   * bn_stats_*       batch statistics of a stored pre-BN conv output (shifted one-pass sums, per-split partials folded in a fixed order)
//                      and nn.BatchNorm2d's running-statistics update;
//   * bn_apply_kernel  y = act(x * scale + shift [+ x2 * scale2 + shift2 | + residual]) with scale / shift from the batch statistics;
//   * bn_bwd_*         BatchNorm backward from the ReLU-gated output gradient: dgamma, dbeta (deterministic) and dx, for one or two
//                      branches that share the gated gradient (a downsampling Bottleneck's bn3 and downsample.1);
//   * pw_wgrad_kernel  weight gradient of a pointwise conv, dW[Cout][Cin] = sum_rows dY[r][co] X[pix(r)][ci] (stride-2 gather of the
//                      downsample conv): both operands are row (K) strided in NHWC, so they are staged TRANSPOSED into LDS and the
//                      matrix cores read 16-byte runs of K; deterministic split-K over rows;
//   * stem_wgrad_kernel the 7x7/2 stem's weight gradient from the fp32 NCHW image (im2col patches staged in LDS, VALU FMA).
// Every reduction writes per-split partial sums to a caller-owned workspace and a fold kernel adds them in split order: no atomics,
// results independent of the launch schedule.
#include "wu_common.h"

namespace {

inline bool aligned16(const void* p, int ld, int esz) { return ((uintptr_t)p % 16) == 0 && (ld * esz) % 16 == 0; }

#define TRAIN_DISPATCH(dtype, ...)                                  \
    do {                                                            \
        if ((dtype) == WU_BF16) { using T = bf16_t; __VA_ARGS__; }  \
        else { using T = float; __VA_ARGS__; }                      \
    } while (0)

template <typename T> __device__ __forceinline__ void ld_vec(const T* p, float* f) { unpack16<T>(*(const uint4*)p, f); }
template <typename T> __device__ __forceinline__ void st_vec(T* p, const float* f) { *(uint4*)p = pack16<T>(f); }

// =================================================================================================
// BatchNorm statistics.  Rows = the N*H*W pixels of an NHWC tensor with pixel stride ld; channels in groups of 64.
// A workgroup owns 64 channels and a contiguous range of rows; a thread owns one 16-byte channel vector (8 bf16 / 4 fp32) and every
// RP-th row of the range.  Sums are SHIFTED by the channel's value in row 0 (sum (x - K), sum (x - K)^2): on offset data (|mean| >> std)
// the naive E[x^2] - E[x]^2 cancels catastrophically in fp32; after the shift both sums stay O(n * var).
// =================================================================================================
constexpr int kBnMaxSplits = 256;
constexpr int kBnThreads = 256;

template <typename T> struct BnGeom {
    static constexpr int VEC = 16 / (int)sizeof(T);        // channels per thread
    static constexpr int TPR = 64 / VEC;                   // threads per row of 64 channels
    static constexpr int RP = kBnThreads / TPR;            // rows in flight per workgroup
};

inline int bn_splits(long long M, int C, int rp) {
    // ~1024 workgroups over the chip, but at least 8 rows per thread
    long long s = (1024 + C / 64 - 1) / (C / 64);
    const long long cap = M / (8LL * rp);
    if (s > cap) s = cap;
    if (s > kBnMaxSplits) s = kBnMaxSplits;
    return s < 1 ? 1 : (int)s;
}

template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn_stats_partial_kernel(const T* __restrict__ x, int ldx, long long M, int C,
                                                                      long long rows_per_split, float* __restrict__ part) {
    using G = BnGeom<T>;
    __shared__ float red[2][G::RP][64];
    const int t = threadIdx.x, cv = t % G::TPR, rr = t / G::TPR;
    const int c0 = blockIdx.x * 64 + cv * G::VEC;
    const long long r0 = (long long)blockIdx.y * rows_per_split;
    long long r1 = r0 + rows_per_split;
    if (r1 > M) r1 = M;
    float k[G::VEC], s1[G::VEC], s2[G::VEC];
    ld_vec<T>(x + c0, k);
#pragma unroll
    for (int e = 0; e < G::VEC; ++e) s1[e] = s2[e] = 0.f;
    for (long long r = r0 + rr; r < r1; r += G::RP) {
        float v[G::VEC];
        ld_vec<T>(x + r * ldx + c0, v);
#pragma unroll
        for (int e = 0; e < G::VEC; ++e) {
            const float d = v[e] - k[e];
            s1[e] += d;
            s2[e] = fmaf(d, d, s2[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < G::VEC; ++e) {
        red[0][rr][cv * G::VEC + e] = s1[e];
        red[1][rr][cv * G::VEC + e] = s2[e];
    }
    __syncthreads();
    if (t < 128) {
        const int q = t >> 6, c = t & 63;
        float s = 0.f;
        for (int i = 0; i < G::RP; ++i) s += red[q][i][c];          // fixed order
        part[((size_t)blockIdx.y * 2 + q) * C + blockIdx.x * 64 + c] = s;
    }
}

template <typename T>
__global__ void bn_stats_final_kernel(const T* __restrict__ x, const float* __restrict__ part, int splits, long long M, int C, float eps,
                                      float momentum, float* __restrict__ stats, float* running_mean, float* running_var,
                                      long long* num_batches_tracked) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && num_batches_tracked) num_batches_tracked[0] += 1;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < splits; ++s) {                               // split order: deterministic
        s1 += (double)part[((size_t)s * 2) * C + c];
        s2 += (double)part[((size_t)s * 2 + 1) * C + c];
    }
    const double n = (double)M, dm = s1 / n;
    double var = s2 / n - dm * dm;
    if (var < 0.0) var = 0.0;
    const float mean = ElemTraits<T>::load(x + c) + (float)dm;
    stats[c] = mean;
    stats[C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[c] = momentum * mean + (1.f - momentum) * running_mean[c];
    if (running_var) {
        const float unbiased = (float)(M > 1 ? var * n / (n - 1.0) : var);
        running_var[c] = momentum * unbiased + (1.f - momentum) * running_var[c];
    }
}

// =================================================================================================
// BatchNorm apply: y = act(x * g rstd + (b - mean g rstd) [+ x2 * ... | + res])
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ st, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const T* __restrict__ x2, int ldx2, const float* __restrict__ st2,
                                                       const float* __restrict__ gamma2, const float* __restrict__ beta2, const T* __restrict__ res,
                                                       int ldres, T* __restrict__ y, int ldy, long long M, int C, int act) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int cvs = C / VEC;
    const long long total = M * cvs;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cvs;
        const int c0 = (int)(i - r * cvs) * VEC;
        float v[VEC], o[VEC];
        ld_vec<T>(x + r * ldx + c0, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int c = c0 + e;
            const float sc = gamma[c] * st[C + c];
            o[e] = fmaf(v[e], sc, beta[c] - st[c] * sc);
        }
        if (x2) {
            ld_vec<T>(x2 + r * ldx2 + c0, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int c = c0 + e;
                const float sc = gamma2[c] * st2[C + c];
                o[e] += fmaf(v[e], sc, beta2[c] - st2[c] * sc);
            }
        } else if (res) {
            ld_vec<T>(res + r * ldres + c0, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = act_apply(o[e], act);
        st_vec<T>(y + r * ldy + c0, o);
    }
}

// =================================================================================================
// BatchNorm backward.  gg = g * act'(y) (y: the stored output of the activation; NULL = no gate).
//   partial: per split and channel  sum gg,  sum gg (x - mean)  [, sum gg (x2 - mean2)]
//   final:   dbeta = sum gg, dgamma = rstd sum gg (x - mean)  (fixed split order)
//   dx:      dx = gamma rstd (gg - dbeta / n - xhat dgamma / n)  [dx2 likewise]  [gres = gg]
// =================================================================================================
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_partial_kernel(const T* __restrict__ g, int ldg, const T* __restrict__ y, int ldy, int act,
                                                                    const T* __restrict__ x, int ldx, const float* __restrict__ st,
                                                                    const T* __restrict__ x2, int ldx2, const float* __restrict__ st2,
                                                                    long long M, int C, long long rows_per_split, float* __restrict__ part) {
    using G = BnGeom<T>;
    __shared__ float red[3][G::RP][64];
    const int t = threadIdx.x, cv = t % G::TPR, rr = t / G::TPR;
    const int c0 = blockIdx.x * 64 + cv * G::VEC;
    const long long r0 = (long long)blockIdx.y * rows_per_split;
    long long r1 = r0 + rows_per_split;
    if (r1 > M) r1 = M;
    float m1[G::VEC], m2[G::VEC], sg[G::VEC], sx[G::VEC], sx2[G::VEC];
#pragma unroll
    for (int e = 0; e < G::VEC; ++e) {
        m1[e] = st[c0 + e];
        m2[e] = x2 ? st2[c0 + e] : 0.f;
        sg[e] = sx[e] = sx2[e] = 0.f;
    }
    for (long long r = r0 + rr; r < r1; r += G::RP) {
        float gv[G::VEC], xv[G::VEC];
        ld_vec<T>(g + r * ldg + c0, gv);
        if (y) {
            float yv[G::VEC];
            ld_vec<T>(y + r * ldy + c0, yv);
#pragma unroll
            for (int e = 0; e < G::VEC; ++e) gv[e] = act_gate(gv[e], yv[e], act);
        }
        ld_vec<T>(x + r * ldx + c0, xv);
#pragma unroll
        for (int e = 0; e < G::VEC; ++e) {
            sg[e] += gv[e];
            sx[e] = fmaf(gv[e], xv[e] - m1[e], sx[e]);
        }
        if (x2) {
            ld_vec<T>(x2 + r * ldx2 + c0, xv);
#pragma unroll
            for (int e = 0; e < G::VEC; ++e) sx2[e] = fmaf(gv[e], xv[e] - m2[e], sx2[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < G::VEC; ++e) {
        red[0][rr][cv * G::VEC + e] = sg[e];
        red[1][rr][cv * G::VEC + e] = sx[e];
        red[2][rr][cv * G::VEC + e] = sx2[e];
    }
    __syncthreads();
    if (t < 192) {
        const int q = t >> 6, c = t & 63;
        float s = 0.f;
        for (int i = 0; i < G::RP; ++i) s += red[q][i][c];
        part[((size_t)blockIdx.y * 3 + q) * C + blockIdx.x * 64 + c] = s;
    }
}

__global__ void bn_bwd_final_kernel(const float* __restrict__ part, int splits, int C, const float* __restrict__ st, const float* __restrict__ st2,
                                    float* dgamma, float* dbeta, float* dgamma2, float* dbeta2) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double sg = 0.0, sx = 0.0, sx2 = 0.0;
    for (int s = 0; s < splits; ++s) {
        sg += (double)part[((size_t)s * 3) * C + c];
        sx += (double)part[((size_t)s * 3 + 1) * C + c];
        sx2 += (double)part[((size_t)s * 3 + 2) * C + c];
    }
    dbeta[c] = (float)sg;
    dgamma[c] = (float)(sx * (double)st[C + c]);
    if (dgamma2) {
        dbeta2[c] = (float)sg;
        dgamma2[c] = (float)(sx2 * (double)st2[C + c]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const T* __restrict__ g, int ldg, const T* __restrict__ y, int ldy, int act,
                                                        const T* __restrict__ x, int ldx, const float* __restrict__ st, const float* __restrict__ gamma,
                                                        const float* __restrict__ dgamma, const float* __restrict__ dbeta, T* __restrict__ dx, int lddx,
                                                        const T* __restrict__ x2, int ldx2, const float* __restrict__ st2, const float* __restrict__ gamma2,
                                                        const float* __restrict__ dgamma2, T* __restrict__ dx2, int lddx2, T* __restrict__ gres, int ldgres,
                                                        long long M, int C) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int cvs = C / VEC;
    const long long total = M * cvs;
    const float inv_n = 1.f / (float)M;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cvs;
        const int c0 = (int)(i - r * cvs) * VEC;
        float gv[VEC], v[VEC], o[VEC];
        ld_vec<T>(g + r * ldg + c0, gv);
        if (y) {
            ld_vec<T>(y + r * ldy + c0, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) gv[e] = act_gate(gv[e], v[e], act);
        }
        if (gres) st_vec<T>(gres + r * ldgres + c0, gv);
        ld_vec<T>(x + r * ldx + c0, v);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int c = c0 + e;
            const float rs = st[C + c], xh = (v[e] - st[c]) * rs;
            o[e] = gamma[c] * rs * (gv[e] - dbeta[c] * inv_n - xh * (dgamma[c] * inv_n));
        }
        st_vec<T>(dx + r * lddx + c0, o);
        if (x2) {
            ld_vec<T>(x2 + r * ldx2 + c0, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int c = c0 + e;
                const float rs = st2[C + c], xh = (v[e] - st2[c]) * rs;
                o[e] = gamma2[c] * rs * (gv[e] - dbeta[c] * inv_n - xh * (dgamma2[c] * inv_n));
            }
            st_vec<T>(dx2 + r * lddx2 + c0, o);
        }
    }
}

inline int ew_grid(long long total) {
    long long g = (total + 255) / 256;
    if (g > 256 * 32) g = 256 * 32;
    return g < 1 ? 1 : (int)g;
}

// =================================================================================================
// Pointwise conv weight gradient: a 64 (cout) x 64 (cin) tile per workgroup, 4 waves of 32 x 32, K = rows in stages of 64.
// Staging: each thread loads 16-byte channel vectors of one row of dY / X and scatters them TRANSPOSED into LDS ([channel][row],
// pitch 64 + one vector), so an MFMA fragment (8 consecutive K of one channel for bf16, 4 for fp32) is one 16-byte LDS read.
// =================================================================================================
constexpr int kWgKT = 64;
constexpr int kWgMaxSplits = 64;

struct PwWgArgs {
    const void* x; const void* dy; float* slab;
    int ldx, lddy;
    int Hc, Wc, in_stride, Hin, Win, Cin, Cout;
    long long M, rows_per_split;
    int ci_tiles;
};

template <typename T> struct WgMma;
template <> struct WgMma<bf16_t> {
    static __device__ __forceinline__ void run(f32x16_t& acc, const uint4& a, const uint4& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct WgMma<float> {     // exact fp32: four 32x32x2 steps per 16-byte fragment pair (same k permutation on both operands)
    static __device__ __forceinline__ void run(f32x16_t& acc, const uint4& a, const uint4& b) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
};

template <typename T>
__global__ __launch_bounds__(256) void pw_wgrad_kernel(const PwWgArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T);
    constexpr int PITCH = kWgKT + VEC;                   // elements; a multiple of 16 bytes
    constexpr int ITEMS = kWgKT * 64 / VEC / 256;        // 16-byte items per thread and operand per stage
    constexpr int VPR = 64 / VEC;                        // items per row
    __shared__ __attribute__((aligned(16))) T xs[64 * PITCH];
    __shared__ __attribute__((aligned(16))) T ds[64 * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int ci0 = (blockIdx.x % a.ci_tiles) * 64, co0 = (blockIdx.x / a.ci_tiles) * 64;
    const long long r0 = (long long)blockIdx.y * a.rows_per_split;
    long long r1 = r0 + a.rows_per_split;
    if (r1 > a.M) r1 = a.M;
    const T* X = (const T*)a.x;
    const T* D = (const T*)a.dy;

    uint4 xr[ITEMS], dr[ITEMS];
    auto load = [&](long long kb) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int it = tid + 256 * k, row = it / VPR, cv = it % VPR;
            const long long r = kb + row;
            if (r < r1) {
                long long pix = r;
                if (a.in_stride != 1) {
                    const int wc = (int)(r % a.Wc);
                    const long long q = r / a.Wc;
                    const int hc = (int)(q % a.Hc);
                    const long long n = q / a.Hc;
                    pix = (n * a.Hin + (long long)hc * a.in_stride) * a.Win + (long long)wc * a.in_stride;
                }
                xr[k] = *(const uint4*)(X + pix * a.ldx + ci0 + cv * VEC);
                dr[k] = *(const uint4*)(D + r * a.lddy + co0 + cv * VEC);
            } else {
                xr[k] = make_uint4(0u, 0u, 0u, 0u);
                dr[k] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
    };
    auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int it = tid + 256 * k, row = it / VPR, cv = it % VPR;
            const T* xe = (const T*)&xr[k];
            const T* de = (const T*)&dr[k];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                xs[(cv * VEC + e) * PITCH + row] = xe[e];
                ds[(cv * VEC + e) * PITCH + row] = de[e];
            }
        }
    };

    f32x16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const T* arow = ds + ((wave >> 1) * 32 + l31) * PITCH + lh * (VEC == 8 ? 8 : 4);
    const T* brow = xs + ((wave & 1) * 32 + l31) * PITCH + lh * (VEC == 8 ? 8 : 4);
    constexpr int KSTEP = VEC == 8 ? 16 : 8;             // K per fragment read (both lane halves)

    load(r0);
    for (long long kb = r0; kb < r1; kb += kWgKT) {
        __syncthreads();                                 // the previous stage's fragment reads are done
        store();
        __syncthreads();
        if (kb + kWgKT < r1) load(kb + kWgKT);           // next stage's global loads in flight under the MFMAs
#pragma unroll
        for (int kk = 0; kk < kWgKT; kk += KSTEP) {
            const uint4 av = *(const uint4*)(arow + kk);
            const uint4 bv = *(const uint4*)(brow + kk);
            WgMma<T>::run(acc, av, bv);
        }
    }
    // D[m = cout][n = cin]: row = (j & 3) + 8 (j >> 2) + 4 lh, col = l31
    float* out = a.slab + (size_t)blockIdx.y * a.Cout * a.Cin;
    const int cb = co0 + (wave >> 1) * 32, ci = ci0 + (wave & 1) * 32 + l31;
#pragma unroll
    for (int j = 0; j < 16; ++j) out[(size_t)(cb + (j & 3) + 8 * (j >> 2) + 4 * lh) * a.Cin + ci] = acc[j];
}

__global__ void slab_fold_kernel(const float* __restrict__ slab, int splits, long long n, float* __restrict__ out, int accumulate) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += slab[(size_t)k * n + i];
        out[i] = accumulate ? out[i] + s : s;
    }
}

struct PwWgPlan { int splits; long long rows_per_split; size_t ws; };
inline PwWgPlan pw_wgrad_plan(long long M, int Cin, int Cout) {
    const int tiles = (Cin / 64) * (Cout / 64);
    long long s = (1024 + tiles - 1) / tiles;
    const long long cap = (M + 255) / 256;               // at least 256 rows per split
    if (s > cap) s = cap;
    if (s > kWgMaxSplits) s = kWgMaxSplits;
    if (s < 1) s = 1;
    long long rps = (M + s - 1) / s;
    rps = (rps + kWgKT - 1) / kWgKT * kWgKT;
    PwWgPlan p;
    p.splits = (int)((M + rps - 1) / rps);
    p.rows_per_split = rps;
    p.ws = (size_t)p.splits * Cout * Cin * sizeof(float);
    return p;
}

// =================================================================================================
// Stem weight gradient: dW[co][tap], tap = ci*49 + kh*7 + kw, over the N*Ho*Wo output pixels.  A workgroup owns a contiguous range of
// output pixels; per stage of 32 pixels the im2col patches (fp32, zero padding) and the gradient rows are staged in LDS; thread
// (co = t & 63, group = t >> 6) accumulates 40 consecutive taps of one output channel in registers.
// =================================================================================================
constexpr int kStP = 32, kStTaps = 147, kStPitch = 160, kStGroup = 40, kStMaxSplits = 512;

template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, const T* __restrict__ dy, int lddy, int N, int H, int W,
                                                         int Ho, int Wo, long long pix_per_split, float* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) float patch[kStP][kStPitch];
    __shared__ float dys[kStP][64];
    const int t = threadIdx.x, co = t & 63, grp = t >> 6;
    const long long P = (long long)N * Ho * Wo;
    const long long p0 = (long long)blockIdx.x * pix_per_split;
    long long p1 = p0 + pix_per_split;
    if (p1 > P) p1 = P;
    float acc[kStGroup];
#pragma unroll
    for (int i = 0; i < kStGroup; ++i) acc[i] = 0.f;
    for (long long pb = p0; pb < p1; pb += kStP) {
        __syncthreads();
        for (int i = t; i < kStP * kStPitch; i += 256) {
            const int p = i / kStPitch, tap = i % kStPitch;
            const long long pix = pb + p;
            float v = 0.f;
            if (pix < p1 && tap < kStTaps) {
                const int ow = (int)(pix % Wo);
                const long long q = pix / Wo;
                const int oh = (int)(q % Ho);
                const int n = (int)(q / Ho);
                const int ci = tap / 49, kh = (tap % 49) / 7, kw = tap % 7;
                const int ih = 2 * oh - 3 + kh, iw = 2 * ow - 3 + kw;
                if (ih >= 0 && ih < H && iw >= 0 && iw < W) v = x[(((size_t)n * 3 + ci) * H + ih) * W + iw];
            }
            patch[p][tap] = v;
        }
        for (int i = t; i < kStP * 64; i += 256) {
            const int p = i >> 6, c = i & 63;
            const long long pix = pb + p;
            dys[p][c] = pix < p1 ? ElemTraits<T>::load(dy + pix * lddy + c) : 0.f;
        }
        __syncthreads();
        for (int p = 0; p < kStP; ++p) {
            const float d = dys[p][co];
#pragma unroll
            for (int q = 0; q < kStGroup / 4; ++q) {
                const float4 v = *(const float4*)&patch[p][grp * kStGroup + 4 * q];
                acc[4 * q] = fmaf(d, v.x, acc[4 * q]);
                acc[4 * q + 1] = fmaf(d, v.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(d, v.z, acc[4 * q + 2]);
                acc[4 * q + 3] = fmaf(d, v.w, acc[4 * q + 3]);
            }
        }
    }
    float* out = slab + (size_t)blockIdx.x * 64 * kStTaps + (size_t)co * kStTaps;
#pragma unroll
    for (int i = 0; i < kStGroup; ++i) {
        const int tap = grp * kStGroup + i;
        if (tap < kStTaps) out[tap] = acc[i];
    }
}

struct StemWgPlan { int splits; long long pix_per_split; size_t ws; };
inline StemWgPlan stem_wgrad_plan(int N, int H, int W) {
    const long long P = (long long)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1);
    long long s = (P + 255) / 256;                       // at least 256 pixels per workgroup
    if (s > kStMaxSplits) s = kStMaxSplits;
    if (s < 1) s = 1;
    long long pps = (P + s - 1) / s;
    pps = (pps + kStP - 1) / kStP * kStP;
    StemWgPlan p;
    p.splits = (int)((P + pps - 1) / pps);
    p.pix_per_split = pps;
    p.ws = (size_t)p.splits * 64 * kStTaps * sizeof(float);
    return p;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t wu_bn_stats_workspace(long long M, int C, int dtype) {
    if (M <= 0 || C <= 0 || C % 64) return 0;
    const int rp = dtype == WU_BF16 ? BnGeom<bf16_t>::RP : BnGeom<float>::RP;
    return (size_t)bn_splits(M, C, rp) * 2 * C * sizeof(float);
}

extern "C" int wu_bn_stats(const void* x, int ldx, long long M, int C, float eps, float momentum, float* stats,
                           float* running_mean, float* running_var, long long* num_batches_tracked,
                           void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    const int esz = dtype == WU_BF16 ? 2 : 4;
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "bn_stats: bad dtype");
    WU_REQUIRE(M > 0 && C > 0 && C % 64 == 0 && ldx >= C && aligned16(x, ldx, esz), "bn_stats: bad shape M=%lld C=%d ld=%d", M, C, ldx);
    WU_REQUIRE(stats != nullptr, "bn_stats: stats is NULL");
    const size_t need = wu_bn_stats_workspace(M, C, dtype);
    WU_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace % 16) == 0, "bn_stats: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    TRAIN_DISPATCH(dtype, {
        const int splits = bn_splits(M, C, BnGeom<T>::RP);
        const long long rps = (M + splits - 1) / splits;
        hipLaunchKernelGGL(bn_stats_partial_kernel<T>, dim3(C / 64, splits), dim3(kBnThreads), 0, s, (const T*)x, ldx, M, C, rps, (float*)workspace);
        hipLaunchKernelGGL(bn_stats_final_kernel<T>, dim3((C + 255) / 256), dim3(256), 0, s, (const T*)x, (const float*)workspace, splits, M, C, eps,
                           momentum, stats, running_mean, running_var, num_batches_tracked);
    });
    WU_LAUNCH_CHECK("bn_stats");
    return 0;
}

extern "C" int wu_bn_apply(const void* x, int ldx, const float* stats, const float* gamma, const float* beta,
                           const void* x2, int ldx2, const float* stats2, const float* gamma2, const float* beta2,
                           const void* residual, int ldres, void* y, int ldy, long long M, int C, int act, int dtype, void* stream) {
    const int esz = dtype == WU_BF16 ? 2 : 4;
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "bn_apply: bad dtype");
    WU_REQUIRE(M > 0 && C > 0 && C % 64 == 0 && ldx >= C && ldy >= C, "bn_apply: bad shape M=%lld C=%d", M, C);
    WU_REQUIRE(aligned16(x, ldx, esz) && aligned16(y, ldy, esz) && stats && gamma && beta, "bn_apply: alignment / NULL operand");
    WU_REQUIRE(!(x2 && residual), "bn_apply: x2 and residual are exclusive");
    if (x2) WU_REQUIRE(aligned16(x2, ldx2, esz) && ldx2 >= C && stats2 && gamma2 && beta2, "bn_apply: second branch");
    if (residual) WU_REQUIRE(aligned16(residual, ldres, esz) && ldres >= C, "bn_apply: residual alignment");
    const long long total = M * (C / (16 / esz));
    TRAIN_DISPATCH(dtype, hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, stats, gamma,
                                             beta, (const T*)x2, ldx2, stats2, gamma2, beta2, (const T*)residual, ldres, (T*)y, ldy, M, C, act));
    WU_LAUNCH_CHECK("bn_apply");
    return 0;
}

extern "C" size_t wu_bn_bwd_workspace(long long M, int C, int dtype) {
    if (M <= 0 || C <= 0 || C % 64) return 0;
    const int rp = dtype == WU_BF16 ? BnGeom<bf16_t>::RP : BnGeom<float>::RP;
    return (size_t)bn_splits(M, C, rp) * 3 * C * sizeof(float);
}

extern "C" int wu_bn_bwd(const void* g, int ldg, const void* y, int ldy, int act,
                         const void* x, int ldx, const float* stats, const float* gamma, float* dgamma, float* dbeta, void* dx, int lddx,
                         const void* x2, int ldx2, const float* stats2, const float* gamma2, float* dgamma2, float* dbeta2, void* dx2, int lddx2,
                         void* gres, int ldgres, long long M, int C, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
    const int esz = dtype == WU_BF16 ? 2 : 4;
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "bn_bwd: bad dtype");
    WU_REQUIRE(M > 0 && C > 0 && C % 64 == 0, "bn_bwd: bad shape M=%lld C=%d", M, C);
    WU_REQUIRE(aligned16(g, ldg, esz) && aligned16(x, ldx, esz) && aligned16(dx, lddx, esz) && ldg >= C && ldx >= C && lddx >= C,
               "bn_bwd: alignment");
    WU_REQUIRE(stats && gamma && dgamma && dbeta, "bn_bwd: NULL per-channel operand");
    if (y) WU_REQUIRE(aligned16(y, ldy, esz) && ldy >= C, "bn_bwd: y alignment");
    if (x2) WU_REQUIRE(aligned16(x2, ldx2, esz) && aligned16(dx2, lddx2, esz) && ldx2 >= C && lddx2 >= C && stats2 && gamma2 && dgamma2 && dbeta2,
                       "bn_bwd: second branch");
    if (gres) WU_REQUIRE(aligned16(gres, ldgres, esz) && ldgres >= C, "bn_bwd: gres alignment");
    const size_t need = wu_bn_bwd_workspace(M, C, dtype);
    WU_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace % 16) == 0, "bn_bwd: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const long long total = M * (C / (16 / esz));
    TRAIN_DISPATCH(dtype, {
        const int splits = bn_splits(M, C, BnGeom<T>::RP);
        const long long rps = (M + splits - 1) / splits;
        hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3(C / 64, splits), dim3(kBnThreads), 0, s, (const T*)g, ldg, (const T*)y, ldy, act,
                           (const T*)x, ldx, stats, (const T*)x2, ldx2, stats2, M, C, rps, (float*)workspace);
        hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)workspace, splits, C, stats, stats2,
                           dgamma, dbeta, x2 ? dgamma2 : nullptr, dbeta2);
        hipLaunchKernelGGL(bn_bwd_dx_kernel<T>, dim3(ew_grid(total)), dim3(256), 0, s, (const T*)g, ldg, (const T*)y, ldy, act, (const T*)x, ldx,
                           stats, gamma, dgamma, dbeta, (T*)dx, lddx, (const T*)x2, ldx2, stats2, gamma2, dgamma2, (T*)dx2, lddx2, (T*)gres, ldgres, M, C);
    });
    WU_LAUNCH_CHECK("bn_bwd");
    return 0;
}

extern "C" size_t wu_conv1x1_wgrad_workspace(long long M, int Cin, int Cout) {
    if (M <= 0 || Cin <= 0 || Cout <= 0 || Cin % 64 || Cout % 64) return 0;
    return pw_wgrad_plan(M, Cin, Cout).ws;
}

extern "C" int wu_conv1x1_wgrad(const void* x, int ldx, const void* dy, int lddy, float* dw, void* workspace, size_t workspace_bytes,
                                int N, int Hc, int Wc, int in_stride, int Hin, int Win, int Cin, int Cout, int accumulate, int dtype, void* stream) {
    const int esz = dtype == WU_BF16 ? 2 : 4;
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "conv1x1_wgrad: bad dtype");
    WU_REQUIRE(N > 0 && Hc > 0 && Wc > 0 && Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % 64 == 0, "conv1x1_wgrad: Cin=%d Cout=%d must be multiples of 64", Cin, Cout);
    WU_REQUIRE(in_stride == 1 || in_stride == 2, "conv1x1_wgrad: in_stride");
    if (in_stride == 1) WU_REQUIRE(Hin == Hc && Win == Wc, "conv1x1_wgrad: stride 1 needs Hin == Hc, Win == Wc");
    else WU_REQUIRE(Hc == (Hin - 1) / 2 + 1 && Wc == (Win - 1) / 2 + 1, "conv1x1_wgrad: stride-2 grid");
    WU_REQUIRE(aligned16(x, ldx, esz) && aligned16(dy, lddy, esz) && ldx >= Cin && lddy >= Cout && dw, "conv1x1_wgrad: alignment");
    const long long M = (long long)N * Hc * Wc;
    const PwWgPlan p = pw_wgrad_plan(M, Cin, Cout);
    WU_REQUIRE(workspace && workspace_bytes >= p.ws && ((uintptr_t)workspace % 16) == 0, "conv1x1_wgrad: workspace too small (%zu < %zu)", workspace_bytes, p.ws);
    PwWgArgs a;
    a.x = x; a.dy = dy; a.slab = (float*)workspace;
    a.ldx = ldx; a.lddy = lddy; a.Hc = Hc; a.Wc = Wc; a.in_stride = in_stride; a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.Cout = Cout;
    a.M = M; a.rows_per_split = p.rows_per_split; a.ci_tiles = Cin / 64;
    hipStream_t s = (hipStream_t)stream;
    TRAIN_DISPATCH(dtype, hipLaunchKernelGGL(pw_wgrad_kernel<T>, dim3((Cin / 64) * (Cout / 64), p.splits), dim3(256), 0, s, a));
    const long long n = (long long)Cout * Cin;
    hipLaunchKernelGGL(slab_fold_kernel, dim3(ew_grid(n)), dim3(256), 0, s, (const float*)workspace, p.splits, n, dw, accumulate);
    WU_LAUNCH_CHECK("conv1x1_wgrad");
    return 0;
}

extern "C" size_t wu_stem7x7_wgrad_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return stem_wgrad_plan(N, H, W).ws;
}

extern "C" int wu_stem7x7_wgrad(const float* x_nchw, const void* dy, int lddy, float* dw_oihw, void* workspace, size_t workspace_bytes,
                                int N, int H, int W, int accumulate, int dtype, void* stream) {
    const int esz = dtype == WU_BF16 ? 2 : 4;
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16, "stem7x7_wgrad: bad dtype");
    WU_REQUIRE(N > 0 && H > 0 && W > 0 && lddy >= 64 && x_nchw && dy && dw_oihw && (lddy * esz) % 16 == 0, "stem7x7_wgrad: bad arguments");
    const StemWgPlan p = stem_wgrad_plan(N, H, W);
    WU_REQUIRE(workspace && workspace_bytes >= p.ws && ((uintptr_t)workspace % 16) == 0, "stem7x7_wgrad: workspace too small (%zu < %zu)", workspace_bytes, p.ws);
    hipStream_t s = (hipStream_t)stream;
    TRAIN_DISPATCH(dtype, hipLaunchKernelGGL(stem_wgrad_kernel<T>, dim3(p.splits), dim3(256), 0, s, x_nchw, (const T*)dy, lddy, N, H, W,
                                             (H - 1) / 2 + 1, (W - 1) / 2 + 1, p.pix_per_split, (float*)workspace));
    const long long n = 64LL * kStTaps;
    hipLaunchKernelGGL(slab_fold_kernel, dim3(ew_grid(n)), dim3(256), 0, s, (const float*)workspace, p.splits, n, dw_oihw, accumulate);
    WU_LAUNCH_CHECK("stem7x7_wgrad");
    return 0;
}
