// What the image encoders (jpeg_enc.hip, png_enc.hip) share: the conversion of a source sample to a byte and the workgroup prefix sum.
#pragma once
#include "wu_common.h"

namespace {

static_assert(WU_JPEG_ENC_U8 == WU_PNG_ENC_U8, "the encoders share one sample code for uint8");
constexpr int kCodecU8 = WU_JPEG_ENC_U8;   // sample type of the source besides WU_F32 / WU_BF16

// ---- samples ------------------------------------------------------------------------------------------------------------------
// the byte wu.infer_driver.to_uint8 makes of a float sample: x * 255 in the tensor's own precision, clamp to [0, 255], truncate
__device__ __forceinline__ int float_byte(float x) {
    const float v = x * 255.f;
    return v >= 255.f ? 255 : (v > 0.f ? (int)v : 0);             // NaN -> 0
}
template <int DT> __device__ __forceinline__ int load_byte(const void* p, long long i);
template <> __device__ __forceinline__ int load_byte<kCodecU8>(const void* p, long long i) { return ((const uint8_t*)p)[i]; }
template <> __device__ __forceinline__ int load_byte<WU_F32>(const void* p, long long i) { return float_byte(((const float*)p)[i]); }
template <> __device__ __forceinline__ int load_byte<WU_BF16>(const void* p, long long i) {
    const float v = bf16_to_f32(f32_to_bf16(bf16_to_f32(((const bf16_t*)p)[i]) * 255.f));     // the product is rounded to bf16, as torch does
    return v >= 255.f ? 255 : (v > 0.f ? (int)v : 0);
}

// inclusive prefix sum over the 256 threads of a workgroup (Hillis-Steele in LDS)
__device__ __forceinline__ unsigned block_scan_inclusive(unsigned v, unsigned* sm, int tid) {
    sm[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned add = tid >= off ? sm[tid - off] : 0u;
        __syncthreads();
        sm[tid] += add;
        __syncthreads();
    }
    return sm[tid];
}

}  // namespace
