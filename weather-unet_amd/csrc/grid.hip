// Image grids and tables for the encoders: torchvision.utils.make_grid(..., normalize=True, scale_each=True) as the reference's
// drivers call it (demo.py:74-82, t_cls_train.py:361-378, t_est_train.py:342), composed on the device in three launches whatever the
// number of cells and frames.
//
// A table is a list of CELLS (wu_grid_cell, include/wu_kernels.h): a source image with its element strides, the frame it goes to and
// where, a normalisation group, flags.  The kernels are bytes-bound streaming kernels:
//   grid_init_kernel     fills the output with pad_value and resets the per-group range slots
//   grid_range_kernel    min / max of every group over all its cells: per-thread, per-wave (shuffles), per-workgroup (LDS), then ONE
//                        atomicMin / atomicMax per workgroup on the order-preserving unsigned image of the float -- min and max do not
//                        depend on the order, so the result does not depend on the launch geometry
//   grid_compose_kernel  clamp / subtract / divide per pixel and the write, fp32 planar or uint8 interleaved
// Thread mapping: one wave per pixel row of a cell, a lane per run of four pixels; the runs start where the OUTPUT is 16-byte (fp32)
// or 4-byte (uint8: four pixels are twelve bytes, three whole dwords) aligned, and a run whose source is contiguous is read with one
// 16-byte (fp32) / 8-byte (bf16) load per channel wherever it starts on a dword: a global vector load needs no more than that, so the
// load does not depend on the phase between source and output (with make_grid's padding of 2 the two never coincide).  Heads, tails,
// strided sources and bf16 runs that start on an odd element take the element path.
//
// NaN in a source: the range of its group is unspecified (fminf / fmaxf drop NaNs, the integer image orders them outside the
// infinities), and so is every pixel normalised by it.  No attempt is made to match torch there.
#include "wu_common.h"

#pragma clang fp contract(off)      // every operation below is one IEEE fp32 operation, in the order written

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTargetBlocks = 4096;

// a cell the kernels follow: positive size, inside its frame (64-bit sums: the descriptor is device memory, nothing about it is trusted)
__device__ __forceinline__ bool cell_ok(const wu_grid_cell& c, int frames, int Hg, int Wg) {
    return c.h > 0 && c.w > 0 && c.frame >= 0 && c.frame < frames && c.y0 >= 0 && c.x0 >= 0 &&
           (long long)c.y0 + c.h <= Hg && (long long)c.x0 + c.w <= Wg && ((c.flags & WU_GRID_BLANK) || c.src != 0);
}
__device__ __forceinline__ bool reduces(const wu_grid_cell& c, int n_groups) {
    return (c.flags & WU_GRID_NORMALIZE) && !(c.flags & WU_GRID_FIXED_RANGE) && c.group >= 0 && c.group < n_groups;
}

// order-preserving map float -> uint32 (a < b as floats <=> enc(a) < enc(b) as unsigned; -0 sorts below +0)
__device__ __forceinline__ uint32_t enc_ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_ord(uint32_t e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

__device__ __forceinline__ float pre_transform(float x) { return (x + 1.f) * 127.5f; }      // demo.py:80
__device__ __forceinline__ uint8_t to_u8(float v) {                                         // grid.mul(255).clamp(0, 255).byte()
    v = v * 255.f;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return (uint8_t)(int)v;
}

// The sources arrive as integers inside the descriptors, so the compiler cannot know their address space: say it (global_load, not flat_load).
#define WU_GLOBAL __attribute__((address_space(1)))
// Vector loads need the alignment of a dword only (global memory): a run that starts where the OUTPUT is aligned is still one load.
typedef float f32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned u32x2_a4_t __attribute__((ext_vector_type(2), aligned(4)));

// Four pixels x .. x + 3 of one source row (`row`: element offset of its x = 0); only x in [0, w) is read, the rest is 0.
__device__ __forceinline__ void load4(uint64_t src, bool bf16, long long row, long long sx, int x, int w, float* f) {
    const bool full = x >= 0 && x + 4 <= w;
    if (!bf16) {
        const WU_GLOBAL float* p = (const WU_GLOBAL float*)(uintptr_t)src + row;
        if (full && sx == 1 && (((uintptr_t)(p + x)) & 3) == 0) {
            const f32x4_a4_t v = *(const WU_GLOBAL f32x4_a4_t*)(p + x);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (x + i >= 0 && x + i < w) ? p[(long long)(x + i) * sx] : 0.f;
    } else {
        const WU_GLOBAL bf16_t* p = (const WU_GLOBAL bf16_t*)(uintptr_t)src + row;
        if (full && sx == 1 && (((uintptr_t)(p + x)) & 3) == 0) {
            const u32x2_a4_t v = *(const WU_GLOBAL u32x2_a4_t*)(p + x);
            f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
            f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (x + i >= 0 && x + i < w) ? bf16_to_f32(p[(long long)(x + i) * sx]) : 0.f;
    }
}

// ---- launch 1: pad_value everywhere, range slots reset --------------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(kThreads) void grid_init_kernel(void* out, size_t out_elems, float pad_value, uint32_t* enc, float* pairs, int n_groups) {
    const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x, nth = (size_t)gridDim.x * kThreads;
    for (size_t g = tid; g < (size_t)n_groups; g += nth) {
        enc[2 * g] = 0xffffffffu;
        enc[2 * g + 1] = 0u;
        pairs[2 * g] = 0.f;
        pairs[2 * g + 1] = 0.f;
    }
    uint4 v;
    if (U8) {
        const uint32_t b = to_u8(pad_value);
        v.x = v.y = v.z = v.w = b * 0x01010101u;
    } else {
        v.x = v.y = v.z = v.w = __float_as_uint(pad_value);
    }
    const size_t bytes = out_elems * (U8 ? 1 : 4), n16 = bytes >> 4;
    uint4* o = (uint4*)out;
    for (size_t i = tid; i < n16; i += nth) o[i] = v;
    if (U8) {
        for (size_t i = (n16 << 4) + tid; i < bytes; i += nth) ((uint8_t*)out)[i] = (uint8_t)v.x;
    }       // fp32: 3 * Hg * Wg floats per frame at a 16-byte aligned base; a tail of up to 3 floats
    else {
        for (size_t i = (n16 << 2) + tid; i < out_elems; i += nth) ((float*)out)[i] = pad_value;
    }
}

// ---- launch 2: ranges -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_range_kernel(const wu_grid_cell* cells, int n_cells, int n_groups, int tiles, uint32_t* enc,
                                                              int frames, int Hg, int Wg) {
    const int ci = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    if (ci >= n_cells) return;
    const wu_grid_cell c = cells[ci];
    if (!cell_ok(c, frames, Hg, Wg) || !reduces(c, n_groups)) return;
    if (c.flags & WU_GRID_BLANK) {                       // zeros that count in the range, nothing to read
        if (tile == 0 && threadIdx.x == 0) {
            atomicMin(&enc[2 * c.group], enc_ord(0.f));
            atomicMax(&enc[2 * c.group + 1], enc_ord(0.f));
        }
        return;
    }
    const int rows = 3 * c.h;
    if (tile * kWaves >= rows) return;                   // workgroup-uniform: no barrier is skipped by part of a workgroup
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool bf16 = c.flags & WU_GRID_BF16;
    const uint64_t src = c.src;
    float lo = INFINITY, hi = -INFINITY;
    for (int r = tile * kWaves + wave; r < rows; r += tiles * kWaves) {
        const int ch = r / c.h, y = r - ch * c.h;
        const long long row = (long long)ch * c.sc + (long long)y * c.sy;
        // runs of four start where the SOURCE is 16-byte aligned (contiguous rows; any phase otherwise)
        int p = 0;
        if (c.sx == 1) {
            const uint64_t a = src + (uint64_t)(row * (bf16 ? 2 : 4));
            p = bf16 ? (int)(((8 - (a & 7)) & 7) >> 1) : (int)(((16 - (a & 15)) & 15) >> 2);
        }
        for (int x = (p ? p - 4 : 0) + 4 * lane; x < c.w; x += 256) {
            float f[4];
            load4(src, bf16, row, c.sx, x, c.w, f);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i >= 0 && x + i < c.w) { lo = fminf(lo, f[i]); hi = fmaxf(hi, f[i]); }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m, 64));
        hi = fmaxf(hi, __shfl_xor(hi, m, 64));
    }
    __shared__ float s_lo[kWaves], s_hi[kWaves];
    if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kWaves; ++i) { lo = fminf(lo, s_lo[i]); hi = fmaxf(hi, s_hi[i]); }
        if (lo <= hi) {                                  // at least one value seen
            // the pre-transform is monotone: transform the two results, not every value (same bits)
            if (c.flags & WU_GRID_PRE) { lo = pre_transform(lo); hi = pre_transform(hi); }
            atomicMin(&enc[2 * c.group], enc_ord(lo));
            atomicMax(&enc[2 * c.group + 1], enc_ord(hi));
        }
    }
}

// ---- launch 3: compose ----------------------------------------------------------------------------------------------------------------
struct Norm { bool pre, on; float lo, hi, den; };
__device__ __forceinline__ float norm1(float x, const Norm& n) {
    if (n.pre) x = pre_transform(x);
    if (n.on) {
        const float v = fminf(fmaxf(x, n.lo), n.hi);     // clamp(x, lo, hi)
        x = (v - n.lo) / n.den;                          // true division, correctly rounded
    }
    return x;
}

template <bool U8>
__global__ __launch_bounds__(kThreads) void grid_compose_kernel(const wu_grid_cell* cells, int n_cells, int n_groups, int tiles, const uint32_t* enc,
                                                                float* pairs, void* out, int frames, int Hg, int Wg) {
    const int ci = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    if (ci >= n_cells) return;
    const wu_grid_cell c = cells[ci];
    if (!cell_ok(c, frames, Hg, Wg)) return;
    Norm nm;
    nm.pre = (c.flags & WU_GRID_PRE) && !(c.flags & WU_GRID_BLANK);
    nm.on = c.flags & WU_GRID_NORMALIZE;
    nm.lo = 0.f; nm.hi = 1.f;
    if (nm.on) {
        if (c.flags & WU_GRID_FIXED_RANGE) { nm.lo = c.lo; nm.hi = c.hi; }
        else if (c.group >= 0 && c.group < n_groups) { nm.lo = dec_ord(enc[2 * c.group]); nm.hi = dec_ord(enc[2 * c.group + 1]); }
        else return;                                     // no such group: the cell is ignored, as in the range launch
        if (tile == 0 && threadIdx.x == 0 && c.group >= 0 && c.group < n_groups) {     // for tests and tools; every cell of a group writes the same pair
            pairs[2 * c.group] = nm.lo;
            pairs[2 * c.group + 1] = nm.hi;
        }
    }
    nm.den = nm.hi - nm.lo + 1e-5f;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool bf16 = c.flags & WU_GRID_BF16, blank = c.flags & WU_GRID_BLANK;
    const uint64_t src = c.src;
    const int rows = U8 ? c.h : 3 * c.h;                 // uint8: a row of pixels (three channels each); fp32: a row of one plane
    for (int r = tile * kWaves + wave; r < rows; r += tiles * kWaves) {
        if (U8) {
            const int y = r;
            const size_t ob = (((size_t)c.frame * Hg + (size_t)(c.y0 + y)) * Wg + (size_t)c.x0) * 3;     // byte offset of pixel x = 0
            const int p = (int)(ob & 3);                 // (ob + 3 x) % 4 == 0 for x = p + 4 k
            uint8_t* o = (uint8_t*)out + ob;
            for (int x = (p ? p - 4 : 0) + 4 * lane; x < c.w; x += 256) {
                float f[3][4];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    if (blank) { f[ch][0] = f[ch][1] = f[ch][2] = f[ch][3] = 0.f; }
                    else load4(src, bf16, (long long)ch * c.sc + (long long)y * c.sy, c.sx, x, c.w, f[ch]);
                }
                uint8_t b[12];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) b[3 * i + ch] = to_u8(norm1(f[ch][i], nm));
                if (x >= 0 && x + 4 <= c.w) {
                    struct __attribute__((aligned(4))) u3 { uint32_t a, b, c; };
                    u3 v;
                    v.a = b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
                    v.b = b[4] | (b[5] << 8) | (b[6] << 16) | ((uint32_t)b[7] << 24);
                    v.c = b[8] | (b[9] << 8) | (b[10] << 16) | ((uint32_t)b[11] << 24);
                    *(u3*)(o + (size_t)x * 3) = v;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (x + i >= 0 && x + i < c.w) {
                            uint8_t* q = o + (size_t)(x + i) * 3;
                            q[0] = b[3 * i]; q[1] = b[3 * i + 1]; q[2] = b[3 * i + 2];
                        }
                }
            }
        } else {
            const int ch = r / c.h, y = r - ch * c.h;
            const size_t oe = (((size_t)c.frame * 3 + ch) * Hg + (size_t)(c.y0 + y)) * Wg + (size_t)c.x0;  // element offset of x = 0
            const int p = (int)((4 - (oe & 3)) & 3);
            float* o = (float*)out + oe;
            const long long row = (long long)ch * c.sc + (long long)y * c.sy;
            for (int x = (p ? p - 4 : 0) + 4 * lane; x < c.w; x += 256) {
                float f[4];
                if (blank) { f[0] = f[1] = f[2] = f[3] = 0.f; }
                else load4(src, bf16, row, c.sx, x, c.w, f);
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = norm1(f[i], nm);
                if (x >= 0 && x + 4 <= c.w) {
                    *(float4*)(o + x) = make_float4(f[0], f[1], f[2], f[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (x + i >= 0 && x + i < c.w) o[x + i] = f[i];
                }
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
constexpr int kMaxCells = 1 << 20, kMaxGroups = 1 << 20, kMaxSide = 1 << 20, kMaxFrames = 1 << 20;
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Layout { size_t off_enc, off_pairs, total; };
bool make_layout(int n_cells, int n_groups, Layout& L) {
    if (n_cells < 1 || n_cells > kMaxCells || n_groups < 1 || n_groups > kMaxGroups) return false;
    L.off_enc = 0;
    L.off_pairs = align256((size_t)n_groups * 8);
    L.total = L.off_pairs + align256((size_t)n_groups * 8);
    return true;
}
int tiles_for(int n_cells, long long rows_max) {
    long long t = kTargetBlocks / n_cells, cap = (rows_max + kWaves - 1) / kWaves;
    if (t > cap) t = cap;
    return t < 1 ? 1 : (int)t;
}

}  // namespace

static_assert(sizeof(wu_grid_cell) == 72, "wu_grid_cell is 72 bytes (include/wu_kernels.h, wu/grid.py)");

extern "C" size_t wu_grid_cell_bytes(void) { return sizeof(wu_grid_cell); }

extern "C" size_t wu_grid_workspace_bytes(int n_cells, int n_groups) {
    Layout L;
    return make_layout(n_cells, n_groups, L) ? L.total : 0;
}

extern "C" int wu_grid_workspace_layout(int n_cells, int n_groups, long long* out2) {
    Layout L;
    WU_REQUIRE(out2, "grid_workspace_layout: null argument");
    WU_REQUIRE(make_layout(n_cells, n_groups, L), "grid_workspace_layout: bad counts n_cells=%d n_groups=%d", n_cells, n_groups);
    out2[0] = (long long)L.off_pairs;
    out2[1] = (long long)L.off_enc;
    return 0;
}

extern "C" int wu_grid_compose(const void* cells_dev, int n_cells, int n_groups, void* workspace, size_t workspace_bytes, void* out,
                               size_t out_bytes, int out_kind, int frames, int Hg, int Wg, float pad_value, void* stream) {
    Layout L;
    WU_REQUIRE(make_layout(n_cells, n_groups, L), "grid_compose: bad counts n_cells=%d n_groups=%d (1 .. %d each)", n_cells, n_groups, kMaxCells);
    WU_REQUIRE(frames >= 1 && frames <= kMaxFrames && Hg >= 1 && Hg <= kMaxSide && Wg >= 1 && Wg <= kMaxSide,
               "grid_compose: bad geometry frames=%d Hg=%d Wg=%d", frames, Hg, Wg);
    WU_REQUIRE(out_kind == WU_GRID_OUT_F32 || out_kind == WU_GRID_OUT_U8, "grid_compose: out_kind %d is not fp32 planar (0) / uint8 interleaved (1)", out_kind);
    // every factor is at most 2^20 (checked above): the product fits 64 bits
    const uint64_t need64 = (uint64_t)frames * (uint64_t)Hg * (uint64_t)Wg * (out_kind == WU_GRID_OUT_F32 ? 12u : 3u);
    WU_REQUIRE(need64 < (1ull << 46), "grid_compose: frames=%d Hg=%d Wg=%d is too large", frames, Hg, Wg);
    const size_t need = (size_t)need64;
    WU_REQUIRE(out_bytes >= need, "grid_compose: output too small (%zu of %zu bytes)", out_bytes, need);
    WU_REQUIRE(workspace_bytes >= L.total, "grid_compose: workspace too small (%zu of %zu bytes)", workspace_bytes, L.total);
    WU_REQUIRE(cells_dev && workspace && out, "grid_compose: null argument");
    WU_REQUIRE(((uintptr_t)cells_dev & 7) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out & 15) == 0,
               "grid_compose: descriptors must be 8-byte aligned, workspace and output 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const wu_grid_cell* cells = (const wu_grid_cell*)cells_dev;
    uint32_t* enc = (uint32_t*)((uint8_t*)workspace + L.off_enc);
    float* pairs = (float*)((uint8_t*)workspace + L.off_pairs);
    const bool u8 = out_kind == WU_GRID_OUT_U8;
    const size_t out_elems = need / (u8 ? 1 : 4);

    size_t fill_blocks = (need / 16 + kThreads - 1) / kThreads;
    if (fill_blocks > 2048) fill_blocks = 2048;
    if (fill_blocks < 1) fill_blocks = 1;
    wu_prof_pre(WU_FAM_GRID, s);
    if (u8) hipLaunchKernelGGL(grid_init_kernel<true>, dim3((unsigned)fill_blocks), dim3(kThreads), 0, s, out, out_elems, pad_value, enc, pairs, n_groups);
    else hipLaunchKernelGGL(grid_init_kernel<false>, dim3((unsigned)fill_blocks), dim3(kThreads), 0, s, out, out_elems, pad_value, enc, pairs, n_groups);
    wu_prof_post(WU_FAM_GRID, s, 0.0, (double)need);
    WU_LAUNCH_CHECK("grid_init_kernel");

    const int rt = tiles_for(n_cells, 3ll * Hg);
    wu_prof_pre(WU_FAM_GRID, s);
    hipLaunchKernelGGL(grid_range_kernel, dim3((unsigned)((long long)n_cells * rt)), dim3(kThreads), 0, s, cells, n_cells, n_groups, rt, enc, frames, Hg, Wg);
    wu_prof_post(WU_FAM_GRID, s, 0.0, 0.0);
    WU_LAUNCH_CHECK("grid_range_kernel");

    const int ct = tiles_for(n_cells, u8 ? (long long)Hg : 3ll * Hg);
    wu_prof_pre(WU_FAM_GRID, s);
    if (u8) hipLaunchKernelGGL(grid_compose_kernel<true>, dim3((unsigned)((long long)n_cells * ct)), dim3(kThreads), 0, s, cells, n_cells, n_groups, ct, enc, pairs, out, frames, Hg, Wg);
    else hipLaunchKernelGGL(grid_compose_kernel<false>, dim3((unsigned)((long long)n_cells * ct)), dim3(kThreads), 0, s, cells, n_cells, n_groups, ct, enc, pairs, out, frames, Hg, Wg);
    wu_prof_post(WU_FAM_GRID, s, 0.0, 0.0);
    WU_LAUNCH_CHECK("grid_compose_kernel");
    return 0;
}
