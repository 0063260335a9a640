// Baseline JPEG decoding for the input pipeline (replaces Image.open(path).convert('RGB') of dataset.py:64-67, 92-96, 128-129, 148-149).
//
// Two halves:
//   * HOST (plain C++, re-entrant, no global mutable state, no allocation): marker parsing and Huffman decoding -- the part of JPEG
//     that is sequential by construction.  Output: quantised int16 coefficients, one 64-entry block after the other in NATURAL
//     (row-major) order, component planes one after the other, blocks of a plane in raster order; plus the quantisation tables.
//   * DEVICE (two launches for a whole batch): (a) dequantise + 8x8 inverse DCT into uint8 component planes, (b) chroma upsampling
//     + YCbCr -> RGB + interleave + zero padding straight into the (N, Hmax, Wmax, 3) uint8 batch GPUInputPipeline consumes.
//
// The arithmetic is libjpeg's default decode path (what Pillow runs), integer throughout, so results equal Pillow's byte for byte:
// jidctint's "islow" IDCT (CONST_BITS 13, PASS1_BITS 2), "fancy" (triangle) h2v1 / h2v2 chroma upsampling evaluated on the
// component's true down-sampled size, plain replication when that width is <= 2, jdcolor's 16.16 fixed-point colour tables.
//
// The host half lives in jpeg_host.h (no HIP in it, so a plain C++ compiler can build it alone); with WU_JPEG_ALLOW_PROGRESSIVE it also
// runs the scans of a progressive file into the same coefficient buffer, and with WU_JPEG_ALLOW_H1V2 the colour kernel up-samples the
// chroma of a 4:4:0 file (libjpeg-turbo's h1v2 fancy rule).  Neither changes the IDCT kernel or the descriptor.
#include "wu_common.h"

#include "jpeg_host.h"

// ---- device -----------------------------------------------------------------------------------------------------------------------
namespace {

struct JpegDesc {              // one per image, 16 ints (wu/jpeg.py fills it)
    int first_block;           // first 64-entry block of the image in the coefficient buffer; also its plane storage / 64 in the workspace
    int h, w, mode;
    int bw_y, bh_y, bw_c, bh_c;    // blocks per row / rows of the luma and of each chroma plane (MCU-padded)
    int first_tile;            // first IDCT workgroup (32 blocks each) of the image
    int nblocks;               // blocks of the image (all components)
    int pad[6];
};

constexpr int kTileBlocks = 32;

#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// one 1-D pass of jidctint.c (jpeg_idct_islow); out[i] = DESCALE(., SHIFT)
template <int SHIFT> __device__ __forceinline__ void idct_pass(const int* in, int* out) {
    int z2 = in[2], z3 = in[6];
    int z1 = (z2 + z3) * FIX_0_541196100;
    int tmp2 = z1 + z3 * (-FIX_1_847759065);
    int tmp3 = z1 + z2 * FIX_0_765366865;
    int tmp0 = (in[0] + in[4]) * 8192;
    int tmp1 = (in[0] - in[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 *= FIX_0_298631336; tmp1 *= FIX_2_053119869; tmp2 *= FIX_3_072711026; tmp3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    out[0] = (tmp10 + tmp3 + R) >> SHIFT; out[7] = (tmp10 - tmp3 + R) >> SHIFT;
    out[1] = (tmp11 + tmp2 + R) >> SHIFT; out[6] = (tmp11 - tmp2 + R) >> SHIFT;
    out[2] = (tmp12 + tmp1 + R) >> SHIFT; out[5] = (tmp12 - tmp1 + R) >> SHIFT;
    out[3] = (tmp13 + tmp0 + R) >> SHIFT; out[4] = (tmp13 - tmp0 + R) >> SHIFT;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// (a) dequantise + IDCT.  One workgroup = 32 blocks of ONE image (tile_image[] names it: no search), 8 lanes per block.
// Lane r loads ROW r of its block as one 16-byte load, the block is transposed through LDS (rows padded to 9 words) for the column
// pass, written back in place, and lane r then runs the row pass on row r and stores its 8 output bytes as one 8-byte store.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const JpegDesc* __restrict__ desc,
                                                        const int* __restrict__ tile_image, const uint16_t* __restrict__ qtab,
                                                        uint8_t* __restrict__ planes) {
    __shared__ int s[kTileBlocks][8][9];
    const int tile = blockIdx.x, tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    const int n = tile_image[tile];
    const JpegDesc d = desc[n];
    const int b = (tile - d.first_tile) * kTileBlocks + lb;
    const bool valid = b < d.nblocks;
    const int ny = d.bw_y * d.bh_y, nc = d.bw_c * d.bh_c;
    int c = 0, bb = b, bw = d.bw_y;
    if (b >= ny) {
        c = b < ny + nc ? 1 : 2;
        bb = b - ny - (c - 1) * nc;
        bw = d.bw_c;
    }
    if (valid) {
        const uint4 cv = *reinterpret_cast<const uint4*>(coef + ((size_t)d.first_block + b) * 64 + r * 8);
        const uint4 qv = *reinterpret_cast<const uint4*>(qtab + ((size_t)n * 3 + c) * 64 + r * 8);
        const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[lb][r][2 * k] = (int)(short)(cw[k] & 0xffffu) * (int)(qw[k] & 0xffffu);
            s[lb][r][2 * k + 1] = ((int)cw[k] >> 16) * (int)(qw[k] >> 16);
        }
    }
    __syncthreads();
    int in[8], out[8];
    if (valid) {
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j] = s[lb][j][r];           // column r
        idct_pass<11>(in, out);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[lb][j][r] = out[j];          // the same words this lane just read
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int j = 0; j < 8; ++j) in[j] = s[lb][r][j];           // row r
        idct_pass<18>(in, out);
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo |= (unsigned)clamp255(out[j] + 128) << (8 * j);
            hi |= (unsigned)clamp255(out[4 + j] + 128) << (8 * j);
        }
        const int by = bb / bw, bx = bb - by * bw;
        uint8_t* plane = planes + (size_t)d.first_block * 64 + (size_t)(b - bb) * 64;      // b - bb = blocks of the planes before this one
        *reinterpret_cast<uint2*>(plane + (size_t)(by * 8 + r) * (bw * 8) + bx * 8) = make_uint2(lo, hi);
    }
}

// one up-sampled chroma sample at full-resolution (x, y); pw = row stride of the plane, dw x dh = the component's true size
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ pl, int pw, int mode, int x, int y, int dw, int dh) {
    if (mode == WU_JPEG_MODE_444) return pl[(size_t)y * pw + x];
    if (mode == WU_JPEG_MODE_H1V2) {                               // jdsample.c h1v2_fancy_upsample: 3/4 nearer row + 1/4 farther row, any width
        const int r = y >> 1;
        const int nb = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
        return (3 * pl[(size_t)r * pw + x] + pl[(size_t)nb * pw + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    const int i = x >> 1;
    if (mode == WU_JPEG_MODE_H2V1) {
        const uint8_t* row = pl + (size_t)y * pw;
        const int v = row[i];
        if (dw <= 2) return v;
        if (x & 1) return i == dw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
        return i == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    if (dw <= 2) return pl[(size_t)r * pw + i];
    const int nb = (y & 1) ? (r + 1 < dh ? r + 1 : dh - 1) : (r > 0 ? r - 1 : 0);
    const uint8_t* r0 = pl + (size_t)r * pw;
    const uint8_t* r1 = pl + (size_t)nb * pw;
    const int cs = 3 * r0[i] + r1[i];
    if (x & 1) {
        if (i == dw - 1) return (4 * cs + 7) >> 4;
        return (3 * cs + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    }
    if (i == 0) return (4 * cs + 8) >> 4;
    return (3 * cs + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

// RGB of batch pixel (n, y, x) packed as R | G << 8 | B << 16; zero outside the image
__device__ __forceinline__ unsigned jpeg_pixel(const uint8_t* __restrict__ planes, const JpegDesc& d, int y, int x) {
    if (y >= d.h || x >= d.w) return 0u;
    const uint8_t* py = planes + (size_t)d.first_block * 64;
    const int pwy = d.bw_y * 8;
    const int Y = py[(size_t)y * pwy + x];
    if (d.mode == WU_JPEG_MODE_GREY) return (unsigned)Y * 0x010101u;
    const int pwc = d.bw_c * 8;
    const size_t csz = (size_t)d.bw_c * d.bh_c * 64;
    const uint8_t* pcb = py + (size_t)d.bw_y * d.bh_y * 64;
    const int dw = d.mode == WU_JPEG_MODE_444 || d.mode == WU_JPEG_MODE_H1V2 ? d.w : (d.w + 1) >> 1;
    const int dh = d.mode == WU_JPEG_MODE_H2V2 || d.mode == WU_JPEG_MODE_H1V2 ? (d.h + 1) >> 1 : d.h;
    const int cb = chroma_at(pcb, pwc, d.mode, x, y, dw, dh) - 128;
    const int cr = chroma_at(pcb + csz, pwc, d.mode, x, y, dw, dh) - 128;
    // jdcolor.c build_ycc_rgb_table: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554
    const int R = clamp255(Y + ((91881 * cr + 32768) >> 16));
    const int G = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    const int B = clamp255(Y + ((116130 * cb + 32768) >> 16));
    return (unsigned)R | ((unsigned)G << 8) | ((unsigned)B << 16);
}

// (b) upsample + colour + interleave + pad.  Thread t owns batch pixels 4t .. 4t+3 of the flat (N*Hmax*Wmax) pixel array = bytes
// 12t .. 12t+11: always dword aligned whatever Wmax is, stored as three dwords.  The four pixels may straddle a row or an image.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ planes, const JpegDesc* __restrict__ desc,
                                                         uint8_t* __restrict__ out, int Hmax, int Wmax, long long npix) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p0 = t * 4;
    if (p0 >= npix) return;
    const unsigned per = (unsigned)Hmax * (unsigned)Wmax;                               // < 2^31 (host check)
    int n = (int)(p0 / per);
    const unsigned rem = (unsigned)(p0 - (long long)n * per);
    int y = (int)(rem / (unsigned)Wmax), x = (int)(rem - (unsigned)y * (unsigned)Wmax);
    JpegDesc d = desc[n];
    unsigned px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k] = p0 + k < npix ? jpeg_pixel(planes, d, y, x) : 0u;
        if (++x == Wmax) {
            x = 0;
            if (++y == Hmax) {
                y = 0;
                ++n;
                if (p0 + k + 1 < npix) d = desc[n];
            }
        }
    }
    if (p0 + 4 <= npix) {
        unsigned* o = reinterpret_cast<unsigned*>(out + p0 * 3);
        o[0] = px[0] | (px[1] << 24);
        o[1] = (px[1] >> 8) | (px[2] << 16);
        o[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int k = 0; p0 + k < npix; ++k) {
            out[(p0 + k) * 3] = (uint8_t)px[k];
            out[(p0 + k) * 3 + 1] = (uint8_t)(px[k] >> 8);
            out[(p0 + k) * 3 + 2] = (uint8_t)(px[k] >> 16);
        }
    }
}

}  // namespace

extern "C" size_t wu_jpeg_desc_bytes(void) { return sizeof(JpegDesc); }

extern "C" size_t wu_jpeg_workspace_bytes(long long total_blocks) { return total_blocks > 0 ? (size_t)total_blocks * 64 : 0; }

extern "C" int wu_jpeg_reconstruct(const int16_t* coef_dev, const void* desc_dev, const int* tile_image_dev, const uint16_t* qtab_dev,
                                   void* workspace, size_t workspace_bytes, uint8_t* out_u8, int N, int Hmax, int Wmax, int n_tiles,
                                   void* stream) {
    WU_REQUIRE(coef_dev && desc_dev && tile_image_dev && qtab_dev && workspace && out_u8, "jpeg_reconstruct: null argument");
    WU_REQUIRE(N > 0 && Hmax > 0 && Wmax > 0 && Hmax <= 65535 && Wmax <= 65535 && n_tiles >= 0, "jpeg_reconstruct: bad shape N=%d Hmax=%d Wmax=%d tiles=%d",
               N, Hmax, Wmax, n_tiles);
    WU_REQUIRE((long long)Hmax * Wmax < (1ll << 31) && (long long)n_tiles * 32 < (1ll << 31), "jpeg_reconstruct: batch too large");
    WU_REQUIRE(workspace_bytes >= wu_jpeg_workspace_bytes((long long)n_tiles * 32), "jpeg_reconstruct: workspace too small");
    WU_REQUIRE(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)qtab_dev & 15) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)out_u8 & 3) == 0,
               "jpeg_reconstruct: misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    if (n_tiles > 0)                                               // 0: every image of the batch was decoded elsewhere (h = w = 0 slots)
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3(n_tiles), dim3(256), 0, s, coef_dev, (const JpegDesc*)desc_dev, tile_image_dev, qtab_dev,
                           (uint8_t*)workspace);
    const long long npix = (long long)N * Hmax * Wmax;
    const long long threads = (npix + 3) / 4;
    WU_REQUIRE((threads + 255) / 256 < (1ll << 31), "jpeg_reconstruct: batch too large");
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (const uint8_t*)workspace,
                       (const JpegDesc*)desc_dev, out_u8, Hmax, Wmax, npix);
    WU_LAUNCH_CHECK("jpeg_reconstruct");
    return 0;
}
