// Baseline JPEG encoding of image batches on the GPU (replaces the save_image(output, '....jpg', normalize=True) that ends
// inference/inf_transfer_c.py:119-120, inf_transfer_e.py:141-142 and inf_1year_signals.py:105: one Pillow Image.save per image).
//
// The mirror image of jpeg.hip.  Baseline encoding is parallel from end to end -- a block's code length depends on its own coefficients
// and its predecessor's DC only, and a prefix sum places every block in the bit stream -- so all of it runs on the device, five launches
// for a whole batch whatever N and the image sizes:
//   1. transform: samples (u8 / f32 / bf16 through arbitrary element strides) -> RGB bytes -> YCbCr -> h2v2 chroma downsampling ->
//      level shift -> 8x8 forward DCT -> quantisation; int16 blocks in zig-zag order, stored in SCAN order (MCU-interleaved), dummy
//      blocks materialised.  Also zeroes the image's raw bit-stream slot.
//   2. size: one thread per block counts its Huffman bits; exclusive prefix sum inside a 256-block tile, one total per tile.
//   3. pack: a tile adds up the totals of the tiles in front of it and every thread ORs its block's bits into the zeroed slot at its
//      bit offset, MSB first; the last block fills the final byte with ones.
//   4. count: 0xFF bytes per 4 KiB chunk of the raw stream.
//   5. frame: header, the chunk's bytes with 0x00 stuffed behind every 0xFF (offsets from the chunk counts), FF D9, byte count.
// The host part (quantisation tables, header) is plain C++ and works without a GPU.
//
// The arithmetic is libjpeg's default compress path, which is what Pillow runs (quality scaling of the Annex K tables forced to
// baseline, jccolor's 16.16 fixed point, jcsample's h2v2_downsample with its alternating bias and its asymmetric edge padding,
// jfdctint's "islow" DCT, quantisation by true integer division, jccoefct's dummy blocks, the Annex K Huffman tables), integer
// throughout, so the files equal Pillow's byte for byte.
#include "codec_internal.h"

namespace {

constexpr int kHeaderBytes = 623;          // SOI 2 + APP0 18 + DQT 2 x 69 + SOF0 19 + DHT 33 + 183 + 33 + 183 + SOS 14
constexpr int kXformBlocks = 32;           // blocks per transform workgroup, 8 lanes each
constexpr int kTileBlocks = 256;           // blocks per size / pack workgroup, one thread each
constexpr int kChunkBytes = 4096;          // raw bytes per count / frame workgroup, 16 per thread

constexpr uint8_t kZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 quantisation tables, natural order
constexpr uint8_t kQLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                  99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3 Huffman tables: 16 code-length counts, then the symbols in code order
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// symbol -> code | length << 16 (Annex C), built at compile time
struct EncTab { uint32_t e[256]; };
struct InvZigZag { uint8_t pos[64]; };
constexpr EncTab make_enc_tab(const uint8_t* bits, const uint8_t* vals) {
    EncTab t = {};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) t.e[vals[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
    return t;
}
constexpr InvZigZag make_inv_zigzag() {
    InvZigZag z = {};
    for (int i = 0; i < 64; ++i) z.pos[kZigZag[i]] = (uint8_t)i;
    return z;
}
// 0 DC luma, 1 DC chroma, 2 AC luma, 3 AC chroma
__device__ const EncTab kEncTab[4] = {make_enc_tab(kDcLumaBits, kDcVals), make_enc_tab(kDcChromaBits, kDcVals),
                                      make_enc_tab(kAcLumaBits, kAcLumaVals), make_enc_tab(kAcChromaBits, kAcChromaVals)};
__device__ const InvZigZag kInvZigZag = make_inv_zigzag();      // natural index -> position in the zig-zag sequence

struct JpegEncDesc {           // 16 bytes per image, built by the caller
    int h, w;
    int capacity;              // bytes the entropy-coded data of this image may take (stuffing included)
    int pad;
};

// what the kernels derive from a descriptor; h, w and capacity are clamped to the batch bounds so that a bad descriptor cannot make
// a kernel leave its buffers
struct Geo {
    int h, w, mx, my, bpm, nblocks, bw_y, bh_y;
    unsigned cap;
};
__device__ __forceinline__ Geo make_geo(const JpegEncDesc d, int Hmax, int Wmax, long long cap_max, bool s420) {
    Geo g;
    g.h = min(max(d.h, 1), Hmax);
    g.w = min(max(d.w, 1), Wmax);
    const int m = s420 ? 16 : 8;
    g.mx = (g.w + m - 1) / m;
    g.my = (g.h + m - 1) / m;
    g.bpm = s420 ? 6 : 3;
    g.nblocks = g.mx * g.my * g.bpm;
    g.bw_y = (g.w + 7) >> 3;
    g.bh_y = (g.h + 7) >> 3;
    g.cap = (unsigned)min((long long)max(d.capacity, 0), cap_max);
    return g;
}

// ---- samples (float_byte / load_byte<DT>: codec_internal.h) ------------------------------------------------------------------
// jccolor.c rgb_ycc_convert, FIX(x) = (int)(x * 65536 + 0.5)
__device__ __forceinline__ int ycc(int r, int g, int b, int comp) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// RGB bytes of the 8 pixels x0 .. x0 + 7 (x0 a multiple of 8) of one row, columns clamped to w - 1.  `vec`: the layout allows wide
// loads (fp32 planes with unit pixel stride and 16-byte aligned rows: two 16-byte loads per channel; interleaved uint8 with 4-byte
// aligned rows: six dwords); a run that touches the right edge takes the element-wise path.
template <int DT>
__device__ __forceinline__ void fetch8(const void* __restrict__ src, long long row, int x0, int w, long long sc, long long sx, bool vec,
                                       int* R, int* G, int* B) {
    if (DT == WU_F32 && vec && x0 + 8 <= w) {
        int* const out[3] = {R, G, B};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4* p = (const float4*)((const float*)src + row + c * sc + x0);
            const float4 a = p[0], b = p[1];
            out[c][0] = float_byte(a.x); out[c][1] = float_byte(a.y); out[c][2] = float_byte(a.z); out[c][3] = float_byte(a.w);
            out[c][4] = float_byte(b.x); out[c][5] = float_byte(b.y); out[c][6] = float_byte(b.z); out[c][7] = float_byte(b.w);
        }
        return;
    }
    if (DT == WU_JPEG_ENC_U8 && vec && x0 + 8 <= w) {
        const uint32_t* p = (const uint32_t*)((const uint8_t*)src + row + (long long)x0 * 3);
        uint32_t v[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = p[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            R[i] = (int)((v[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255u);
            G[i] = (int)((v[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255u);
            B[i] = (int)((v[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255u);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long long at = row + (long long)min(x0 + i, w - 1) * sx;
        R[i] = load_byte<DT>(src, at);
        G[i] = load_byte<DT>(src, at + sc);
        B[i] = load_byte<DT>(src, at + 2 * sc);
    }
}

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

// one 1-D pass of jfdctint.c (jpeg_fdct_islow).  FIRST (rows): outputs 0 and 4 are << 2, the others DESCALE(., 11);
// second (columns): outputs 0 and 4 are DESCALE(., 2), the others DESCALE(., 15)
template <bool FIRST> __device__ __forceinline__ void fdct_pass(const int* d, int* out) {
    constexpr int SH = FIRST ? 11 : 15, R = 1 << (SH - 1);
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        out[0] = (tmp10 + tmp11) * 4;
        out[4] = (tmp10 - tmp11) * 4;
    } else {
        out[0] = (tmp10 + tmp11 + 2) >> 2;
        out[4] = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * FIX_0_541196100;
    out[2] = (z1 + tmp13 * FIX_0_765366865 + R) >> SH;
    out[6] = (z1 + tmp12 * (-FIX_1_847759065) + R) >> SH;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp4 *= FIX_0_298631336; tmp5 *= FIX_2_053119869; tmp6 *= FIX_3_072711026; tmp7 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    out[7] = (tmp4 + z1 + z3 + R) >> SH;
    out[5] = (tmp5 + z2 + z4 + R) >> SH;
    out[3] = (tmp6 + z2 + z3 + R) >> SH;
    out[1] = (tmp7 + z1 + z4 + R) >> SH;
}

// ---- 1. transform ---------------------------------------------------------------------------------------------------------------
// One workgroup = 32 consecutive scan-order blocks of ONE image (grid.y = image), 8 lanes per block.  Lane r builds ROW r of its
// block's samples straight from the pixels (edge padding is a clamp of the coordinates: see the rules below), runs the row pass, the
// block is transposed through LDS (rows padded to 9 words), lane r runs the column pass on COLUMN r and quantises, the coefficients
// go to their zig-zag positions in LDS and leave as one 16-byte store per lane.
//
// Edges (jcprepct.c / jcsample.c): luma replicates its last row and column.  Chroma of 4:2:0: to the right the last FULL-RESOLUTION
// column is replicated and then downsampled (the bias keeps alternating with the output column); at the bottom the last
// full-resolution row is replicated only to complete a row pair (odd h), below that the last DOWNSAMPLED row is replicated.  Both
// are pure functions of the output coordinate.
//
// Dummy blocks (jccoefct.c compress_data; only luma of 4:2:0 has them, where ceil(w / 8) or ceil(h / 8) is odd): AC zero, DC = the DC
// of the previous block in MCU order, which always resolves to a real block of the same MCU.  The lanes of a dummy block compute
// that source block again instead of waiting for it, so blocks need no order.
template <int DT>
__global__ __launch_bounds__(256) void jpeg_enc_transform_kernel(const void* __restrict__ src, long long sn, long long sc, long long sy,
                                                                 long long sx, const JpegEncDesc* __restrict__ desc,
                                                                 const uint16_t* __restrict__ qtab, int16_t* __restrict__ coef,
                                                                 uint32_t* __restrict__ raw, long long raw_stride_words, int blocks_max,
                                                                 int Hmax, int Wmax, long long cap_max, int s420, int vec) {
    __shared__ int s[kXformBlocks][8][9];
    __shared__ __attribute__((aligned(16))) int16_t sout[kXformBlocks][64];
    __shared__ uint16_t sq[128];
    const int tile = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    const Geo g = make_geo(desc[n], Hmax, Wmax, cap_max, s420 != 0);
    const int ntiles = (g.nblocks + kXformBlocks - 1) / kXformBlocks;
    if (tile >= ntiles) return;
    {   // zero this tile's share of the image's raw bit-stream slot (pack ORs into it)
        const long long words = ((long long)g.cap + 3) >> 2;
        const long long lo = words * tile / ntiles, hi = words * (tile + 1) / ntiles;
        uint32_t* slot = raw + (long long)n * raw_stride_words;
        for (long long i = lo + tid; i < hi; i += 256) slot[i] = 0u;
    }
    if (tid < 128) sq[tid] = qtab[tid];
    const int b = tile * kXformBlocks + lb;
    const bool valid = b < g.nblocks;
    int comp = 0, bx = 0, by = 0;
    bool dummy = false;
    if (valid) {
        const int mcu = b / g.bpm, k = b - mcu * g.bpm, mcy = mcu / g.mx, mcx = mcu - mcy * g.mx;
        if (s420) {
            if (k < 4) {
                const bool r1 = 2 * mcx + 1 >= g.bw_y, b1 = 2 * mcy + 1 >= g.bh_y;     // the MCU's right column / bottom row is dummy
                int ks = k;
                if (k == 1 && r1) { dummy = true; ks = 0; }
                if (k == 2 && b1) { dummy = true; ks = r1 ? 0 : 1; }
                if (k == 3 && (r1 || b1)) { dummy = true; ks = b1 ? (r1 ? 0 : 1) : 2; }
                bx = 2 * mcx + (ks & 1);
                by = 2 * mcy + (ks >> 1);
            } else {
                comp = k - 3;
                bx = mcx;
                by = mcy;
            }
        } else {
            comp = k;
            bx = mcx;
            by = mcy;
        }
    }
    int d[8], o[8];
    if (valid) {
        const long long base = (long long)n * sn;
        int R[8], G[8], B[8];
        if (comp == 0 || !s420) {
            fetch8<DT>(src, base + (long long)min(by * 8 + r, g.h - 1) * sy, bx * 8, g.w, sc, sx, vec != 0, R, G, B);
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = ycc(R[j], G[j], B[j], comp) - 128;
        } else {
            const int cy = min(by * 8 + r, ((g.h + 1) >> 1) - 1);
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = (j & 1) ? 2 : 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {                              // two rows x two runs of 8 full-resolution pixels
                const int yy = (q & 2) ? min(2 * cy + 1, g.h - 1) : 2 * cy;
                fetch8<DT>(src, base + (long long)yy * sy, bx * 16 + (q & 1) * 8, g.w, sc, sx, vec != 0, R, G, B);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    d[(q & 1) * 4 + j] += ycc(R[2 * j], G[2 * j], B[2 * j], comp) + ycc(R[2 * j + 1], G[2 * j + 1], B[2 * j + 1], comp);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = (d[j] >> 2) - 128;
        }
        fdct_pass<true>(d, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[lb][r][j] = o[j];
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = s[lb][i][r];
        fdct_pass<false>(d, o);
        const uint16_t* q = sq + (comp ? 64 : 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int nat = i * 8 + r, div = 8 * (int)q[nat], x = o[i];
            const int m = ((x < 0 ? -x : x) + (div >> 1)) / div;
            sout[lb][kInvZigZag.pos[nat]] = (int16_t)((dummy && nat) ? 0 : (x < 0 ? -m : m));
        }
    }
    __syncthreads();
    if (valid)
        *(uint4*)(coef + ((long long)n * blocks_max + b) * 64 + r * 8) = *(const uint4*)&sout[lb][r * 8];
}

// ---- Huffman coding of one block ------------------------------------------------------------------------------------------------------
struct BitWriter {             // MSB-first bit stream ORed into zeroed 32-bit words (stored big-endian); neighbours share edge words
    uint32_t* words;
    unsigned widx, nwords;
    unsigned long long acc;    // the low `nacc` bits are pending
    int nacc;
    __device__ __forceinline__ void start(uint32_t* w, unsigned nw, unsigned bitpos) {
        words = w; nwords = nw; widx = bitpos >> 5; nacc = (int)(bitpos & 31u); acc = 0ull;      // the leading bits are a neighbour's: OR zeros
    }
    __device__ __forceinline__ void word(uint32_t v) {
        if (widx < nwords && v) atomicOr(words + widx, __builtin_bswap32(v));
        ++widx;
    }
    __device__ __forceinline__ void put(uint32_t code, int n) {      // n <= 26
        acc = (acc << n) | code;
        nacc += n;
        if (nacc >= 32) {
            nacc -= 32;
            word((uint32_t)(acc >> nacc));
            acc &= (1ull << nacc) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (nacc > 0) word((uint32_t)(acc << (32 - nacc)));
    }
};

// block index of the previous block of the same component in scan order, negative in the first MCU
__device__ __forceinline__ int pred_block(int b, int k, bool s420) {
    if (!s420) return b - 3;
    return k == 0 ? b - 3 : (k < 4 ? b - 1 : b - 6);
}

// jchuff.c encode_one_block on 64 zig-zag coefficients held in registers (fully unrolled: every index is static).  Returns the bit
// count; EMIT also writes the bits.
template <bool EMIT>
__device__ __forceinline__ unsigned encode_block(const uint4* __restrict__ cp, int pred, const uint32_t* dc, const uint32_t* ac, BitWriter& bw) {
    uint32_t wd[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = cp[i];
        wd[4 * i] = v.x; wd[4 * i + 1] = v.y; wd[4 * i + 2] = v.z; wd[4 * i + 3] = v.w;
    }
    unsigned total = 0;
    {
        const int diff = (int)(short)(wd[0] & 0xffffu) - pred;
        const int n = 32 - __clz(diff < 0 ? -diff : diff);
        const uint32_t e = dc[n];
        total += (e >> 16) + n;
        if (EMIT) bw.put(((e & 0xffffu) << n) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u)), (int)(e >> 16) + n);
    }
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = (int)(short)((k & 1) ? (wd[k >> 1] >> 16) : (wd[k >> 1] & 0xffffu));
        if (v == 0) {
            ++run;
        } else {
            while (run > 15) {
                const uint32_t z = ac[0xF0];
                total += z >> 16;
                if (EMIT) bw.put(z & 0xffffu, (int)(z >> 16));
                run -= 16;
            }
            const int n = 32 - __clz(v < 0 ? -v : v);
            const uint32_t e = ac[((run << 4) | n) & 255];
            total += (e >> 16) + n;
            if (EMIT) bw.put(((e & 0xffffu) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), (int)(e >> 16) + n);
            run = 0;
        }
    }
    if (run > 0) {
        const uint32_t e = ac[0];
        total += e >> 16;
        if (EMIT) bw.put(e & 0xffffu, (int)(e >> 16));
    }
    return total;
}

__device__ __forceinline__ void load_enc_tabs(uint32_t (*sdc)[16], uint32_t (*sac)[256], int tid) {
    for (int i = tid; i < 512; i += 256) sac[i >> 8][i & 255] = kEncTab[2 + (i >> 8)].e[i & 255];
    if (tid < 32) sdc[tid >> 4][tid & 15] = kEncTab[tid >> 4].e[tid & 15];
}

// ---- 2. size --------------------------------------------------------------------------------------------------------------------
template <bool EMIT>
__global__ __launch_bounds__(256) void jpeg_enc_entropy_kernel(const int16_t* __restrict__ coef, const JpegEncDesc* __restrict__ desc,
                                                               uint32_t* __restrict__ blk_off, uint32_t* __restrict__ tile_sum,
                                                               uint32_t* __restrict__ img_info, uint32_t* __restrict__ raw,
                                                               long long raw_stride_words, int blocks_max, int tiles_max, int Hmax,
                                                               int Wmax, long long cap_max, int s420) {
    __shared__ uint32_t sdc[2][16];
    __shared__ uint32_t sac[2][256];
    __shared__ unsigned sscan[256];
    const int tile = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const Geo g = make_geo(desc[n], Hmax, Wmax, cap_max, s420 != 0);
    const int ntiles = (g.nblocks + kTileBlocks - 1) / kTileBlocks;
    if (tile >= ntiles) return;
    unsigned long long base = 0ull, total = 0ull;
    if (EMIT) {
        // ---- 3. pack: the bit offset of this tile and the image's total from the tile totals (a uniform loop: scalar loads) ----
        for (int t = 0; t < ntiles; ++t) {
            const unsigned v = tile_sum[(long long)n * tiles_max + t];
            total += v;
            if (t < tile) base += v;
        }
        const bool over = total > 8ull * g.cap;
        if (tile == 0 && tid == 0) {
            img_info[2 * n] = over ? 0u : (uint32_t)total;
            img_info[2 * n + 1] = over ? 1u : 0u;
        }
        if (over) return;              // never truncated: the caller encodes this image elsewhere
    }
    load_enc_tabs(sdc, sac, tid);
    __syncthreads();
    const int b = tile * kTileBlocks + tid;
    unsigned bits = 0;
    if (b < g.nblocks) {
        const int k = b % g.bpm, comp = s420 ? (k < 4 ? 0 : k - 3) : k, t = comp ? 1 : 0;
        const int16_t* blocks = coef + (long long)n * blocks_max * 64;
        const int pb = pred_block(b, k, s420 != 0);
        const int pred = pb >= 0 ? (int)blocks[(long long)pb * 64] : 0;
        BitWriter bw;
        if (EMIT) bw.start(raw + (long long)n * raw_stride_words, (g.cap + 3u) >> 2, (unsigned)(base + blk_off[(long long)n * blocks_max + b]));
        bits = encode_block<EMIT>((const uint4*)(blocks + (long long)b * 64), pred, sdc[t], sac[t], bw);
        if (EMIT) {
            if (b == g.nblocks - 1) {                                  // fill the final byte with ones
                const int p = (int)((8u - (unsigned)(total & 7ull)) & 7u);
                bw.put((1u << p) - 1u, p);
            }
            bw.finish();
        }
    }
    if (!EMIT) {
        const unsigned incl = block_scan_inclusive(bits, sscan, tid);
        if (b < g.nblocks) blk_off[(long long)n * blocks_max + b] = incl - bits;
        if (tid == 255) tile_sum[(long long)n * tiles_max + tile] = incl;
    }
}

// ---- 4. count -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned count_ff(const uint4 v, long long first, long long nbytes) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    unsigned c = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) c += (first + i < nbytes && ((w[i >> 2] >> (8 * (i & 3))) & 255u) == 255u) ? 1u : 0u;
    return c;
}

__global__ __launch_bounds__(256) void jpeg_enc_count_kernel(const uint32_t* __restrict__ raw, long long raw_stride_words,
                                                             const uint32_t* __restrict__ img_info, uint32_t* __restrict__ ff_cnt,
                                                             int chunks_max) {
    __shared__ unsigned ssum;
    const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    if (img_info[2 * n + 1]) return;
    const long long nbytes = ((long long)img_info[2 * n] + 7) >> 3;
    if ((long long)c * kChunkBytes >= nbytes) return;
    if (tid == 0) ssum = 0u;
    __syncthreads();
    const uint4 v = *(const uint4*)(raw + (long long)n * raw_stride_words + (long long)c * (kChunkBytes / 4) + tid * 4);
    const unsigned cnt = count_ff(v, (long long)c * kChunkBytes + tid * 16, nbytes);
    if (cnt) atomicAdd(&ssum, cnt);
    __syncthreads();
    if (tid == 0) ff_cnt[(long long)n * chunks_max + c] = ssum;
}

// ---- 5. stuff and frame -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_enc_frame_kernel(const uint32_t* __restrict__ raw, long long raw_stride_words,
                                                             const uint32_t* __restrict__ img_info, const uint32_t* __restrict__ ff_cnt,
                                                             int chunks_max, const JpegEncDesc* __restrict__ desc,
                                                             const uint8_t* __restrict__ hdr, int hdr_stride, uint8_t* __restrict__ out,
                                                             long long out_stride, int* __restrict__ result, long long cap_max) {
    __shared__ unsigned sscan[256];
    const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    if (img_info[2 * n + 1]) {                                         // the raw stream alone was over the capacity
        if (c == 0 && tid == 0) { result[2 * n] = 0; result[2 * n + 1] = 1; }
        return;
    }
    const long long nbytes = ((long long)img_info[2 * n] + 7) >> 3;
    if (c > 0 && (long long)c * kChunkBytes >= nbytes) return;
    const int nchunks = (int)((nbytes + kChunkBytes - 1) / kChunkBytes);
    long long ff_before = 0, ff_total = 0;
    for (int t = 0; t < nchunks; ++t) {                                // uniform: scalar loads
        const unsigned v = ff_cnt[(long long)n * chunks_max + t];
        ff_total += v;
        if (t < c) ff_before += v;
    }
    const long long cap = min((long long)max(desc[n].capacity, 0), cap_max);
    if (nbytes + ff_total > cap) {
        if (c == 0 && tid == 0) { result[2 * n] = 0; result[2 * n + 1] = 1; }
        return;
    }
    uint8_t* o = out + (long long)n * out_stride;
    if (c == 0) {
        for (int i = tid; i < kHeaderBytes; i += 256) o[i] = hdr[(long long)n * hdr_stride + i];
        if (tid == 0) {
            o[kHeaderBytes + nbytes + ff_total] = 0xFF;
            o[kHeaderBytes + nbytes + ff_total + 1] = 0xD9;
            result[2 * n] = (int)(kHeaderBytes + nbytes + ff_total + 2);
            result[2 * n + 1] = 0;
        }
    }
    const long long first = (long long)c * kChunkBytes + tid * 16;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (first < nbytes) v = *(const uint4*)(raw + (long long)n * raw_stride_words + (long long)c * (kChunkBytes / 4) + tid * 4);
    const unsigned cnt = count_ff(v, first, nbytes);
    const unsigned incl = block_scan_inclusive(cnt, sscan, tid);
    if (first < nbytes) {
        uint8_t* p = o + kHeaderBytes + first + ff_before + (incl - cnt);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (first + i < nbytes) {
                const uint8_t byte = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
                *p++ = byte;
                if (byte == 0xFF) *p++ = 0;
            }
        }
    }
}

// ---- host: tables and header ------------------------------------------------------------------------------------------------------
void scaled_qtables(int quality, uint16_t* out128) {                 // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            long v = ((long)(t ? kQChroma[i] : kQLuma[i]) * scale + 50) / 100;
            out128[t * 64 + i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

struct Layout {
    long long blocks_max, tiles_max, chunks_max, raw_stride, out_stride;
    size_t off_coef, off_blk, off_tile, off_info, off_raw, off_ff, total;
};
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
bool make_layout(int N, int Hmax, int Wmax, int subsampling, long long cap_max, Layout& L) {
    if (N <= 0 || Hmax <= 0 || Wmax <= 0 || Hmax > 65535 || Wmax > 65535 || cap_max <= 0 || cap_max >= (1ll << 28)) return false;
    if (subsampling != WU_JPEG_ENC_420 && subsampling != WU_JPEG_ENC_444) return false;
    const int m = subsampling == WU_JPEG_ENC_420 ? 16 : 8;
    L.blocks_max = (long long)((Wmax + m - 1) / m) * ((Hmax + m - 1) / m) * (subsampling == WU_JPEG_ENC_420 ? 6 : 3);
    if (L.blocks_max >= (1ll << 26) || L.blocks_max * N >= (1ll << 31)) return false;
    L.tiles_max = (L.blocks_max + kTileBlocks - 1) / kTileBlocks;
    L.raw_stride = (cap_max + kChunkBytes - 1) / kChunkBytes * kChunkBytes;
    L.chunks_max = L.raw_stride / kChunkBytes;
    L.out_stride = (long long)align256((size_t)(kHeaderBytes + cap_max + 2));
    size_t at = 0;
    L.off_coef = at; at = align256(at + (size_t)N * L.blocks_max * 128);
    L.off_blk = at;  at = align256(at + (size_t)N * L.blocks_max * 4);
    L.off_tile = at; at = align256(at + (size_t)N * L.tiles_max * 4);
    L.off_info = at; at = align256(at + (size_t)N * 8);
    L.off_raw = at;  at = align256(at + (size_t)N * L.raw_stride);
    L.off_ff = at;   at = align256(at + (size_t)N * L.chunks_max * 4);
    L.total = at;
    return true;
}

}  // namespace

extern "C" size_t wu_jpeg_enc_desc_bytes(void) { return sizeof(JpegEncDesc); }
extern "C" size_t wu_jpeg_enc_header_bytes(void) { return kHeaderBytes; }

extern "C" int wu_jpeg_enc_qtables(int quality, uint16_t* out128) {
    WU_REQUIRE(out128, "jpeg_enc_qtables: null argument");
    WU_REQUIRE(quality >= 1 && quality <= 100, "jpeg_enc_qtables: quality %d outside 1..100", quality);
    scaled_qtables(quality, out128);
    return 0;
}

extern "C" int wu_jpeg_enc_header(int h, int w, int quality, int subsampling, uint8_t* out, size_t capacity) {
    WU_REQUIRE(out, "jpeg_enc_header: null argument");
    WU_REQUIRE(h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "jpeg_enc_header: bad size %d x %d (JPEG holds 1..65535)", h, w);
    WU_REQUIRE(quality >= 1 && quality <= 100, "jpeg_enc_header: quality %d outside 1..100", quality);
    WU_REQUIRE(subsampling == WU_JPEG_ENC_420 || subsampling == WU_JPEG_ENC_444, "jpeg_enc_header: subsampling %d is neither 4:2:0 nor 4:4:4", subsampling);
    WU_REQUIRE(capacity >= (size_t)kHeaderBytes, "jpeg_enc_header: buffer of %zu bytes, the header takes %d", capacity, kHeaderBytes);
    uint16_t q[128];
    scaled_qtables(quality, q);
    uint8_t* p = out;
    auto put = [&](int v) { *p++ = (uint8_t)v; };
    auto marker = [&](int m, int body) { put(0xFF); put(m); put((body + 2) >> 8); put((body + 2) & 255); };
    put(0xFF); put(0xD8);
    marker(0xE0, 14);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);      // "JFIF\0" 1.01, no units, 1:1, no thumbnail
    for (int t = 0; t < 2; ++t) {
        marker(0xDB, 65);
        put(t);
        for (int i = 0; i < 64; ++i) put(q[t * 64 + kZigZag[i]]);
    }
    marker(0xC0, 15);
    for (int v : {8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, subsampling == WU_JPEG_ENC_420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
    const struct { int id; const uint8_t* bits; const uint8_t* vals; int n; } tabs[4] = {
        {0x00, kDcLumaBits, kDcVals, 12}, {0x10, kAcLumaBits, kAcLumaVals, 162}, {0x01, kDcChromaBits, kDcVals, 12}, {0x11, kAcChromaBits, kAcChromaVals, 162}};
    for (const auto& t : tabs) {
        marker(0xC4, 17 + t.n);
        put(t.id);
        for (int i = 0; i < 16; ++i) put(t.bits[i]);
        for (int i = 0; i < t.n; ++i) put(t.vals[i]);
    }
    marker(0xDA, 10);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
    return (int)(p - out);
}

extern "C" size_t wu_jpeg_enc_workspace_bytes(int N, int Hmax, int Wmax, int subsampling, long long cap_max) {
    Layout L;
    return make_layout(N, Hmax, Wmax, subsampling, cap_max, L) ? L.total : 0;
}

extern "C" size_t wu_jpeg_enc_out_stride(long long cap_max) {
    return cap_max > 0 && cap_max < (1ll << 28) ? align256((size_t)(kHeaderBytes + cap_max + 2)) : 0;
}

extern "C" int wu_jpeg_enc_workspace_layout(int N, int Hmax, int Wmax, int subsampling, long long cap_max, long long* out8) {
    Layout L;
    WU_REQUIRE(out8, "jpeg_enc_workspace_layout: null argument");
    WU_REQUIRE(make_layout(N, Hmax, Wmax, subsampling, cap_max, L), "jpeg_enc_workspace_layout: bad shape N=%d Hmax=%d Wmax=%d subsampling=%d capacity=%lld",
               N, Hmax, Wmax, subsampling, cap_max);
    const long long v[8] = {(long long)L.off_coef, (long long)L.off_blk, (long long)L.off_tile, (long long)L.off_info,
                            (long long)L.off_raw,  (long long)L.off_ff,  L.blocks_max,          L.raw_stride};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return 0;
}

extern "C" int wu_jpeg_enc_encode(const void* src, int dtype, long long sn, long long sc, long long sy, long long sx, const void* desc_dev,
                                  const uint16_t* qtab_dev, const uint8_t* hdr_dev, int hdr_stride, void* workspace, size_t workspace_bytes,
                                  uint8_t* out, size_t out_bytes, int* result_dev, int N, int Hmax, int Wmax, int subsampling,
                                  long long cap_max, void* stream) {
    WU_REQUIRE(src && desc_dev && qtab_dev && hdr_dev && workspace && out && result_dev, "jpeg_enc_encode: null argument");
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16 || dtype == WU_JPEG_ENC_U8, "jpeg_enc_encode: dtype %d is not u8 / f32 / bf16", dtype);
    Layout L;
    WU_REQUIRE(make_layout(N, Hmax, Wmax, subsampling, cap_max, L), "jpeg_enc_encode: bad shape N=%d Hmax=%d Wmax=%d subsampling=%d capacity=%lld",
               N, Hmax, Wmax, subsampling, cap_max);
    WU_REQUIRE(N <= 65535, "jpeg_enc_encode: N=%d over 65535 images per batch", N);
    WU_REQUIRE(hdr_stride >= kHeaderBytes, "jpeg_enc_encode: header stride %d under %d", hdr_stride, kHeaderBytes);
    WU_REQUIRE(workspace_bytes >= L.total, "jpeg_enc_encode: workspace too small (%zu of %zu bytes)", workspace_bytes, L.total);
    WU_REQUIRE(out_bytes >= (size_t)N * L.out_stride, "jpeg_enc_encode: output too small (%zu of %zu bytes)", out_bytes, (size_t)((size_t)N * L.out_stride));
    WU_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)desc_dev & 3) == 0 && ((uintptr_t)qtab_dev & 1) == 0 && ((uintptr_t)result_dev & 3) == 0,
               "jpeg_enc_encode: workspace must be 256-byte aligned, descriptors / tables / results naturally aligned");
    const int esz = dtype == WU_F32 ? 4 : (dtype == WU_BF16 ? 2 : 1);
    WU_REQUIRE(((uintptr_t)src & (esz - 1)) == 0, "jpeg_enc_encode: source pointer not aligned to its element size");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    int16_t* coef = (int16_t*)(ws + L.off_coef);
    uint32_t* blk_off = (uint32_t*)(ws + L.off_blk);
    uint32_t* tile_sum = (uint32_t*)(ws + L.off_tile);
    uint32_t* info = (uint32_t*)(ws + L.off_info);
    uint32_t* raw = (uint32_t*)(ws + L.off_raw);
    uint32_t* ff = (uint32_t*)(ws + L.off_ff);
    const JpegEncDesc* desc = (const JpegEncDesc*)desc_dev;
    const int s420 = subsampling == WU_JPEG_ENC_420;
    const long long rsw = L.raw_stride / 4;
    // wide loads: fp32 planes with unit pixel stride and 16-byte aligned rows, or interleaved uint8 with 4-byte aligned rows
    const int vec = dtype == WU_F32 ? (sx == 1 && ((sn | sc | sy) & 3) == 0 && ((uintptr_t)src & 15) == 0)
                                    : (dtype == WU_JPEG_ENC_U8 && sc == 1 && sx == 3 && ((sn | sy) & 3) == 0 && ((uintptr_t)src & 3) == 0);
    const dim3 gx((unsigned)((L.blocks_max + kXformBlocks - 1) / kXformBlocks), N), gt((unsigned)L.tiles_max, N), gc((unsigned)L.chunks_max, N);
#define WU_ENC_XFORM(DT) \
    hipLaunchKernelGGL(jpeg_enc_transform_kernel<DT>, gx, dim3(256), 0, s, src, sn, sc, sy, sx, desc, qtab_dev, coef, raw, rsw, (int)L.blocks_max, Hmax, Wmax, cap_max, s420, vec)
    if (dtype == WU_JPEG_ENC_U8) WU_ENC_XFORM(WU_JPEG_ENC_U8);
    else if (dtype == WU_F32) WU_ENC_XFORM(WU_F32);
    else WU_ENC_XFORM(WU_BF16);
#undef WU_ENC_XFORM
    WU_LAUNCH_CHECK("jpeg_enc_transform_kernel");
    hipLaunchKernelGGL(jpeg_enc_entropy_kernel<false>, gt, dim3(256), 0, s, coef, desc, blk_off, tile_sum, info, raw, rsw, (int)L.blocks_max,
                       (int)L.tiles_max, Hmax, Wmax, cap_max, s420);
    WU_LAUNCH_CHECK("jpeg_enc_entropy_kernel<size>");
    hipLaunchKernelGGL(jpeg_enc_entropy_kernel<true>, gt, dim3(256), 0, s, coef, desc, blk_off, tile_sum, info, raw, rsw, (int)L.blocks_max,
                       (int)L.tiles_max, Hmax, Wmax, cap_max, s420);
    WU_LAUNCH_CHECK("jpeg_enc_entropy_kernel<pack>");
    hipLaunchKernelGGL(jpeg_enc_count_kernel, gc, dim3(256), 0, s, raw, rsw, info, ff, (int)L.chunks_max);
    WU_LAUNCH_CHECK("jpeg_enc_count_kernel");
    hipLaunchKernelGGL(jpeg_enc_frame_kernel, gc, dim3(256), 0, s, raw, rsw, info, ff, (int)L.chunks_max, desc, hdr_dev, hdr_stride, out,
                       L.out_stride, result_dev, cap_max);
    WU_LAUNCH_CHECK("jpeg_enc_frame_kernel");
    return 0;
}
