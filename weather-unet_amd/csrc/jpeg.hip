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
#include "wu_common.h"

namespace {

const uint8_t kZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- the overflow bound -------------------------------------------------------------------------------------------------------
// Every temporary of one 1-D pass of jidctint is a linear function of the pass's 8 inputs.  Running the pass on the 8 unit vectors
// gives, per input, the largest |weight| any temporary carries: 25172 (input 3: tmp2 * FIX_3_072711026), and the largest |weight|
// of a pass OUTPUT before its shift: 11363.  With A = sum |c*q| over a block (so every column's and row's L1 norm is <= A):
//   pass 1 temporaries <= 25172 * A;            pass 1 outputs <= 11363 * A / 2^11 + 1 <= 5.549 A + 1
//   pass 2 inputs of a row: L1 <= 5.549 A + 8;  pass 2 temporaries <= 25172 * (5.549 A + 8) + 2^17
// 32-bit temporaries hold for A < 15372.  libjpeg-turbo's SIMD IDCT (the code Pillow actually runs) additionally keeps the pass 1
// outputs and the dequantised inputs in SIGNED 16-BIT lanes, so equality with it needs 5.549 A + 1 <= 32767, A <= 5904.
// The bound below is the tighter one, rounded down.  For scale: the DCT of 8-bit samples has L2 norm <= 1024 per block, a block of
// N(0, 25) noise on top of a full-range gradient has A around 2500; only synthetic full-swing noise gets near the bound, and such
// an image is reported unsupported (the caller decodes it with Pillow), never decoded approximately.
constexpr int kMaxBlockL1 = 5900;

struct HuffTab {
    uint8_t look_nbits[512];   // 9-bit look-ahead: code length (0 = longer than 9 bits) and symbol
    uint8_t look_sym[512];
    int maxcode[18];           // largest code of each length (-1 if none); [17] = sentinel
    int valoffset[17];
    const uint8_t* vals;
    int nvals;
};

bool build_huff(const uint8_t* counts, HuffTab& t) {
    t.vals = counts + 16;
    memset(t.look_nbits, 0, sizeof(t.look_nbits));
    memset(t.look_sym, 0, sizeof(t.look_sym));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        t.valoffset[l] = k - code;
        if (code + c > (1 << l)) return false;                      // more codes than the code space of this length holds
        if (l <= 9)
            for (int i = 0; i < c; ++i) {
                const int first = (code + i) << (9 - l);
                for (int j = 0; j < (1 << (9 - l)); ++j) {
                    t.look_nbits[first + j] = (uint8_t)l;
                    t.look_sym[first + j] = t.vals[k + i];
                }
            }
        k += c;
        code += c;
        t.maxcode[l] = c ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.nvals = k;
    return k <= 256;
}

struct BitReader {             // 64-bit buffer, MSB first; stops in front of any marker and feeds zero bits from there on
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int n;                     // bits in acc
    int fake;                  // of those, zero bits made up after a marker / the end of the data (always the lowest ones)
    inline void fill() {
        while (n <= 56) {
            unsigned b = 0;
            if (p < end && *p != 0xFF) {
                b = *p++;
            } else if (p + 1 < end && p[1] == 0x00) {              // stuffed 0xFF
                b = 0xFF;
                p += 2;
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    inline void skip(int k) { n -= k; }
    inline bool overrun() const { return n < fake; }
};

inline int decode_symbol(BitReader& br, const HuffTab& t) {     // needs >= 16 bits in the buffer; -1 on a code no table entry matches
    const unsigned look = br.peek(9);
    int l = t.look_nbits[look];
    if (l) {
        br.skip(l);
        return t.look_sym[look];
    }
    l = 10;
    int code = (int)br.peek(10);
    while (code > t.maxcode[l]) {
        ++l;
        if (l > 16) return -1;
        code = (int)br.peek(l);
    }
    br.skip(l);
    const int idx = code + t.valoffset[l];
    if (idx < 0 || idx >= t.nvals) return -1;
    return t.vals[idx];
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

}  // namespace

// ---- host: markers ------------------------------------------------------------------------------------------------------------
extern "C" int wu_jpeg_parse(const uint8_t* d, size_t n, wu_jpeg_info* info) {
    WU_REQUIRE(d && info, "jpeg_parse: null argument");
    memset(info, 0, sizeof(*info));
#define WU_JPEG_UNSUP(r)      \
    do {                      \
        info->supported = 0;  \
        info->reason = (r);   \
        return 0;             \
    } while (0)
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) WU_JPEG_UNSUP(WU_JPEG_NOT_JPEG);
    if (n > 0x7fffffffu) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
    size_t pos = 2;
    bool jfif = false, have_sof = false;
    int adobe = -1, comp_id[3] = {0, 0, 0};
    bool dqt16[4] = {false, false, false, false};
    for (;;) {
        if (pos + 4 > n || d[pos] != 0xFF) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
        while (d[pos + 1] == 0xFF) {                               // fill bytes in front of a marker
            ++pos;
            if (pos + 4 > n) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
        }
        const int m = d[pos + 1];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) {               // stand-alone markers
            pos += 2;
            continue;
        }
        if (m == 0xD9 || m == 0x00) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
        const size_t L = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (L < 2 || pos + 2 + L > n) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
        const uint8_t* seg = d + pos + 4;
        const size_t sl = L - 2;
        if (m == 0xDB) {                                           // DQT
            size_t k = 0;
            while (k < sl) {
                const int pq = seg[k] >> 4, tq = seg[k] & 15;
                if (tq > 3 || pq > 1 || k + 1 + (pq ? 128 : 64) > sl) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
                dqt16[tq] = pq == 1;
                info->dqt_off[tq] = (int)(pos + 4 + k + 1);
                k += 1 + (pq ? 128 : 64);
            }
        } else if (m == 0xC4) {                                    // DHT
            size_t k = 0;
            while (k < sl) {
                if (k + 17 > sl) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
                const int tc = seg[k] >> 4, th = seg[k] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += seg[k + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || k + 17 + cnt > sl) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
                info->dht_off[tc * 4 + th] = (int)(pos + 4 + k + 1);
                k += 17 + cnt;
            }
        } else if (m == 0xC0 || m == 0xC1) {                       // SOF0 / SOF1: sequential Huffman
            if (have_sof || sl < 6) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            if (seg[0] != 8) WU_JPEG_UNSUP(WU_JPEG_PRECISION);
            info->height = (seg[1] << 8) | seg[2];
            info->width = (seg[3] << 8) | seg[4];
            info->ncomp = seg[5];
            if (info->height == 0 || info->width == 0 || info->ncomp == 0 || sl != (size_t)(6 + 3 * info->ncomp)) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            if (info->ncomp != 1 && info->ncomp != 3) WU_JPEG_UNSUP(WU_JPEG_COLORSPACE);     // CMYK / YCCK / two components
            for (int c = 0; c < info->ncomp; ++c) {
                comp_id[c] = seg[6 + 3 * c];
                info->hs[c] = seg[7 + 3 * c] >> 4;
                info->vs[c] = seg[7 + 3 * c] & 15;
                info->tq[c] = seg[8 + 3 * c];
                if (info->hs[c] < 1 || info->hs[c] > 4 || info->vs[c] < 1 || info->vs[c] > 4 || info->tq[c] > 3) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            }
            have_sof = true;
        } else if (m == 0xC2) {
            WU_JPEG_UNSUP(WU_JPEG_PROGRESSIVE);
        } else if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF || m == 0xCC) {
            WU_JPEG_UNSUP(WU_JPEG_ARITHMETIC);
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) {
            WU_JPEG_UNSUP(WU_JPEG_LOSSLESS);                       // lossless / hierarchical frames
        } else if (m == 0xDD) {                                    // DRI
            if (sl < 2) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            info->restart_interval = (seg[0] << 8) | seg[1];
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
        } else if (m == 0xDA) {                                    // SOS
            if (!have_sof || sl < 1) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            const int ns = seg[0];
            if (ns < 1 || ns > 4 || sl != (size_t)(4 + 2 * ns)) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            if (ns != info->ncomp) WU_JPEG_UNSUP(WU_JPEG_MULTISCAN);
            for (int c = 0; c < ns; ++c) {
                if (seg[1 + 2 * c] != comp_id[c]) WU_JPEG_UNSUP(WU_JPEG_MULTISCAN);          // components out of frame order
                info->td[c] = seg[2 + 2 * c] >> 4;
                info->ta[c] = seg[2 + 2 * c] & 15;
                if (info->td[c] > 3 || info->ta[c] > 3 || !info->dht_off[info->td[c]] || !info->dht_off[4 + info->ta[c]] ||
                    !info->dqt_off[info->tq[c]])
                    WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
                if (dqt16[info->tq[c]]) WU_JPEG_UNSUP(WU_JPEG_QTABLE16);
            }
            if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) WU_JPEG_UNSUP(WU_JPEG_CORRUPT);
            info->scan_offset = (int)(pos + 2 + L);
            break;
        }
        pos += 2 + L;
    }
    // colour space as libjpeg's default_decompress_parms reads it; only grey and YCbCr are decoded here
    if (info->ncomp == 3) {
        bool ycc;
        if (jfif) ycc = true;
        else if (adobe >= 0) ycc = adobe == 1;
        else ycc = comp_id[0] == 1 && comp_id[1] == 2 && comp_id[2] == 3;
        if (!ycc) WU_JPEG_UNSUP(WU_JPEG_COLORSPACE);
        if (info->hs[1] != 1 || info->vs[1] != 1 || info->hs[2] != 1 || info->vs[2] != 1) WU_JPEG_UNSUP(WU_JPEG_SAMPLING);
        if (info->hs[0] == 1 && info->vs[0] == 1) info->mode = WU_JPEG_MODE_444;
        else if (info->hs[0] == 2 && info->vs[0] == 1) info->mode = WU_JPEG_MODE_H2V1;
        else if (info->hs[0] == 2 && info->vs[0] == 2) info->mode = WU_JPEG_MODE_H2V2;
        else WU_JPEG_UNSUP(WU_JPEG_SAMPLING);
    } else {
        if (info->hs[0] != 1 || info->vs[0] != 1) WU_JPEG_UNSUP(WU_JPEG_SAMPLING);
        info->mode = WU_JPEG_MODE_GREY;
    }
    const int hmax = info->hs[0], vmax = info->vs[0];
    info->mcus_x = (info->width + 8 * hmax - 1) / (8 * hmax);
    info->mcus_y = (info->height + 8 * vmax - 1) / (8 * vmax);
    info->total_blocks = 0;
    for (int c = 0; c < info->ncomp; ++c) {
        info->blocks_w[c] = info->mcus_x * info->hs[c];
        info->blocks_h[c] = info->mcus_y * info->vs[c];
        info->total_blocks += info->blocks_w[c] * info->blocks_h[c];     // <= 3 * 8192^2: fits
    }
    info->coef_bytes = (long long)info->total_blocks * 128;
    info->supported = 1;
    info->reason = WU_JPEG_OK;
    return 0;
#undef WU_JPEG_UNSUP
}

// ---- host: Huffman decoding of the one interleaved scan --------------------------------------------------------------------------
extern "C" int wu_jpeg_entropy_decode(const uint8_t* d, size_t n, wu_jpeg_info* info, int16_t* coef, size_t coef_capacity,
                                      uint16_t* qtab_out) {
    WU_REQUIRE(d && info && coef && qtab_out, "jpeg_entropy_decode: null argument");
    WU_REQUIRE(info->supported == 1 && info->ncomp >= 1 && info->ncomp <= 3, "jpeg_entropy_decode: the file was not parsed as supported");
    // the struct came from wu_jpeg_parse on the SAME bytes; re-check everything that indexes memory all the same
    long long blocks = 0;
    int plane_off[3] = {0, 0, 0};
    for (int c = 0; c < info->ncomp; ++c) {
        WU_REQUIRE(info->hs[c] >= 1 && info->hs[c] <= 2 && info->vs[c] >= 1 && info->vs[c] <= 2 && info->mcus_x > 0 && info->mcus_y > 0 &&
                       info->mcus_x <= 8192 && info->mcus_y <= 8192 && info->blocks_w[c] == info->mcus_x * info->hs[c] &&
                       info->blocks_h[c] == info->mcus_y * info->vs[c],
                   "jpeg_entropy_decode: inconsistent geometry");
        WU_REQUIRE(info->td[c] >= 0 && info->td[c] <= 3 && info->ta[c] >= 0 && info->ta[c] <= 3 && info->tq[c] >= 0 && info->tq[c] <= 3,
                   "jpeg_entropy_decode: bad table id");
        plane_off[c] = (int)blocks;
        blocks += (long long)info->blocks_w[c] * info->blocks_h[c];
    }
    WU_REQUIRE(blocks == info->total_blocks && (unsigned long long)blocks * 128ull <= coef_capacity,
               "jpeg_entropy_decode: coefficient buffer too small (%lld blocks, %zu bytes)", blocks, coef_capacity);
    WU_REQUIRE(info->scan_offset > 0 && (size_t)info->scan_offset <= n, "jpeg_entropy_decode: scan offset outside the data");

    HuffTab dc[3], ac[3];
    uint16_t qzz[3][64];
    for (int c = 0; c < info->ncomp; ++c) {
        const int od = info->dht_off[info->td[c]], oa = info->dht_off[4 + info->ta[c]], oq = info->dqt_off[info->tq[c]];
        WU_REQUIRE(od > 0 && (size_t)od + 16 <= n && oa > 0 && (size_t)oa + 16 <= n && oq > 0 && (size_t)oq + 64 <= n,
                   "jpeg_entropy_decode: table offset outside the data");
        if (!build_huff(d + od, dc[c]) || !build_huff(d + oa, ac[c]) || (size_t)od + 16 + dc[c].nvals > n || (size_t)oa + 16 + ac[c].nvals > n)
            WU_FAIL(-2, "jpeg: corrupt Huffman table");
        for (int k = 0; k < 64; ++k) {
            qzz[c][k] = d[oq + k];
            qtab_out[c * 64 + kZigZag[k]] = d[oq + k];
        }
    }
    for (int c = info->ncomp; c < 3; ++c)
        for (int k = 0; k < 64; ++k) qtab_out[c * 64 + k] = 1;
    memset(coef, 0, (size_t)blocks * 128);

    BitReader br{d + info->scan_offset, d + n, 0, 0, 0};
    int pred[3] = {0, 0, 0};
    int max_l1 = 0, next_rst = 0;
    long long mcu = 0;
    const int ri = info->restart_interval;
    for (int my = 0; my < info->mcus_y; ++my) {
        for (int mx = 0; mx < info->mcus_x; ++mx, ++mcu) {
            if (ri && mcu && mcu % ri == 0) {
                // the reader never steps over a marker, so after the interval's last block it stands right in front of RSTn
                if (br.p + 1 >= br.end || br.p[0] != 0xFF || br.p[1] != 0xD0 + next_rst)
                    WU_FAIL(-3, "jpeg: bad restart marker sequence at MCU %lld", mcu);
                br.p += 2;
                br.acc = 0;
                br.n = 0;
                br.fake = 0;
                next_rst = (next_rst + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < info->ncomp; ++c) {
                const HuffTab& tdc = dc[c];
                const HuffTab& tac = ac[c];
                const uint16_t* q = qzz[c];
                for (int v = 0; v < info->vs[c]; ++v) {
                    for (int h = 0; h < info->hs[c]; ++h) {
                        int16_t* blk = coef + ((size_t)plane_off[c] + (size_t)(my * info->vs[c] + v) * info->blocks_w[c] + mx * info->hs[c] + h) * 64;
                        br.fill();
                        int s = decode_symbol(br, tdc);
                        if (s < 0 || s > 15) WU_FAIL(-4, "jpeg: bad Huffman code (DC) at MCU %lld", mcu);
                        if (s) {
                            const int bits = (int)br.peek(s);
                            br.skip(s);
                            pred[c] += extend(bits, s);
                        }
                        if (pred[c] < -32768 || pred[c] > 32767) WU_FAIL(-5, "jpeg: DC coefficient out of range at MCU %lld", mcu);
                        blk[0] = (int16_t)pred[c];
                        int l1 = (pred[c] < 0 ? -pred[c] : pred[c]) * q[0];
                        for (int k = 1; k < 64; ++k) {
                            if (br.n < 32) br.fill();
                            const int rs = decode_symbol(br, tac);
                            if (rs < 0) WU_FAIL(-4, "jpeg: bad Huffman code (AC) at MCU %lld", mcu);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;                 // end of block
                                k += 15;
                                continue;
                            }
                            k += r;
                            if (k > 63) WU_FAIL(-6, "jpeg: coefficient index past 63 at MCU %lld", mcu);
                            const int val = extend((int)br.peek(s), s);
                            br.skip(s);
                            blk[kZigZag[k]] = (int16_t)val;
                            l1 += (val < 0 ? -val : val) * q[k];
                            if (l1 > (1 << 28)) l1 = 1 << 28;       // saturate: a corrupt stream must not wrap the sum
                        }
                        if (br.overrun()) WU_FAIL(-7, "jpeg: premature marker or end of data at MCU %lld", mcu);
                        if (l1 > max_l1) max_l1 = l1;
                    }
                }
            }
        }
    }
    info->max_block_l1 = max_l1;
    if (max_l1 > kMaxBlockL1) {
        snprintf(g_wu_err, sizeof(g_wu_err), "jpeg: a block's sum |c*q| = %d exceeds %d (16-bit IDCT lanes would saturate)", max_l1, kMaxBlockL1);
        info->reason = WU_JPEG_MAGNITUDE;
        return 1;
    }
    return 0;
}

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
    const int dw = d.mode == WU_JPEG_MODE_444 ? d.w : (d.w + 1) >> 1;
    const int dh = d.mode == WU_JPEG_MODE_H2V2 ? (d.h + 1) >> 1 : d.h;
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

extern "C" size_t wu_jpeg_info_bytes(void) { return sizeof(wu_jpeg_info); }
extern "C" size_t wu_jpeg_desc_bytes(void) { return sizeof(JpegDesc); }
extern "C" int wu_jpeg_max_block_l1(void) { return kMaxBlockL1; }

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
