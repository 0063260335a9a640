// The HOST half of the JPEG decoder (csrc/jpeg.hip includes this file; the C ABI is declared in include/wu_kernels.h): marker parsing
// and Huffman decoding -- the part of JPEG that is sequential by construction -- as plain re-entrant C++: no global mutable state, no
// allocation, no HIP.  Any C++17 compiler can build it, so a stand-alone program may include it directly and run it under host
// sanitizers (scratch/jpeg_prog_asan.cpp); whoever includes it owns g_wu_err.
//
// Output of the entropy stage: quantised int16 coefficients, one 64-entry block after the other in NATURAL (row-major) order,
// component planes one after the other (MCU-padded), blocks of a plane in raster order; plus the quantisation tables.
//
// Two frame kinds end in that same buffer:
//   * sequential (SOF0 / SOF1), ONE interleaved scan: one pass over the MCUs;
//   * progressive (SOF2, opt-in: WU_JPEG_ALLOW_PROGRESSIVE): every scan from the first SOS to EOI is run into the zeroed buffer by one
//     of the four procedures of ITU T.81 G.1.2 / G.2 (DC first, DC refinement, AC first, AC refinement) as libjpeg's jdphuff.c states
//     them.  Refinement scans read bits according to the coefficient history, so this does not parallelise.
#ifndef WU_JPEG_HOST_H
#define WU_JPEG_HOST_H
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/wu_kernels.h"

#ifndef WU_FAIL
extern thread_local char g_wu_err[256];
#define WU_FAIL(code, ...)                                   \
    do {                                                     \
        snprintf(g_wu_err, sizeof(g_wu_err), __VA_ARGS__);   \
        return (code);                                       \
    } while (0)
#define WU_REQUIRE(cond, ...) \
    do {                      \
        if (!(cond)) WU_FAIL(-1, __VA_ARGS__); \
    } while (0)
#endif

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

// ---- markers ------------------------------------------------------------------------------------------------------------------
extern "C" int wu_jpeg_parse_ex(const uint8_t* d, size_t n, wu_jpeg_info* info, int flags) {
    WU_REQUIRE(d && info, "jpeg_parse: null argument");
    WU_REQUIRE((flags & ~(WU_JPEG_ALLOW_PROGRESSIVE | WU_JPEG_ALLOW_H1V2)) == 0, "jpeg_parse: unknown flag bits 0x%x", flags);
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
    bool jfif = false, have_sof = false, progressive = false;
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
        } else if (m == 0xC2 && !(flags & WU_JPEG_ALLOW_PROGRESSIVE)) {
            WU_JPEG_UNSUP(WU_JPEG_PROGRESSIVE);
        } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {          // SOF0 / SOF1: sequential Huffman; SOF2: progressive Huffman
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
            progressive = m == 0xC2;
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
            if (progressive) {
                // The first of several scans: which components it names, its tables and its spectral band are the entropy stage's to
                // check, scan by scan.  Only what no scan can mend is settled here: a 16-bit table a component would latch.
                for (int c = 0; c < info->ncomp; ++c)
                    if (info->dqt_off[info->tq[c]] && dqt16[info->tq[c]]) WU_JPEG_UNSUP(WU_JPEG_QTABLE16);
                info->scan_offset = (int)(pos + 2 + L);
                break;
            }
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
        else if (info->hs[0] == 1 && info->vs[0] == 2 && (flags & WU_JPEG_ALLOW_H1V2)) info->mode = WU_JPEG_MODE_H1V2;   // 4:4:0
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
    info->reserved = progressive ? WU_JPEG_FRAME_PROGRESSIVE : WU_JPEG_FRAME_SEQUENTIAL;
    info->supported = 1;
    info->reason = WU_JPEG_OK;
    return 0;
#undef WU_JPEG_UNSUP
}

extern "C" int wu_jpeg_parse(const uint8_t* d, size_t n, wu_jpeg_info* info) { return wu_jpeg_parse_ex(d, n, info, 0); }

// ---- progressive frames: every scan into one coefficient buffer -------------------------------------------------------------------
namespace {

inline int prog_bit(BitReader& br) {
    if (br.n < 32) br.fill();
    const int b = (int)br.peek(1);
    br.skip(1);
    return b;
}

// One block of each procedure (jdphuff.c decode_mcu_DC_first / _DC_refine / _AC_first / _AC_refine).  0, or the negative code of
// wu_jpeg_entropy_decode; the caller words the message.  `eobrun` = blocks still covered by the running end-of-band run.
inline int prog_dc_first(BitReader& br, const HuffTab& t, int16_t* blk, int& pred, int al) {
    br.fill();
    const int s = decode_symbol(br, t);
    if (s < 0 || s > 15) return -4;
    if (s) {
        const int bits = (int)br.peek(s);
        br.skip(s);
        pred += extend(bits, s);
    }
    if (pred < -32768 || pred > 32767) return -5;
    const int v = pred * (1 << al);                                // the point transform: the scan carries the value >> al
    if (v < -32768 || v > 32767) return -5;
    blk[0] = (int16_t)v;
    return 0;
}

inline int prog_ac_first(BitReader& br, const HuffTab& t, int16_t* blk, int ss, int se, int al, int& eobrun) {
    if (eobrun > 0) {                                              // this block is all zero in the band
        --eobrun;
        return 0;
    }
    for (int k = ss; k <= se; ++k) {
        if (br.n < 32) br.fill();
        const int rs = decode_symbol(br, t);
        if (rs < 0) return -4;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            k += r;
            if (k > se) return -6;
            const int val = extend((int)br.peek(s), s) * (1 << al);
            br.skip(s);
            if (val < -32768 || val > 32767) return -5;
            blk[kZigZag[k]] = (int16_t)val;
        } else if (r == 15) {
            k += 15;                                               // ZRL: 16 zeros
        } else {                                                   // EOBr: this block and 2^r + bits - 1 more end here
            eobrun = 1 << r;
            if (r) {
                if (br.n < 32) br.fill();
                eobrun += (int)br.peek(r);
                br.skip(r);
            }
            --eobrun;
            break;
        }
    }
    return 0;
}

// A correction bit follows every coefficient that is ALREADY non-zero and is passed on the way -- inside a zero run, behind the last
// new coefficient, during an end-of-band run; it is applied only where bit `al` is not set yet, and away from zero.  Zero runs (ZRL's
// 16 included) count zero-HISTORY coefficients only.  A new coefficient is +-(1 << al).
inline void prog_correct(BitReader& br, int16_t& c, int p1) {
    if (prog_bit(br) && (c & p1) == 0) c = (int16_t)(c >= 0 ? c + p1 : c - p1);
}

inline int prog_ac_refine(BitReader& br, const HuffTab& t, int16_t* blk, int ss, int se, int al, int& eobrun) {
    const int p1 = 1 << al;
    int k = ss;
    if (eobrun == 0) {
        for (; k <= se; ++k) {
            if (br.n < 32) br.fill();
            const int rs = decode_symbol(br, t);
            if (rs < 0) return -4;
            int r = rs >> 4, s = rs & 15;
            if (s) {
                if (s != 1) return -4;                             // a new coefficient has magnitude 1 at this precision
                s = prog_bit(br) ? p1 : -p1;
            } else if (r != 15) {
                eobrun = 1 << r;
                if (r) {
                    if (br.n < 32) br.fill();
                    eobrun += (int)br.peek(r);
                    br.skip(r);
                }
                break;                                             // the rest of this block is handled as the run's first block
            }
            do {
                int16_t& c = blk[kZigZag[k]];
                if (c != 0) {
                    prog_correct(br, c, p1);
                } else if (--r < 0) {
                    break;                                         // the zero the run ends on: the new coefficient's place
                }
                ++k;
            } while (k <= se);
            if (s) {
                if (k > se) return -6;                             // the run left the band
                blk[kZigZag[k]] = (int16_t)s;
            }
        }
    }
    if (eobrun > 0) {
        for (; k <= se; ++k) {
            int16_t& c = blk[kZigZag[k]];
            if (c != 0) prog_correct(br, c, p1);
        }
        --eobrun;
    }
    return 0;
}

// Returns like wu_jpeg_entropy_decode.  `info` passed its geometry checks; nothing else of it is trusted: the frame header is read
// again and must agree, and the tables come from the marker walk, not from info->dht_off / dqt_off (DHT and DRI, and DQT too, may be
// redefined between scans).
int jpeg_prog_decode(const uint8_t* d, size_t n, wu_jpeg_info* info, int16_t* coef, const int* plane_off, long long blocks,
                     uint16_t* qtab_out) {
    static_assert(sizeof(HuffTab) * 8 < 32768, "the Huffman tables live on the caller's stack");
    HuffTab dc[4], ac[4];
    bool dc_ok[4] = {false, false, false, false}, ac_ok[4] = {false, false, false, false};
    int dqt_at[4] = {0, 0, 0, 0}, latched[3] = {0, 0, 0}, comp_id[3] = {0, 0, 0}, cw[3] = {0, 0, 0}, ch[3] = {0, 0, 0};
    bool dqt16[4] = {false, false, false, false}, have_sof = false;
    int8_t al_of[3][64];                                           // precision delivered so far per coefficient: -1 = none, else the last Al
    memset(al_of, -1, sizeof(al_of));
    int ri = 0;
    const int hmax = info->hs[0], vmax = info->vs[0];
    for (int c = 0; c < info->ncomp; ++c) {
        // the component's own block grid (what a scan of this component ALONE walks): ceil(comp_w / 8) x ceil(comp_h / 8) with
        // comp_w = ceil(width * hs / hmax).  The stored plane is MCU-padded, so its rows may be longer and more than the grid's.
        cw[c] = ((info->width * info->hs[c] + hmax - 1) / hmax + 7) / 8;
        ch[c] = ((info->height * info->vs[c] + vmax - 1) / vmax + 7) / 8;
        WU_REQUIRE(info->hs[c] <= hmax && info->vs[c] <= vmax && cw[c] >= 1 && ch[c] >= 1 && cw[c] <= info->blocks_w[c] && ch[c] <= info->blocks_h[c],
                   "jpeg_entropy_decode: inconsistent geometry");
    }
    memset(coef, 0, (size_t)blocks * 128);

#define WU_JPEG_REFUSE(r)   \
    do {                    \
        info->reason = (r); \
        return 1;           \
    } while (0)
    size_t pos = 2;
    for (;;) {
        if (pos + 2 > n || d[pos] != 0xFF) WU_FAIL(-7, "jpeg: premature end of data or no marker at byte %zu", pos);
        while (d[pos + 1] == 0xFF) {                               // fill bytes in front of a marker
            ++pos;
            if (pos + 2 > n) WU_FAIL(-7, "jpeg: premature end of data at byte %zu", pos);
        }
        const int m = d[pos + 1];
        if (m == 0xD9) break;                                      // EOI
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {               // stand-alone markers
            pos += 2;
            continue;
        }
        if (m == 0xD8 || m == 0x00) WU_FAIL(-7, "jpeg: unexpected marker 0x%02x at byte %zu", m, pos);
        if (pos + 4 > n) WU_FAIL(-7, "jpeg: premature end of data at byte %zu", pos);
        const size_t L = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (L < 2 || pos + 2 + L > n) WU_FAIL(-7, "jpeg: marker segment at byte %zu leaves the data", pos);
        const uint8_t* seg = d + pos + 4;
        const size_t sl = L - 2;
        if (m == 0xDB) {                                           // DQT: in force from here on (see the latch rule at SOS)
            size_t k = 0;
            while (k < sl) {
                const int pq = seg[k] >> 4, tq = seg[k] & 15;
                if (tq > 3 || pq > 1 || k + 1 + (pq ? 128 : 64) > sl) WU_FAIL(-2, "jpeg: corrupt quantisation table segment at byte %zu", pos);
                dqt16[tq] = pq == 1;
                dqt_at[tq] = (int)(pos + 4 + k + 1);
                k += 1 + (pq ? 128 : 64);
            }
        } else if (m == 0xC4) {                                    // DHT: replaces the table of its class and id from here on
            size_t k = 0;
            while (k < sl) {
                if (k + 17 > sl) WU_FAIL(-2, "jpeg: corrupt Huffman table segment at byte %zu", pos);
                const int tc = seg[k] >> 4, th = seg[k] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += seg[k + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || k + 17 + cnt > sl) WU_FAIL(-2, "jpeg: corrupt Huffman table segment at byte %zu", pos);
                (tc ? ac_ok : dc_ok)[th] = build_huff(seg + k + 1, (tc ? ac : dc)[th]);       // a bad table is an error where a scan uses it
                k += 17 + cnt;
            }
        } else if (m == 0xDD) {                                    // DRI
            if (sl < 2) WU_FAIL(-7, "jpeg: short DRI segment at byte %zu", pos);
            ri = (seg[0] << 8) | seg[1];
        } else if (m == 0xC2) {                                    // the frame header wu_jpeg_parse_ex read: it must be this one
            bool same = !have_sof && sl == (size_t)(6 + 3 * info->ncomp) && seg[0] == 8 && ((seg[1] << 8) | seg[2]) == info->height &&
                        ((seg[3] << 8) | seg[4]) == info->width && seg[5] == info->ncomp;
            for (int c = 0; same && c < info->ncomp; ++c) {
                comp_id[c] = seg[6 + 3 * c];
                same = (seg[7 + 3 * c] >> 4) == info->hs[c] && (seg[7 + 3 * c] & 15) == info->vs[c] && seg[8 + 3 * c] == info->tq[c];
            }
            if (!same) WU_FAIL(-1, "jpeg_entropy_decode: the frame header does not match the parsed one");
            have_sof = true;
        } else if ((m >= 0xC0 && m <= 0xCF) || m == 0xDC || m == 0xDE || m == 0xDF) {      // another frame, DAC, DNL, hierarchical
            WU_FAIL(-7, "jpeg: unexpected marker 0x%02x at byte %zu", m, pos);
        } else if (m == 0xDA) {                                    // SOS: one scan
            if (!have_sof || sl < 1) WU_FAIL(-7, "jpeg: scan without a frame header at byte %zu", pos);
            const int ns = seg[0];
            if (ns < 1 || ns > 4 || sl != (size_t)(4 + 2 * ns) || ns > info->ncomp) WU_FAIL(-7, "jpeg: bad scan header at byte %zu", pos);
            int sc[3] = {0, 0, 0}, std_[3] = {0, 0, 0}, sta[3] = {0, 0, 0};
            for (int i = 0; i < ns; ++i) {
                int c = 0;
                while (c < info->ncomp && comp_id[c] != seg[1 + 2 * i]) ++c;
                if (c == info->ncomp) WU_FAIL(-7, "jpeg: scan names an unknown component at byte %zu", pos);
                sc[i] = c;
                std_[i] = seg[2 + 2 * i] >> 4;
                sta[i] = seg[2 + 2 * i] & 15;
                if (std_[i] > 3 || sta[i] > 3) WU_FAIL(-7, "jpeg: bad table id in the scan header at byte %zu", pos);
                // a component twice, or components out of frame order: nothing a writer produces -- left to the other decoder
                if (i > 0 && c <= sc[i - 1]) WU_JPEG_REFUSE(WU_JPEG_PROGRESSIVE_INCOMPLETE);
            }
            const int ss = seg[1 + 2 * ns], se = seg[2 + 2 * ns], ah = seg[3 + 2 * ns] >> 4, al = seg[3 + 2 * ns] & 15;
            // jdphuff.c start_pass_phuff_decoder: Ss <= Se <= 63; Ss = 0 implies Se = 0 (DC and AC never share a scan); an AC scan names
            // exactly one component; a refinement lowers Al by exactly one; Al <= 13.  Anything else is an error there and here.
            const bool dc_band = ss == 0;
            if ((dc_band ? se != 0 : (ss > se || se > 63 || ns != 1)) || (ah != 0 && al != ah - 1) || al > 13)
                WU_FAIL(-7, "jpeg: bad progressive scan parameters Ss=%d Se=%d Ah=%d Al=%d at byte %zu", ss, se, ah, al, pos);
            for (int i = 0; i < ns; ++i) {
                const int c = sc[i];
                // The legal Ah / Al sequence per coefficient: the first scan of a coefficient has Ah = 0, every later one has Ah = the
                // Al delivered before; an AC scan needs the component's DC first.  libjpeg only WARNS about a script that breaks this
                // and decodes on; what it then computes is not worth restating -- the file goes to the other decoder.
                if (!dc_band && al_of[c][0] < 0) WU_JPEG_REFUSE(WU_JPEG_PROGRESSIVE_INCOMPLETE);
                for (int k = ss; k <= se; ++k) {
                    if (ah != (al_of[c][k] < 0 ? 0 : al_of[c][k])) WU_JPEG_REFUSE(WU_JPEG_PROGRESSIVE_INCOMPLETE);
                    al_of[c][k] = (int8_t)al;
                }
                // The latch rule (libjpeg jdinput.c latch_quant_tables): a component uses the quantisation table in force when ITS
                // first scan starts; a DQT that redefines the slot later does not reach back.
                if (!latched[c]) {
                    const int tq = info->tq[c];
                    if (!dqt_at[tq]) WU_FAIL(-2, "jpeg: no quantisation table %d at the first scan of component %d", tq, c);
                    if (dqt16[tq]) WU_JPEG_REFUSE(WU_JPEG_QTABLE16);
                    latched[c] = dqt_at[tq];
                }
                if (dc_band ? (ah == 0 && !dc_ok[std_[i]]) : !ac_ok[sta[i]])
                    WU_FAIL(-2, "jpeg: corrupt or missing Huffman table for the scan at byte %zu", pos);
            }

            BitReader br{d + pos + 2 + L, d + n, 0, 0, 0};
            int pred[3] = {0, 0, 0}, eobrun = 0, next_rst = 0;
            // A scan of ONE component walks that component's own grid, block by block (a restart interval then counts blocks); a scan
            // of several walks the frame's MCUs.
            const bool single = ns == 1;
            const int c0 = sc[0];
            const int ux_n = single ? cw[c0] : info->mcus_x, uy_n = single ? ch[c0] : info->mcus_y;
            long long unit = 0;
            for (int uy = 0; uy < uy_n; ++uy) {
                for (int ux = 0; ux < ux_n; ++ux, ++unit) {
                    if (ri && unit && unit % ri == 0) {
                        // the reader never steps over a marker, so after the interval's last block it stands right in front of RSTn
                        if (br.p + 1 >= br.end || br.p[0] != 0xFF || br.p[1] != 0xD0 + next_rst)
                            WU_FAIL(-3, "jpeg: bad restart marker sequence at unit %lld of the scan at byte %zu", unit, pos);
                        br.p += 2;
                        br.acc = 0;
                        br.n = 0;
                        br.fake = 0;
                        next_rst = (next_rst + 1) & 7;
                        pred[0] = pred[1] = pred[2] = 0;
                        eobrun = 0;                                // an end-of-band run never crosses a restart marker (but it does cross rows)
                    }
                    int rc = 0;
                    if (single) {
                        int16_t* blk = coef + ((size_t)plane_off[c0] + (size_t)uy * info->blocks_w[c0] + ux) * 64;
                        if (!dc_band) rc = ah == 0 ? prog_ac_first(br, ac[sta[0]], blk, ss, se, al, eobrun) : prog_ac_refine(br, ac[sta[0]], blk, ss, se, al, eobrun);
                        else if (ah == 0) rc = prog_dc_first(br, dc[std_[0]], blk, pred[0], al);
                        else if (prog_bit(br)) blk[0] = (int16_t)(blk[0] | (1 << al));
                    } else {
                        for (int i = 0; i < ns && rc == 0; ++i) {
                            const int c = sc[i];
                            for (int v = 0; v < info->vs[c] && rc == 0; ++v)
                                for (int h = 0; h < info->hs[c] && rc == 0; ++h) {
                                    int16_t* blk = coef + ((size_t)plane_off[c] + (size_t)(uy * info->vs[c] + v) * info->blocks_w[c] + ux * info->hs[c] + h) * 64;
                                    if (ah == 0) rc = prog_dc_first(br, dc[std_[i]], blk, pred[i], al);
                                    else if (prog_bit(br)) blk[0] = (int16_t)(blk[0] | (1 << al));
                                }
                        }
                    }
                    if (rc == -4) WU_FAIL(-4, "jpeg: bad Huffman code at unit %lld of the scan at byte %zu", unit, pos);
                    if (rc == -5) WU_FAIL(-5, "jpeg: coefficient out of range at unit %lld of the scan at byte %zu", unit, pos);
                    if (rc == -6) WU_FAIL(-6, "jpeg: coefficient index past the band at unit %lld of the scan at byte %zu", unit, pos);
                    if (br.overrun()) WU_FAIL(-7, "jpeg: premature marker or end of data at unit %lld of the scan at byte %zu", unit, pos);
                }
            }
            // more blocks promised than the scan holds: libjpeg does not notice; the blocks are what they are either way
            pos = (size_t)(br.p - d);                              // in front of the next marker (or of bytes no marker claims: an error above)
            continue;
        }
        pos += 2 + L;
    }

    // Completeness.  A file whose scans do not bring every coefficient of every component down to Al = 0 is decoded by libjpeg WITH
    // inter-block smoothing (jdcoefct.c smoothing_ok), which the reconstruction kernels do not do: such a file is refused here.
    for (int c = 0; c < info->ncomp; ++c)
        for (int k = 0; k < 64; ++k)
            if (al_of[c][k] != 0) WU_JPEG_REFUSE(WU_JPEG_PROGRESSIVE_INCOMPLETE);
#undef WU_JPEG_REFUSE

    int max_l1 = 0;
    for (int c = 0; c < 3; ++c) {
        uint16_t* q = qtab_out + c * 64;
        if (c >= info->ncomp) {
            for (int k = 0; k < 64; ++k) q[k] = 1;
            continue;
        }
        for (int k = 0; k < 64; ++k) q[kZigZag[k]] = d[latched[c] + k];                      // latched[c] + 64 <= n: checked where it was read
        const int16_t* blk = coef + (size_t)plane_off[c] * 64;
        const long long nb = (long long)info->blocks_w[c] * info->blocks_h[c];
        for (long long b = 0; b < nb; ++b, blk += 64) {
            int l1 = 0;
            for (int k = 0; k < 64; ++k) l1 += (blk[k] < 0 ? -blk[k] : blk[k]) * q[k];       // <= 64 * 32768 * 255: fits
            if (l1 > (1 << 28)) l1 = 1 << 28;
            if (l1 > max_l1) max_l1 = l1;
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

}  // namespace

// ---- Huffman decoding: the one interleaved scan of a sequential frame, or every scan of a progressive one -----------------------------
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
    if (info->reserved == WU_JPEG_FRAME_PROGRESSIVE) {
        WU_REQUIRE(info->width > 0 && info->height > 0 && info->width <= 65535 && info->height <= 65535 &&
                       info->mcus_x == (info->width + 8 * info->hs[0] - 1) / (8 * info->hs[0]) &&
                       info->mcus_y == (info->height + 8 * info->vs[0] - 1) / (8 * info->vs[0]) && n >= 4,
                   "jpeg_entropy_decode: inconsistent geometry");
        return jpeg_prog_decode(d, n, info, coef, plane_off, blocks, qtab_out);
    }
    WU_REQUIRE(info->reserved == WU_JPEG_FRAME_SEQUENTIAL, "jpeg_entropy_decode: unknown frame kind %d", info->reserved);

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

extern "C" size_t wu_jpeg_info_bytes(void) { return sizeof(wu_jpeg_info); }
extern "C" int wu_jpeg_max_block_l1(void) { return kMaxBlockL1; }

#endif  // WU_JPEG_HOST_H
