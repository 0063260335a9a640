// Huffman decoding of baseline JPEG scans on the device: fills the coefficient buffer of csrc/jpeg.hip (wu_jpeg_reconstruct consumes it)
// bit for bit as wu_jpeg_entropy_decode does, so that the compressed scan and not 2 bytes per sample of zero-filled coefficients goes
// over the link.
//
//   * HOST (plain C++, re-entrant, no allocation, no GPU): wu_jpeg_scan_stage copies the entropy-coded bytes once -- byte stuffing
//     removed, split at the RSTn markers into SEGMENTS that each start on a subsequence boundary -- plus the raw DHT bytes and the
//     quantisation tables.
//   * DEVICE (three launches for a whole batch): zero the images' blocks; the self-synchronising walk (one 256-thread workgroup per
//     image); DC prediction + the magnitude bound.
//
// The walk.  A SUBSEQUENCE is S consecutive bits of a segment.  A decoder state is (bit position, block-in-MCU, zig-zag index k); the
// Huffman tables in use follow from the block-in-MCU.  Started at a wrong place a JPEG decoder falls into step with the true symbol
// sequence after a few dozen symbols (the codes are self-synchronising in practice), and once two decoders agree on the full state at a
// subsequence boundary they agree for ever.  A workgroup walks its image's subsequences in chunks of 256, in order:
//   round 0      thread i decodes subsequence i from (first bit, block 0, k 0) -- exact if the subsequence begins a segment, exact for
//                thread 0 (the previous chunk's exit state is carried), a guess otherwise -- and stores its exit state e[i];
//   round r >= 1 every active thread i decodes subsequence i + r from its own running state and compares the FULL state with e[i + r]:
//                equal -> inactive (the rest of its path is already recorded); otherwise it overwrites e[i + r].  A thread that reaches
//                the end of its segment or of the chunk goes inactive.  No thread active -> done (at most 255 rounds, whatever the data).
// Then every e[] is exact (the last visitor of a subsequence descends from an exact start), thread i re-decodes subsequence i from
// e[i - 1] to count the blocks that begin in it, a prefix sum gives its first block's ordinal in the segment, and a last pass writes the
// coefficients: DC DIFFERENCES into blk[0], AC values into blk[kZigZag[k]].  Only that pass reports errors: speculative decoding is a
// total, memory-safe function of (bits, state) that consumes at least one bit per symbol.
#include "wu_common.h"

#ifndef WU_LDS
#define WU_LDS(type, name) __shared__ type name
#endif

namespace {

const uint8_t kHuffZigZagHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__device__ const uint8_t kHuffZigZag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kHuffThreads = 256;
constexpr int kDhtTable = 272;                 // 16 counts + 256 values
constexpr int kDhtImage = 6 * kDhtTable;       // DC of component 0, 1, 2, AC of component 0, 1, 2
constexpr long long kMaxScanBytes = 1ll << 28; // bit positions stay below 2^31

struct HuffDesc {              // one per image, 16 ints (wu/jpeg.py fills it)
    int scan_off, scan_bytes;  // the image's region of the scan buffer: 16-byte aligned, a multiple of 16 bytes
    int first_seg, nseg, nsub;
    int first_block, nblocks;  // the image's blocks in the coefficient buffer
    int ncomp, hs0, vs0;       // chroma is 1x1 (wu_jpeg_parse accepts nothing else)
    int mcus_x, total_mcus;
    int restart_interval;
    int pad[3];
};

bool valid_subseq_bits(int s) { return s >= 64 && s <= 4096 && (s & 31) == 0; }

// the checks of wu_jpeg_entropy_decode on a struct that came from wu_jpeg_parse
bool info_ok(const wu_jpeg_info* info) {
    if (!info || info->supported != 1 || info->ncomp < 1 || info->ncomp > 3 || info->mcus_x <= 0 || info->mcus_y <= 0 || info->mcus_x > 8192 ||
        info->mcus_y > 8192 || info->restart_interval < 0)
        return false;
    // the device walk knows one interleaved baseline scan with luma 1x1 / 2x1 / 2x2: what wu_jpeg_parse_ex's flags add is not staged
    if (info->reserved != WU_JPEG_FRAME_SEQUENTIAL || info->mode == WU_JPEG_MODE_H1V2) return false;
    long long blocks = 0;
    for (int c = 0; c < info->ncomp; ++c) {
        if (info->hs[c] < 1 || info->hs[c] > 2 || info->vs[c] < 1 || info->vs[c] > 2 || (c > 0 && (info->hs[c] != 1 || info->vs[c] != 1)) ||
            info->blocks_w[c] != info->mcus_x * info->hs[c] || info->blocks_h[c] != info->mcus_y * info->vs[c])
            return false;
        if (info->td[c] < 0 || info->td[c] > 3 || info->ta[c] < 0 || info->ta[c] > 3 || info->tq[c] < 0 || info->tq[c] > 3) return false;
        blocks += (long long)info->blocks_w[c] * info->blocks_h[c];
    }
    return blocks == info->total_blocks && info->scan_offset > 0;
}

// build_huff's verdict (csrc/jpeg.hip) on 16 counts: no length holds more codes than its code space, at most 256 values
int huff_count_values(const uint8_t* counts) {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int c = counts[l - 1];
        if (code + c > (1 << l)) return -1;
        k += c;
        code = (code + c) << 1;
    }
    return k <= 256 ? k : -1;
}

}  // namespace

// ---- host: staging of the scan --------------------------------------------------------------------------------------------------
extern "C" int wu_jpeg_scan_segments(const wu_jpeg_info* info) {
    if (!info_ok(info)) return 0;
    const long long mcus = (long long)info->mcus_x * info->mcus_y, ri = info->restart_interval;
    return (int)(ri > 0 ? (mcus + ri - 1) / ri : 1);
}

extern "C" size_t wu_jpeg_scan_stage_bytes(const wu_jpeg_info* info, size_t nbytes, int subseq_bits) {
    if (!info_ok(info) || !valid_subseq_bits(subseq_bits) || (size_t)info->scan_offset > nbytes || nbytes > 0x7fffffffu) return 0;
    // every segment is padded to a whole number of subsequences (an empty one to one), then 8 zero bytes, then to 16 bytes
    const long long b = (long long)(nbytes - (size_t)info->scan_offset) + (long long)wu_jpeg_scan_segments(info) * (subseq_bits / 8) + 24;
    return b > kMaxScanBytes ? 0 : (size_t)(b & ~15ll);
}

extern "C" int wu_jpeg_scan_stage(const uint8_t* d, size_t n, const wu_jpeg_info* info, int subseq_bits, uint8_t* scan_out, size_t scan_capacity,
                                  int* seg_out, size_t seg_capacity, uint8_t* dht_out, uint16_t* qtab_out, wu_jpeg_scan* result) {
    WU_REQUIRE(d && info && scan_out && seg_out && dht_out && qtab_out && result, "jpeg_scan_stage: null argument");
    WU_REQUIRE(valid_subseq_bits(subseq_bits), "jpeg_scan_stage: subseq_bits %d is not a multiple of 32 in [64, 4096]", subseq_bits);
    WU_REQUIRE(info_ok(info), "jpeg_scan_stage: the file was not parsed as supported, or inconsistent geometry");
    WU_REQUIRE((size_t)info->scan_offset <= n && n <= 0x7fffffffu, "jpeg_scan_stage: scan offset outside the data");
    const size_t bound = wu_jpeg_scan_stage_bytes(info, n, subseq_bits);
    WU_REQUIRE(bound > 0, "jpeg_scan_stage: a scan of more than 2^28 bytes is not staged");
    const int nseg = wu_jpeg_scan_segments(info);
    WU_REQUIRE(scan_capacity >= bound && seg_capacity >= (size_t)nseg * 16,
               "jpeg_scan_stage: capacity too small (scan %zu of %zu bytes, segments %zu of %zu bytes)", scan_capacity, bound, seg_capacity,
               (size_t)nseg * 16);
    memset(result, 0, sizeof(*result));

    memset(dht_out, 0, kDhtImage);
    for (int c = 0; c < info->ncomp; ++c) {
        const int od = info->dht_off[info->td[c]], oa = info->dht_off[4 + info->ta[c]], oq = info->dqt_off[info->tq[c]];
        WU_REQUIRE(od > 0 && (size_t)od + 16 <= n && oa > 0 && (size_t)oa + 16 <= n && oq > 0 && (size_t)oq + 64 <= n,
                   "jpeg_scan_stage: table offset outside the data");
        const int nd = huff_count_values(d + od), na = huff_count_values(d + oa);
        if (nd < 0 || na < 0 || (size_t)od + 16 + nd > n || (size_t)oa + 16 + na > n) WU_FAIL(-2, "jpeg: corrupt Huffman table");
        memcpy(dht_out + c * kDhtTable, d + od, 16 + (size_t)nd);
        memcpy(dht_out + (3 + c) * kDhtTable, d + oa, 16 + (size_t)na);
        for (int k = 0; k < 64; ++k) qtab_out[c * 64 + kHuffZigZagHost[k]] = d[oq + k];
    }
    for (int c = info->ncomp; c < 3; ++c)
        for (int k = 0; k < 64; ++k) qtab_out[c * 64 + k] = 1;

    const size_t sub_bytes = (size_t)subseq_bits / 8;
    const long long mcus = (long long)info->mcus_x * info->mcus_y, ri = info->restart_interval;
    size_t pos = (size_t)info->scan_offset, out = 0;
    int next_rst = 0;
    for (int s = 0; s < nseg; ++s) {
        const size_t seg_start = out;
        for (;;) {                                                 // up to the next marker: runs without 0xFF are copied whole
            const uint8_t* ff = pos < n ? (const uint8_t*)memchr(d + pos, 0xFF, n - pos) : nullptr;
            const size_t run = ff ? (size_t)(ff - d) - pos : n - pos;
            memcpy(scan_out + out, d + pos, run);
            out += run;
            pos += run;
            if (!ff || pos + 1 >= n || d[pos + 1] != 0x00) break;  // the end, a lone last 0xFF, or a marker
            scan_out[out++] = 0xFF;                                // stuffed 0xFF
            pos += 2;
        }
        const size_t len = out - seg_start;
        const size_t nsub = len ? (len + sub_bytes - 1) / sub_bytes : 1;
        memset(scan_out + out, 0, seg_start + nsub * sub_bytes - out);
        out = seg_start + nsub * sub_bytes;
        seg_out[4 * s] = (int)(seg_start / sub_bytes);
        seg_out[4 * s + 1] = (int)(len * 8);
        seg_out[4 * s + 2] = (int)(ri > 0 ? s * ri : 0);
        seg_out[4 * s + 3] = (int)(ri > 0 ? (mcus - s * ri < ri ? mcus - s * ri : ri) : mcus);
        if (s + 1 < nseg) {                                        // the order wu_jpeg_entropy_decode insists on: D0, D1, ... D7, D0
            if (pos + 1 >= n || d[pos] != 0xFF || d[pos + 1] != 0xD0 + next_rst)
                WU_FAIL(-3, "jpeg: bad restart marker sequence at MCU %lld", (long long)(s + 1) * ri);
            pos += 2;
            next_rst = (next_rst + 1) & 7;
        }
    }
    result->n_subseq = (int)(out / sub_bytes);
    const size_t end = (out + 8 + 15) & ~(size_t)15;
    memset(scan_out + out, 0, end - out);
    result->scan_bytes = (int)end;
    result->n_segments = nseg;
    return 0;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
namespace {

struct HuffLds {
    uint8_t look_nbits[6][512];    // 9-bit look-ahead, as HuffTab of csrc/jpeg.hip
    uint8_t look_sym[6][512];
    uint8_t vals[6][256];
    int maxcode[6][18];
    int mincode[6][17];
    int valoffset[6][17];
    int nvals[6];
    uint32_t e_p[kHuffThreads];    // exit states of the chunk's subsequences: bit position, block-in-MCU << 8 | k
    uint32_t e_bk[kHuffThreads];
    int cnt[kHuffThreads];         // blocks begun per subsequence: inclusive, then exclusive prefix sums
    int excl[kHuffThreads];
    int any[2];
    uint32_t carry_p, carry_bk;    // exit state of the previous chunk's last subsequence
    int carry_blocks;              // blocks its segment has begun up to there
    int status;
};

struct HuffState {
    uint32_t p;                    // bit position inside the image's scan region
    int b, k;                      // block-in-MCU; zig-zag index of the next coefficient (0: a DC symbol is next)
};

struct HuffBits {                  // the image's scan region as big-endian words, and this thread's 64-bit window on it
    const uint32_t* w;
    uint32_t nwords;
    uint32_t wi;                   // acc holds words wi and wi + 1 (0xffffffff: nothing yet)
    uint64_t acc;
};

// the 32 bits from bit p on, MSB first; zero past the image's region (aligned loads that never leave it).  Two loads per 32 bits of
// progress, not per symbol.
__device__ __forceinline__ uint32_t huff_peek32(HuffBits& hb, uint32_t p) {
    const uint32_t i = p >> 5, sh = p & 31u;
    if (i != hb.wi) {
        const uint32_t a = i < hb.nwords ? __builtin_bswap32(hb.w[i]) : 0u;
        const uint32_t c = i + 1 < hb.nwords ? __builtin_bswap32(hb.w[i + 1]) : 0u;
        hb.acc = ((uint64_t)a << 32) | c;
        hb.wi = i;
    }
    return (uint32_t)((hb.acc << sh) >> 32);
}

// decode_symbol of csrc/jpeg.hip on a 32-bit window; -1 on a code no table entry matches; len = bits consumed (1 .. 16)
__device__ __forceinline__ int huff_symbol(const HuffLds& s, int t, uint32_t w, int& len) {
    const uint32_t look = w >> 23;
    int l = s.look_nbits[t][look];
    if (l) {
        len = l;
        return s.look_sym[t][look];
    }
    l = 10;
    int code = (int)(w >> 22);
    while (code > s.maxcode[t][l]) {
        ++l;
        if (l > 16) {
            len = 16;
            return -1;
        }
        code = (int)(w >> (32 - l));
    }
    len = l;
    const int idx = code + s.valoffset[t][l];
    if (idx < 0 || idx >= s.nvals[t]) return -1;
    return s.vals[t][idx];
}

__device__ __forceinline__ int huff_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// One symbol with its extra bits: total, deterministic, at least one bit consumed.  Returns the WU_JPEG_HUFF_* bits of what a strict
// decoder would refuse here (a speculative pass ignores them).  out_k: the zig-zag index the value out_v belongs to, -1 = none.
__device__ __forceinline__ int huff_step(const HuffLds& s, HuffBits& hb, HuffState& st, int hv, int bpm, int& out_k, int& out_v) {
    const int comp = st.b < hv ? 0 : 1 + st.b - hv;
    const uint32_t w = huff_peek32(hb, st.p);
    int len, err = 0;
    out_k = -1;
    out_v = 0;
    if (st.k == 0) {
        int sym = huff_symbol(s, comp, w, len);
        if (sym < 0) {
            err = WU_JPEG_HUFF_BAD_CODE;
            sym = 0;
        } else if (sym > 15) {
            err = WU_JPEG_HUFF_DC_CATEGORY;
            sym &= 15;
        }
        if (sym) out_v = huff_extend((int)((w << len) >> (32 - sym)), sym);
        out_k = 0;
        st.p += (uint32_t)(len + sym);
        st.k = 1;
    } else {
        int rs = huff_symbol(s, 3 + comp, w, len);
        if (rs < 0) {
            err = WU_JPEG_HUFF_BAD_CODE;
            rs = 0;                                                // continues as an end of block
        }
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            st.k = r == 15 ? st.k + 16 : 64;
            st.p += (uint32_t)len;
        } else {
            int k = st.k + r;
            if (k > 63) {
                err = WU_JPEG_HUFF_INDEX;
                k = 63;
            } else {
                out_k = k;
                out_v = huff_extend((int)((w << len) >> (32 - sz)), sz);
            }
            st.k = k + 1;
            st.p += (uint32_t)(len + sz);
        }
    }
    if (st.k >= 64) {
        st.k = 0;
        st.b = st.b + 1 == bpm ? 0 : st.b + 1;
    }
    return err;
}

// the symbols that start in front of bit `end`
__device__ __forceinline__ void huff_run(const HuffLds& s, HuffBits& hb, HuffState& st, uint32_t end, int hv, int bpm) {
    int k, v;
    while (st.p < end) huff_step(s, hb, st, hv, bpm, k, v);
}

__global__ __launch_bounds__(256) void jpeg_huff_zero_kernel(const HuffDesc* __restrict__ hdesc, int16_t* __restrict__ coef) {
    const HuffDesc d = hdesc[blockIdx.x];
    uint4* p = reinterpret_cast<uint4*>(coef + (size_t)d.first_block * 64);
    const size_t n16 = (size_t)(d.nblocks > 0 ? d.nblocks : 0) * 8;
    for (size_t i = (size_t)blockIdx.y * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.y * blockDim.x) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(256) void jpeg_huff_walk_kernel(const uint8_t* __restrict__ scan, const int* __restrict__ segs,
                                                             const uint8_t* __restrict__ dht, const HuffDesc* __restrict__ hdesc,
                                                             int16_t* __restrict__ coef, int* __restrict__ status, int S) {
    WU_LDS(HuffLds, s);
    const int img = blockIdx.x, tid = threadIdx.x;
    const HuffDesc d = hdesc[img];
    if (d.nsub <= 0 || d.nseg <= 0) {                              // an image decoded elsewhere
        if (tid == 0) status[img] = 0;
        return;
    }
    // ---- tables: lengths by six threads, values and the look-ahead by all ----
    const uint8_t* tab = dht + (size_t)img * kDhtImage;
    if (tid < 6) {
        const uint8_t* counts = tab + tid * kDhtTable;
        int code = 0, k = 0;
        s.maxcode[tid][0] = -1;
        s.mincode[tid][0] = 0;
        s.valoffset[tid][0] = 0;
        for (int l = 1; l <= 16; ++l) {
            const int c = counts[l - 1];
            s.valoffset[tid][l] = k - code;
            s.mincode[tid][l] = code;
            k += c;
            code += c;
            s.maxcode[tid][l] = c ? code - 1 : -1;
            code <<= 1;
        }
        s.maxcode[tid][17] = 0x7fffffff;
        s.nvals[tid] = k < 256 ? k : 256;
    }
    if (tid == 0) {
        s.status = 0;
        s.carry_p = 0;
        s.carry_bk = 0;
        s.carry_blocks = 0;
    }
    for (int i = tid; i < 6 * 256; i += kHuffThreads) s.vals[i >> 8][i & 255] = tab[(i >> 8) * kDhtTable + 16 + (i & 255)];
    __syncthreads();
    for (int i = tid; i < 6 * 512; i += kHuffThreads) {
        const int t = i >> 9, idx = i & 511;
        int nb = 0, sym = 0;
        for (int l = 1; l <= 9; ++l) {
            const int pre = idx >> (9 - l);
            if (pre >= s.mincode[t][l] && pre <= s.maxcode[t][l]) {
                nb = l;
                sym = s.vals[t][(pre + s.valoffset[t][l]) & 255];
                break;
            }
        }
        s.look_nbits[t][idx] = (uint8_t)nb;
        s.look_sym[t][idx] = (uint8_t)sym;
    }
    __syncthreads();

    HuffBits hb{reinterpret_cast<const uint32_t*>(scan + d.scan_off), (uint32_t)d.scan_bytes >> 2, 0xffffffffu, 0ull};
    const int hv = d.hs0 * d.vs0, bpm = hv + (d.ncomp == 3 ? 2 : 0);
    const int* seg = segs + (size_t)d.first_seg * 4;
    const uint32_t Su = (uint32_t)S;

    for (int c0 = 0; c0 < d.nsub; c0 += kHuffThreads) {
        const int g = c0 + tid;
        const bool valid = g < d.nsub;
        int sj = 0;                                                // the segment of subsequence g: the last one that starts at or before it
        if (valid) {
            int lo = 0, hi = d.nseg - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (seg[4 * mid] <= g) lo = mid;
                else hi = mid - 1;
            }
            sj = lo;
        }
        const int ss = seg[4 * sj], seg_bits = seg[4 * sj + 1], m0 = seg[4 * sj + 2], mc = seg[4 * sj + 3];
        const int se = sj + 1 < d.nseg ? min(seg[4 * (sj + 1)], d.nsub) : d.nsub;     // one past the segment's last subsequence
        const bool exact = valid && (g == ss || tid == 0);
        HuffState entry{(uint32_t)g * Su, 0, 0};
        if (valid && g != ss && tid == 0) entry = HuffState{s.carry_p, (int)(s.carry_bk >> 8), (int)(s.carry_bk & 255u)};
        HuffState st = entry;
        // ---- round 0 ----
        if (valid) {
            huff_run(s, hb, st, (uint32_t)(g + 1) * Su, hv, bpm);
            s.e_p[tid] = st.p;
            s.e_bk[tid] = (uint32_t)(st.b << 8 | st.k);
        }
        // ---- rounds 1 .. 255 ----
        bool active = valid;
        for (int r = 1; r < kHuffThreads; ++r) {
            const int j = tid + r;
            if (active && (j >= kHuffThreads || c0 + j >= se)) active = false;
            if (active) huff_run(s, hb, st, (uint32_t)(c0 + j + 1) * Su, hv, bpm);
            if (tid == 0) s.any[r & 1] = 0;
            __syncthreads();
            bool differs = false;
            if (active) {
                differs = s.e_p[j] != st.p || s.e_bk[j] != (uint32_t)(st.b << 8 | st.k);
                active = differs;
            }
            __syncthreads();
            if (differs) {
                s.e_p[j] = st.p;
                s.e_bk[j] = (uint32_t)(st.b << 8 | st.k);
                atomicOr(&s.any[r & 1], 1);
            }
            __syncthreads();
            if (!s.any[r & 1]) break;
        }
        __syncthreads();
        // ---- exact entry states; count the blocks that begin in each subsequence ----
        if (valid && !exact) entry = HuffState{s.e_p[tid - 1], (int)(s.e_bk[tid - 1] >> 8), (int)(s.e_bk[tid - 1] & 255u)};
        const uint32_t end = (uint32_t)(g + 1) * Su;
        int begun = 0;
        if (valid) {
            HuffState t = entry;
            int k, v;
            while (t.p < end) {
                begun += t.k == 0;
                huff_step(s, hb, t, hv, bpm, k, v);
            }
        }
        s.cnt[tid] = begun;
        for (int off = 1; off < kHuffThreads; off <<= 1) {
            __syncthreads();
            const int add = tid >= off ? s.cnt[tid - off] : 0;
            __syncthreads();
            s.cnt[tid] += add;
        }
        s.excl[tid] = s.cnt[tid] - begun;
        __syncthreads();
        // ordinal, within its segment, of the first block that begins in this subsequence
        int cur = ss >= c0 ? s.excl[tid] - s.excl[ss - c0] : s.carry_blocks + s.excl[tid];
        __syncthreads();
        if (tid == kHuffThreads - 1 && valid) {                    // the carry into the next chunk
            s.carry_p = s.e_p[tid];
            s.carry_bk = s.e_bk[tid];
            s.carry_blocks = cur + begun;
        }
        // ---- write ----
        if (valid) {
            const int total = mc * bpm;                            // blocks of the segment
            const uint32_t seg_end = (uint32_t)ss * Su + (uint32_t)seg_bits;
            HuffState t = entry;
            int16_t* blk = nullptr;
            int err = 0;
            bool in_block = false;                                 // the current symbol belongs to a block inside the segment's count
            if (t.k != 0 && cur >= 1 && cur <= total) {            // in the middle of block cur - 1
                in_block = true;
                const int o = cur - 1, mcu = m0 + o / bpm, bi = o - (o / bpm) * bpm;
                const int my = mcu / d.mcus_x, mx = mcu - my * d.mcus_x;
                int b;
                if (bi < hv) b = (my * d.vs0 + bi / d.hs0) * (d.mcus_x * d.hs0) + mx * d.hs0 + bi % d.hs0;
                else b = d.total_mcus * hv + (bi - hv) * d.total_mcus + mcu;
                if (b >= 0 && b < d.nblocks) blk = coef + ((size_t)d.first_block + (size_t)b) * 64;
            }
            while (t.p < end) {
                if (t.k == 0) {
                    if (cur >= total) {                            // the segment has all its blocks: pad bits and junk are ignored
                        in_block = false;
                        break;
                    }
                    const int o = cur++, mcu = m0 + o / bpm, bi = o - (o / bpm) * bpm;
                    const int my = mcu / d.mcus_x, mx = mcu - my * d.mcus_x;
                    int b;
                    if (bi < hv) b = (my * d.vs0 + bi / d.hs0) * (d.mcus_x * d.hs0) + mx * d.hs0 + bi % d.hs0;
                    else b = d.total_mcus * hv + (bi - hv) * d.total_mcus + mcu;
                    blk = b >= 0 && b < d.nblocks ? coef + ((size_t)d.first_block + (size_t)b) * 64 : nullptr;
                    in_block = true;
                }
                int k, v;
                const int e = huff_step(s, hb, t, hv, bpm, k, v);
                if (in_block) {
                    err |= e;
                    if (t.p > seg_end) err |= WU_JPEG_HUFF_SHORT;  // the symbol used bits the segment does not have
                    else if (k >= 0 && blk) blk[kHuffZigZag[k]] = (int16_t)v;
                    if (t.k == 0 && cur == total && sj + 1 < d.nseg && seg_end - t.p >= 64u && t.p <= seg_end)
                        err |= WU_JPEG_HUFF_SHORT;                 // 8 bytes or more in front of RSTn: the host decoder refuses that too
                }
            }
            if (g == se - 1 && (cur < total || (in_block && t.k != 0))) err |= WU_JPEG_HUFF_SHORT;   // data ended inside the segment's MCUs
            if (err) atomicOr(&s.status, err);
        }
        __syncthreads();
    }
    if (tid == 0) status[img] = s.status;
}

struct DcLds {
    int val[kHuffThreads];
    int flag[kHuffThreads];
    int q[64];
    int carry;
};

// DC differences -> values per (image, component, segment) in scan order, then the magnitude bound.  grid (N, 3).
__global__ __launch_bounds__(256) void jpeg_huff_dc_kernel(const HuffDesc* __restrict__ hdesc, const uint16_t* __restrict__ qtab,
                                                           int16_t* __restrict__ coef, int* __restrict__ status, int max_l1) {
    WU_LDS(DcLds, s);
    const int img = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const HuffDesc d = hdesc[img];
    if (d.nsub <= 0 || c >= d.ncomp) return;
    const int hs = c ? 1 : d.hs0, vs = c ? 1 : d.vs0, nb = hs * vs;
    const int plane = c ? d.total_mcus * d.hs0 * d.vs0 + (c - 1) * d.total_mcus : 0;
    const long long T = (long long)d.total_mcus * nb;
    if (tid < 64) s.q[tid] = qtab[((size_t)img * 3 + c) * 64 + tid];
    if (tid == 0) s.carry = 0;
    int flags = 0;
    for (long long base = 0; base < T; base += kHuffThreads) {
        const long long t = base + tid;
        const bool valid = t < T;
        int16_t* blk = nullptr;
        int v = 0, f = 0;
        if (valid) {
            const int mcu = (int)(t / nb), bi = (int)(t - (long long)mcu * nb);
            const int my = mcu / d.mcus_x, mx = mcu - my * d.mcus_x;
            const int b = plane + (my * vs + bi / hs) * (d.mcus_x * hs) + mx * hs + bi % hs;
            if (b >= 0 && b < d.nblocks) {
                blk = coef + ((size_t)d.first_block + (size_t)b) * 64;
                v = blk[0];
            }
            f = bi == 0 && (d.restart_interval > 0 ? mcu % d.restart_interval == 0 : mcu == 0);
        }
        s.val[tid] = v;
        s.flag[tid] = f;
        for (int off = 1; off < kHuffThreads; off <<= 1) {         // segmented inclusive scan; sums wrap (unsigned) and are exact while
            __syncthreads();                                       // every earlier prefix was inside int16, which is all that is asked
            int av = 0, af = 0;
            const bool take = tid >= off && !s.flag[tid];
            if (tid >= off) {
                av = s.val[tid - off];
                af = s.flag[tid - off];
            }
            __syncthreads();
            if (take) {
                s.val[tid] = (int)((unsigned)s.val[tid] + (unsigned)av);
                s.flag[tid] = af;
            }
        }
        __syncthreads();
        const int dc = s.flag[tid] ? s.val[tid] : (int)((unsigned)s.val[tid] + (unsigned)s.carry);
        __syncthreads();
        if (tid == kHuffThreads - 1) s.carry = dc;
        if (valid && blk) {
            if (dc < -32768 || dc > 32767) flags |= WU_JPEG_HUFF_DC_RANGE;
            blk[0] = (int16_t)dc;
            const int dc16 = (int16_t)dc;                          // 64 * 32768 * 255 < 2^31: the sum cannot wrap
            int l1 = (dc16 < 0 ? -dc16 : dc16) * s.q[0];
            const uint4* row = reinterpret_cast<const uint4*>(blk);
            for (int r = 0; r < 8; ++r) {
                const uint4 cv = row[r];
                const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w};
                for (int j = 0; j < 4; ++j) {
                    const int lo = (int)(short)(cw[j] & 0xffffu), hi = (int)cw[j] >> 16;
                    if (r | j) l1 += (lo < 0 ? -lo : lo) * s.q[r * 8 + 2 * j];
                    l1 += (hi < 0 ? -hi : hi) * s.q[r * 8 + 2 * j + 1];
                }
            }
            if (l1 > max_l1) flags |= WU_JPEG_MAGNITUDE;
        }
        __syncthreads();
    }
    if (flags) atomicOr(&status[img], flags);
}

}  // namespace

extern "C" size_t wu_jpeg_huff_desc_bytes(void) { return sizeof(HuffDesc); }

extern "C" int wu_jpeg_huff_decode(const uint8_t* scan_dev, const int* seg_dev, const uint8_t* dht_dev, const void* hdesc_dev,
                                   const uint16_t* qtab_dev, int16_t* coef_dev, int* status_dev, int N, int subseq_bits, void* stream) {
    WU_REQUIRE(scan_dev && seg_dev && dht_dev && hdesc_dev && qtab_dev && coef_dev && status_dev, "jpeg_huff_decode: null argument");
    WU_REQUIRE(valid_subseq_bits(subseq_bits), "jpeg_huff_decode: subseq_bits %d is not a multiple of 32 in [64, 4096]", subseq_bits);
    WU_REQUIRE(N > 0 && N <= 65535 * 32, "jpeg_huff_decode: bad batch size N=%d", N);
    WU_REQUIRE(((uintptr_t)scan_dev & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)seg_dev & 3) == 0 &&
                   ((uintptr_t)hdesc_dev & 3) == 0 && ((uintptr_t)qtab_dev & 1) == 0 && ((uintptr_t)status_dev & 3) == 0,
               "jpeg_huff_decode: misaligned buffer");
    hipStream_t s = (hipStream_t)stream;
    const HuffDesc* hd = (const HuffDesc*)hdesc_dev;
    hipLaunchKernelGGL(jpeg_huff_zero_kernel, dim3(N, 8), dim3(kHuffThreads), 0, s, hd, coef_dev);
    hipLaunchKernelGGL(jpeg_huff_walk_kernel, dim3(N), dim3(kHuffThreads), 0, s, scan_dev, seg_dev, dht_dev, hd, coef_dev, status_dev, subseq_bits);
    hipLaunchKernelGGL(jpeg_huff_dc_kernel, dim3(N, 3), dim3(kHuffThreads), 0, s, hd, qtab_dev, coef_dev, status_dev, wu_jpeg_max_block_l1());
    WU_LAUNCH_CHECK("jpeg_huff_decode");
    return 0;
}
