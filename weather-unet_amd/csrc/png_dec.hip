// PNG decoding of image batches: the reader of what png_enc.hip writes, and of every file framed the same way -- 8-bit RGB, colour
// type 2, no interlace, IDAT chunk k the deflate data of bytes [32768 k, 32768 (k + 1)) of the filtered stream (zlib's Z_FULL_FLUSH every
// 32 KiB, pigz -i).  The segment boundaries are then the chunk boundaries.
//
// Host: wu_png_dec_parse decides from chunk headers alone (twelve bytes per chunk, no pass over the image bytes, no GPU) whether a file is
// of that class and where its segments lie.
//
// Device: two launches for a whole batch whatever N and the image sizes, both with workgroups of ONE wave whose only ordering device is
// __syncthreads() -- a real fence for compiler and hardware that costs a single wave next to nothing.  Nothing relies on lanes running in
// step: every LDS location written by one lane and read by another has a __syncthreads() in between, which is what lets the CPU
// emulation (scratch/png_dec_emu.cpp: 64 free-running host threads per workgroup under ASan / UBSan / TSan) speak for the hardware.
//   1. png_dec_inflate_kernel, one wave per segment.  All lanes stage the chunk (type + body) in LDS and take its CRC-32 by slices.
//      Lane 0 alone then runs the serial part -- bit reader, block headers, the code-length code, symbol decode, short matches -- and
//      hands over through a few control words in LDS whenever 64 lanes help: the decode tables of a Huffman block (counts, `sorted`, the
//      10-bit `fast` table), a stored block's bytes, a match of kWideCopy bytes or more.  Output goes to a 32 KiB LDS window no distance
//      may leave.  Every table the decode loop indexes with stream data lives in LDS and every index is clamped to its array, so a
//      corrupt stream ends in a status, never in an address.  Epilogue, all lanes: Adler-32 partial sums, the filtered bytes to the
//      workspace at 32768 k inside the image.
//   2. png_dec_unfilter_kernel, one wave per image.  Segment statuses and the Adler-32 combined from the partial sums give the image's
//      status; the wave then reconstructs 64 rows at a time as a skewed wavefront -- lane r at column t - r, so left is the lane's own
//      previous pixel, up what lane r - 1 produced one step earlier, up-left the up of the step before.  A rejected image's slot is all
//      zeros, as is the padding of every slot.
//
// Status of an image: 0, or the first failing check of its first failing segment (chunk-crc, bad-stream, distance, segment-size), then
// filter-type, then adler.  tests/_png_dec_ref.py restates parser, inflate (with the order of the checks) and unfilter.
#include "png_internal.h"

namespace {

constexpr int kSeg = kPngSeg;
constexpr int kMaxBody = 40960;            // largest IDAT body taken: a fixed-Huffman segment of 9-bit literals is 36 KiB + a few bytes

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
uint32_t host_crc(const uint8_t* p, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    }
    return ~c;
}

}  // namespace

extern "C" size_t wu_png_dec_info_bytes(void) { return sizeof(wu_png_dec_info); }
extern "C" size_t wu_png_dec_max_chunk_bytes(void) { return kMaxBody; }

extern "C" int wu_png_dec_parse(const uint8_t* data, size_t nbytes, long long max_pixels, wu_png_dec_info* info, long long* idat,
                                int idat_capacity) {
    WU_REQUIRE(info && (data || nbytes == 0) && (idat || idat_capacity <= 0), "png_dec_parse: null argument");
    memset(info, 0, sizeof(*info));
    auto refuse = [&](int reason) { info->supported = 0; info->reason = reason; return 0; };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    const unsigned long long n = nbytes;                                  // every length below is held against n in 64 bits
    if (n < 8 || memcmp(data, sig, 8) != 0) return refuse(WU_PNG_DEC_NOT_PNG);
    if (n < 8 + 25 || be32(data + 8) != 13 || memcmp(data + 12, "IHDR", 4) != 0 || host_crc(data + 12, 17) != be32(data + 29))
        return refuse(WU_PNG_DEC_HEADER);
    const uint32_t w = be32(data + 16), h = be32(data + 20);
    const int depth = data[24], colour = data[25], comp = data[26], flt = data[27], lace = data[28];
    info->bit_depth = depth; info->colour_type = colour; info->interlace = lace;
    if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || comp != 0 || flt != 0 || lace > 1) return refuse(WU_PNG_DEC_HEADER);
    info->width = (int)w; info->height = (int)h;
    if (colour != 2) return refuse(WU_PNG_DEC_COLOUR_TYPE);
    if (depth != 8) return refuse(WU_PNG_DEC_BIT_DEPTH);
    if (lace != 0) return refuse(WU_PNG_DEC_INTERLACED);
    if ((unsigned long long)w * h > (unsigned long long)(max_pixels < 0 ? 0 : max_pixels) || w > 65535u || h > 65535u) return refuse(WU_PNG_DEC_TOO_LARGE);
    const unsigned long long flen = (unsigned long long)h * (1ull + 3ull * w);
    info->filtered_bytes = (long long)flen;
    info->n_segments = (int)((flen + kSeg - 1) / kSeg);
    unsigned long long at = 8 + 25;
    int state = 0;                                                        // 0: before the IDAT run, 1: inside, 2: behind
    unsigned long long first_off = 0, first_len = 0, last_len = 0;
    bool oversize = false, iend = false;
    while (!iend) {
        if (n - at < 12) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);         // at <= n always
        const unsigned long long len = be32(data + at);
        if (len > n - at - 12) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);
        const uint8_t* type = data + at + 4;
        const unsigned long long body = at + 8;
        if (memcmp(type, "IDAT", 4) == 0) {
            if (state == 2) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);      // IDAT chunks are consecutive
            state = 1;
            if (info->n_idat < idat_capacity) {
                idat[2 * info->n_idat] = (long long)body;
                idat[2 * info->n_idat + 1] = (long long)len;
            }
            if (info->n_idat == 0) { first_off = body; first_len = len; }
            last_len = len;
            oversize = oversize || len > (unsigned long long)kMaxBody;
            if (info->n_idat == 0x7FFFFFFF) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);
            ++info->n_idat;
        } else if (memcmp(type, "IEND", 4) == 0) {
            iend = true;
        } else {
            if (!(type[0] & 0x20)) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);   // a critical chunk this reader does not know, PLTE included
            if (state == 1) state = 2;
        }
        at = body + len + 4;
    }
    if (info->n_idat == 0) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);
    if (info->n_idat != info->n_segments || oversize || first_len < 2 || last_len < 4 || (info->n_idat == 1 && first_len < 6))
        return refuse(WU_PNG_DEC_NOT_SEGMENTED);
    {
        const int cmf = data[first_off], flg = data[first_off + 1];       // the zlib header
        if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return refuse(WU_PNG_DEC_CORRUPT_CHUNK);
    }
    info->supported = 1;
    info->reason = WU_PNG_DEC_OK;
    return 0;
}

// =============================================================================================================================================
// Device stage
// =============================================================================================================================================
#ifndef WU_LDS
#define WU_LDS(type, name) __shared__ type name        // the CPU emulation hands out poisoned heap memory per workgroup instead
#endif

namespace {

constexpr int kWave = 64;                              // threads per workgroup of both kernels: one wave
constexpr int kInWords = (8 + kMaxBody) / 4 + 16;      // staged chunk: up to 2 bytes of padding, type, body; 64 bytes of zeros behind
constexpr int kInBytes = 4 * kInWords;
constexpr int kFastBits = 10, kFast = 1 << kFastBits;
constexpr int kNumLit = 288, kNumDist = 32, kNumLens = kNumLit + kNumDist;
constexpr int kWideCopy = 16;                          // a match of this many bytes or more is copied by all lanes (unmeasured)

enum { ST_OK = 0, ST_CRC = 1, ST_STREAM = 2, ST_DIST = 3, ST_SIZE = 4, ST_FILTER = 5, ST_ADLER = 6 };
enum { EV_NONE = 0, EV_DONE = 1, EV_BUILD = 2, EV_STORED = 3, EV_COPY = 4 };          // what lane 0 asks of the wave
enum { C_EV = 0, C_STATUS = 1, C_A = 2, C_B = 3, C_C = 4, C_OK = 5, C_ADLER = 6, C_WORDS = 8 };
enum { PH_HEADER = 0, PH_SYMBOLS = 1, PH_AFTER = 2, PH_FAIL = 3 };

struct PngDecDesc {            // 32 bytes per image, built by the caller; h = w = 0: not decoded here, the slot is zeroed
    long long src_off;         // the file's first byte in the uploaded buffer
    int file_bytes;
    int h, w;
    int first_seg, nseg;       // its rows of the segment table
    int pad;
};
struct PngDecSeg {             // 16 bytes per segment
    int image, k;              // k-th segment of `image`
    uint32_t off, len;         // its IDAT body: offset inside the file, bytes
};

struct Geo {
    int h, w, nseg;
    long long row, len;        // bytes of a filtered row (1 + 3 w) and of the filtered stream
};
__host__ __device__ __forceinline__ Geo make_geo(int h, int w, int Hmax, int Wmax) {
    Geo g;
    g.h = h < 0 ? 0 : (h > Hmax ? Hmax : h);      // clamped to the batch bounds: a bad descriptor cannot make a kernel leave its buffers
    g.w = w < 0 ? 0 : (w > Wmax ? Wmax : w);
    if (g.h == 0 || g.w == 0) g.h = g.w = 0;
    g.row = 1 + 3ll * g.w;
    g.len = g.h ? g.row * g.h : 0;
    g.nseg = (int)((g.len + kSeg - 1) / kSeg);
    return g;
}
__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- 1. inflate -------------------------------------------------------------------------------------------------------------------------
// Read once, at kernel start, into LDS: the decode loop never turns stream data into a global address.
__device__ const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                           8193, 12289, 16385, 24577};
__device__ const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

struct CodeTab {               // one Huffman code: canonical decoding data and the first-level table
    uint32_t cnt[16];          // codes per length (cnt[0] = 0)
    uint16_t offs[16];         // first index of a length in `sorted`
    uint16_t next[16];         // first canonical code of a length
    uint16_t sorted[kNumLit];  // symbols by (length, symbol)
    uint16_t fast[kFast];      // symbol << 4 | length for codes of at most kFastBits bits, 0 elsewhere
};

struct InflateLds {
    uint32_t in[kInWords];     // the staged chunk, zeros behind it
    uint8_t win[kSeg];         // the inflated segment
    uint32_t crctab[256];
    uint32_t x8[32];
    CodeTab lit, dist;
    uint8_t lens[kNumLens];    // 288 literal/length code lengths, then 32 distance code lengths
    uint16_t len_base[32], dist_base[32];
    uint8_t len_extra[32], dist_extra[32], cl_order[32];
    uint8_t cl[32];            // the code-length code: lengths, symbols by (length, symbol), codes per length; lane 0 only
    uint8_t cl_sorted[32];
    uint32_t cl_cnt[8];
    int ctl[C_WORDS];
    uint32_t crc;
    unsigned long long adl[2];
};

struct BitReader {             // LSB-first over the staged words; positions are bits from the start of the staged array.  Lane 0 only.
    unsigned wi;
    unsigned long long bb;     // the low `nb` bits are unread
    int nb;
    __device__ __forceinline__ uint32_t word(const InflateLds& L, unsigned i) const { return i < (unsigned)kInWords ? L.in[i] : 0u; }
    __device__ __forceinline__ void seek(const InflateLds& L, unsigned bytepos) {
        wi = bytepos >> 2;
        const unsigned sh = 8u * (bytepos & 3u);
        bb = (unsigned long long)(word(L, wi) >> sh);
        ++wi;
        nb = 32 - (int)sh;
    }
    __device__ __forceinline__ void need(const InflateLds& L) {       // at least 33 bits afterwards (zeros behind the staged bytes)
        if (nb <= 32) {
            bb |= (unsigned long long)word(L, wi) << nb;
            ++wi;
            nb += 32;
        }
    }
    __device__ __forceinline__ uint32_t take(int n) {                 // n <= 16
        const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
        bb >>= n;
        nb -= n;
        return v;
    }
    __device__ __forceinline__ long long pos() const { return 32ll * wi - nb; }
};

__device__ __forceinline__ uint32_t crc_shift_lds(const InflateLds& L, uint32_t crc, unsigned after) {       // crc_shift with the LDS copy of x8
    for (int k = 0; after && k < 32; ++k, after >>= 1)
        if (after & 1u) crc = mulmodp(crc, L.x8[k]);
    return crc;
}

// A symbol of code `t`, or -1 where the bits are no code of it.  The reader holds at least 15 bits.
__device__ __forceinline__ int decode_sym(BitReader& br, const CodeTab& t) {
    const uint32_t e = t.fast[(uint32_t)br.bb & (uint32_t)(kFast - 1)];
    if (e) {
        br.take((int)(e & 15u));
        return (int)(e >> 4);
    }
    uint32_t bits = (uint32_t)br.bb;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = (int)t.cnt[len];
        if (code - c < first) {
            br.take(len);
            const int at = index + (code - first);
            return (at >= 0 && at < kNumLit) ? (int)t.sorted[at] : -1;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// The same for the code-length code, whose 19 symbols of at most 7 bits need no table.
__device__ __forceinline__ int decode_cl(BitReader& br, const InflateLds& L) {
    uint32_t bits = (uint32_t)br.bb;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 7; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = (int)L.cl_cnt[len];
        if (code - c < first) {
            br.take(len);
            const int at = index + (code - first);
            return (at >= 0 && at < 19) ? (int)L.cl_sorted[at] : -1;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// zlib's inflate_table verdict on counted lengths, and the canonical first code / first index per length.  Lane 0.
__device__ __forceinline__ bool finish_counts(CodeTab& t, bool single_ok) {
    int left = 1, code = 0, off = 0, maxlen = 0, prev = 0;
    bool ok = true;
    for (int b = 1; b < 16; ++b) {
        const int c = (int)t.cnt[b];
        left = 2 * left - c;
        if (left < 0) { ok = false; left = 0; }
        code = (code + prev) << 1;
        prev = c;
        t.next[b] = (uint16_t)code;
        t.offs[b] = (uint16_t)off;
        off += c;
        if (c) maxlen = b;
    }
    if (!ok) return false;
    return !(left > 0 && !(single_ok && maxlen <= 1));
}

// `sorted` and `fast` of a counted code whose `fast` is zeroed: every lane takes symbols lane, lane + 64, ...  No lane reads what another writes.
__device__ __forceinline__ void fill_tab(const InflateLds& L, int base, int n, CodeTab& t, int lane) {
    for (int sym = lane; sym < n; sym += kWave) {
        const int l = L.lens[base + sym];
        if (l < 1 || l > 15) continue;
        int rank = 0;
        for (int s = 0; s < sym; ++s) rank += L.lens[base + s] == l ? 1 : 0;
        const int at = (int)t.offs[l] + rank;
        if (at < kNumLit) t.sorted[at] = (uint16_t)sym;
        if (l <= kFastBits) {
            const uint32_t code = (uint32_t)t.next[l] + (uint32_t)rank;
            const uint32_t rev = __brev(code) >> (32 - l);
            for (uint32_t k = rev; k < (uint32_t)kFast; k += 1u << l) t.fast[k] = (uint16_t)((sym << 4) | l);
        }
    }
}

// A dynamic block's header behind its three type bits: the code lengths to L.lens.  Lane 0.
__device__ __forceinline__ int dynamic_header(BitReader& br, InflateLds& L, long long end_bits) {
    br.need(L);
    const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
    for (int i = 0; i < 19; ++i) L.cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        br.need(L);
        L.cl[L.cl_order[i] & 31] = (uint8_t)br.take(3);
    }
    if (nlen > 286 || ndist > 30) return ST_STREAM;
    for (int b = 0; b < 8; ++b) L.cl_cnt[b] = 0u;
    for (int i = 0; i < 19; ++i) L.cl_cnt[L.cl[i] & 7] += 1u;
    L.cl_cnt[0] = 0u;
    int left = 1;
    for (int b = 1; b < 8; ++b) {
        left = 2 * left - (int)L.cl_cnt[b];
        if (left < 0) return ST_STREAM;
    }
    if (left > 0) return ST_STREAM;
    int at = 0;
    for (int b = 1; b < 8; ++b)
        for (int i = 0; i < 19; ++i)
            if (L.cl[i] == b && at < 19) L.cl_sorted[at++] = (uint8_t)i;
    for (int i = 0; i < kNumLens / 4; ++i) ((uint32_t*)L.lens)[i] = 0u;
    const int total = nlen + ndist;
    int have = 0, prev = 0;
    while (have < total) {
        br.need(L);
        const int sym = decode_cl(br, L);
        if (sym < 0 || sym > 18) return ST_STREAM;
        int rep = 1, val = sym;
        if (sym == 16) {
            if (have == 0) return ST_STREAM;
            val = prev;
            rep = 3 + (int)br.take(2);
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (int)br.take(3);
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (int)br.take(7);
        }
        if (have + rep > total) return ST_STREAM;
        for (int q = 0; q < rep; ++q) {                               // literal/length lengths at 0, distance lengths at kNumLit
            const int i = have + q;
            L.lens[clampi(i < nlen ? i : kNumLit + (i - nlen), 0, kNumLens - 1)] = (uint8_t)val;
        }
        have += rep;
        prev = val;
    }
    if (br.pos() > end_bits) return ST_STREAM;
    if (L.lens[256] == 0) return ST_STREAM;                           // no end-of-block code
    return ST_OK;
}

// seginfo: 4 words per segment: status, sum of the bytes mod 65521, sum of (len - j) * byte_j mod 65521, the stream's Adler-32 (last segment)
__global__ __launch_bounds__(64) void png_dec_inflate_kernel(const uint8_t* __restrict__ src, long long src_bytes,
                                                             const PngDecDesc* __restrict__ desc, const PngDecSeg* __restrict__ segs,
                                                             int n_segments, uint8_t* __restrict__ filt, long long fstride,
                                                             long long filt_bytes, uint32_t* __restrict__ seginfo, int N, int Hmax, int Wmax) {
    WU_LDS(InflateLds, L);
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= n_segments || lane >= kWave) return;                     // uniform per workgroup
    uint32_t* info = seginfo + 4ll * s;
    const PngDecSeg sg = segs[s];
    bool bad = sg.image < 0 || sg.image >= N;
    const PngDecDesc d = desc[bad ? 0 : sg.image];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    // the chunk as the file has it: length(4) type(4) body(len) crc(4); everything is checked against the file and the buffers
    bad = bad || sg.k < 0 || sg.k >= g.nseg || sg.len > (uint32_t)kMaxBody || sg.off < 8u || d.file_bytes < 0 || d.src_off < 0 ||
          (long long)sg.off + sg.len + 4 > (long long)d.file_bytes || d.src_off + d.file_bytes > src_bytes ||
          (long long)sg.image * fstride + ((long long)sg.k + 1) * kSeg > filt_bytes;
    if (bad) {
        if (lane == 0) { info[0] = ST_STREAM; info[1] = info[2] = info[3] = 0u; }
        return;
    }
    const bool last = sg.k == g.nseg - 1;
    const int expected = (int)min((long long)kSeg, g.len - (long long)sg.k * kSeg);       // 1 .. kSeg
    const int hdr = sg.k == 0 ? 2 : 0;                                // the zlib header, checked by the parser
    const int pad = hdr ? 2 : 0;                                      // the deflate data starts on a word of the staged array
    const int vlen = 4 + (int)sg.len;                                 // type + body: what the CRC covers
    const int staged = pad + vlen;                                    // <= 2 + 4 + kMaxBody < kInBytes - 64
    const uint8_t* chunk = src + d.src_off + sg.off - 4;
    uint8_t* sbytes = (uint8_t*)L.in;
    // ---- tables and the chunk to LDS, all lanes ----
    for (int i = lane; i < kInWords; i += kWave) L.in[i] = 0u;
    for (int i = lane; i < 256; i += kWave) L.crctab[i] = kCrcTab.byte[i];
    if (lane < 32) {
        L.x8[lane] = kCrcTab.x8[lane];
        L.len_base[lane] = lane < 29 ? kLenBase[lane] : (uint16_t)0;
        L.len_extra[lane] = lane < 29 ? kLenExtra[lane] : (uint8_t)0;
        L.dist_base[lane] = lane < 30 ? kDistBase[lane] : (uint16_t)0;
        L.dist_extra[lane] = lane < 30 ? kDistExtra[lane] : (uint8_t)0;
        L.cl_order[lane] = lane < 19 ? kClOrder[lane] : (uint8_t)0;
    }
    if (lane == 0) {
        L.crc = 0u;
        for (int i = 0; i < C_WORDS; ++i) L.ctl[i] = 0;
        L.adl[0] = L.adl[1] = 0ull;
    }
    __syncthreads();
    for (int i = lane; i < vlen; i += kWave) sbytes[clampi(pad + i, 0, kInBytes - 1)] = chunk[i];
    __syncthreads();
    {
        const int per = (vlen + kWave - 1) / kWave, lo = min(lane * per, vlen), hi = min(lo + per, vlen);
        const uint32_t c = crc_shift_lds(L, crc_bytes(L.crctab, sbytes + pad + lo, hi - lo), (unsigned)(vlen - hi));
        if (c) atomicXor(&L.crc, c);
    }
    __syncthreads();
    const uint32_t want_crc = ((uint32_t)chunk[vlen] << 24) | ((uint32_t)chunk[vlen + 1] << 16) | ((uint32_t)chunk[vlen + 2] << 8) | chunk[vlen + 3];
    if (L.crc != want_crc) {                                          // uniform: every lane reads the same word behind the barrier
        if (lane == 0) { info[0] = ST_CRC; info[1] = info[2] = info[3] = 0u; }
        return;
    }
    // ---- the blocks.  Lane 0 decodes until it has something for the wave, publishes it in L.ctl, and every lane meets at barrier A;
    // the wave does its part and meets again at barrier B, behind which lane 0 may rewrite L.ctl and read what the wave wrote. ----
    const int dstart = pad + 4 + hdr;                                 // a multiple of 4
    const long long end_bits = 8ll * staged;
    BitReader br;                                                     // lane 0's: br, opos, bfinal, phase
    br.wi = 0; br.bb = 0ull; br.nb = 0;
    int opos = 0, bfinal = 0;
    int phase = hdr > (int)sg.len ? PH_FAIL : PH_HEADER;              // no room for the zlib header (the parser refuses such a file)
    int fail = ST_STREAM;
    if (lane == 0) br.seek(L, (unsigned)dstart);
    int status = ST_OK;
    for (;;) {
        if (lane == 0) {
            int ev = EV_NONE, a = 0, b = 0, c = 0;
            while (ev == EV_NONE) {
                if (phase == PH_FAIL) {
                    ev = EV_DONE; a = fail;
                } else if (phase == PH_HEADER) {
                    br.need(L);
                    bfinal = (int)br.take(1);
                    const int btype = (int)br.take(2);
                    if (br.pos() > end_bits || btype == 3 || (bfinal && !last)) {
                        phase = PH_FAIL; fail = ST_STREAM;
                    } else if (btype == 0) {
                        br.take(br.nb & 7);                           // to the byte boundary
                        br.need(L);
                        const uint32_t len = br.take(16), nlen = br.take(16);
                        const long long p = br.pos() >> 3;            // byte position in the staged array
                        if (br.pos() > end_bits || (len ^ 0xFFFFu) != nlen || p + (long long)len > (long long)staged) { phase = PH_FAIL; fail = ST_STREAM; }
                        else if (opos + (int)len > expected) { phase = PH_FAIL; fail = ST_SIZE; }
                        else {
                            ev = EV_STORED; a = opos; b = (int)len; c = (int)p;
                            opos += (int)len;
                            br.seek(L, (unsigned)(p + len));
                            phase = PH_AFTER;
                        }
                    } else if (btype == 1) {
                        ev = EV_BUILD; a = 1;
                        phase = PH_SYMBOLS;
                    } else {
                        const int st = dynamic_header(br, L, end_bits);
                        if (st != ST_OK) { phase = PH_FAIL; fail = st; }
                        else { ev = EV_BUILD; a = 2; phase = PH_SYMBOLS; }
                    }
                } else if (phase == PH_SYMBOLS) {
                    for (;;) {
                        br.need(L);
                        int sym = decode_sym(br, L.lit);
                        if (sym < 0 || sym > 285) { phase = PH_FAIL; fail = ST_STREAM; break; }
                        if (sym < 256) {
                            if (br.pos() > end_bits) { phase = PH_FAIL; fail = ST_STREAM; break; }
                            if (opos >= expected) { phase = PH_FAIL; fail = ST_SIZE; break; }
                            L.win[clampi(opos, 0, kSeg - 1)] = (uint8_t)sym;
                            ++opos;
                            continue;
                        }
                        if (sym == 256) {
                            if (br.pos() > end_bits) { phase = PH_FAIL; fail = ST_STREAM; }
                            else phase = PH_AFTER;
                            break;
                        }
                        sym = clampi(sym - 257, 0, 28);
                        const int len = (int)L.len_base[sym] + (int)br.take((int)L.len_extra[sym] & 7);
                        br.need(L);
                        const int ds = decode_sym(br, L.dist);
                        if (ds < 0 || ds > 29) { phase = PH_FAIL; fail = ST_STREAM; break; }
                        const int dist = (int)L.dist_base[ds] + (int)br.take((int)L.dist_extra[ds] & 15);
                        if (br.pos() > end_bits) { phase = PH_FAIL; fail = ST_STREAM; break; }
                        if (dist > opos) { phase = PH_FAIL; fail = ST_DIST; break; }
                        if (opos + len > expected) { phase = PH_FAIL; fail = ST_SIZE; break; }
                        if (len >= kWideCopy) {
                            ev = EV_COPY; a = opos; b = len; c = dist;
                            opos += len;
                            break;
                        }
                        for (int i = 0; i < len; ++i) L.win[clampi(opos + i, 0, kSeg - 1)] = L.win[clampi(opos - dist + i, 0, kSeg - 1)];
                        opos += len;
                    }
                } else {                                              // PH_AFTER: is the segment complete?
                    if (bfinal) {
                        const long long p = (br.pos() + 7) >> 3;
                        if ((long long)staged - p != 4) { phase = PH_FAIL; fail = ST_STREAM; }       // exactly the Adler-32 must follow
                        else if (opos != expected) { phase = PH_FAIL; fail = ST_SIZE; }
                        else {
                            const int q = clampi((int)p, 0, kInBytes - 4);
                            L.ctl[C_ADLER] = (int)(((uint32_t)sbytes[q] << 24) | ((uint32_t)sbytes[q + 1] << 16) | ((uint32_t)sbytes[q + 2] << 8) | sbytes[q + 3]);
                            ev = EV_DONE; a = ST_OK;
                        }
                    } else if (br.pos() >= end_bits) {
                        if (br.pos() > end_bits || last) { phase = PH_FAIL; fail = ST_STREAM; }      // ran out; or no final block
                        else if (opos != expected) { phase = PH_FAIL; fail = ST_SIZE; }
                        else { ev = EV_DONE; a = ST_OK; }
                    } else {
                        phase = PH_HEADER;
                    }
                }
            }
            L.ctl[C_EV] = ev; L.ctl[C_A] = a; L.ctl[C_B] = b; L.ctl[C_C] = c;
        }
        __syncthreads();                                              // A
        const int ev = L.ctl[C_EV], a = L.ctl[C_A], b = L.ctl[C_B], c = L.ctl[C_C];
        if (ev == EV_DONE) {
            status = a;
            break;
        }
        if (ev == EV_STORED) {                                        // b bytes from staged position c to window position a
            for (int i = lane; i < b; i += kWave) L.win[clampi(a + i, 0, kSeg - 1)] = sbytes[clampi(c + i, 0, kInBytes - 1)];
        } else if (ev == EV_COPY) {                                   // b bytes at window position a from distance c: sources all lie below a
            if (c >= 1 && c <= a) {
                if (c >= b) {
                    for (int i = lane; i < b; i += kWave) L.win[clampi(a + i, 0, kSeg - 1)] = L.win[clampi(a - c + i, 0, kSeg - 1)];
                } else {                                              // overlapping: the source repeats with period c
                    for (int i = lane; i < b; i += kWave) L.win[clampi(a + i, 0, kSeg - 1)] = L.win[clampi(a - c + i % c, 0, kSeg - 1)];
                }
            }
        } else if (ev == EV_BUILD) {                                  // a = 1: the fixed code, 2: the lengths lane 0 left in L.lens
            if (a == 1) {
                for (int i = lane; i < kNumLit; i += kWave) L.lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
                if (lane < kNumDist) L.lens[kNumLit + lane] = 5;
            }
            if (lane < 16) { L.lit.cnt[lane] = 0u; L.dist.cnt[lane] = 0u; }
            for (int i = lane; i < kFast; i += kWave) { L.lit.fast[i] = 0; L.dist.fast[i] = 0; }
            __syncthreads();
            for (int i = lane; i < kNumLens; i += kWave) {
                const int l = L.lens[i] & 15;
                if (l) atomicAdd(i < kNumLit ? &L.lit.cnt[l] : &L.dist.cnt[l], 1u);
            }
            __syncthreads();
            if (lane == 0) {
                const bool ok_lit = finish_counts(L.lit, a == 2), ok_dist = finish_counts(L.dist, a == 2);
                L.ctl[C_OK] = (ok_lit && ok_dist) ? 1 : 0;
            }
            __syncthreads();
            if (L.ctl[C_OK]) {
                fill_tab(L, 0, kNumLit, L.lit, lane);
                fill_tab(L, kNumLit, kNumDist, L.dist, lane);
            } else if (lane == 0) {
                phase = PH_FAIL; fail = ST_STREAM;
            }
        }
        __syncthreads();                                              // B
    }
    if (status == ST_OK) {
        // Adler-32 partial sums and the filtered bytes to their place, all lanes
        constexpr int kPerLane = kSeg / kWave;
        uint32_t s1 = 0u;
        unsigned long long s2 = 0ull;
        const int first = lane * kPerLane;
        for (int i = first; i < min(first + kPerLane, expected); ++i) {
            const uint32_t v = L.win[i];
            s1 += v;
            s2 += (unsigned long long)((uint32_t)(expected - i) * v);
        }
        if (s1) {
            atomicAdd(&L.adl[0], (unsigned long long)s1);
            atomicAdd(&L.adl[1], s2);
        }
        uint8_t* o = filt + (long long)sg.image * fstride + (long long)sg.k * kSeg;         // 256-byte aligned
        const int words = expected >> 2;
        for (int i = lane; i < words; i += kWave) ((uint32_t*)o)[i] = ((const uint32_t*)L.win)[i];
        if (lane < (expected & 3)) o[4 * words + lane] = L.win[4 * words + lane];
    }
    __syncthreads();
    if (lane == 0) {
        info[0] = (uint32_t)status;
        info[1] = (uint32_t)(L.adl[0] % kAdlerMod);
        info[2] = (uint32_t)(L.adl[1] % kAdlerMod);
        info[3] = (uint32_t)L.ctl[C_ADLER];
    }
}

// ---- 2. unfilter ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t load3(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

// x: the filtered bytes, a: left, b: above, c: above left; three channels packed in the low 24 bits
__device__ __forceinline__ uint32_t reconstruct(int ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int xv = (int)((x >> (8 * ch)) & 255u), av = (int)((a >> (8 * ch)) & 255u), bv = (int)((b >> (8 * ch)) & 255u),
                  cv = (int)((c >> (8 * ch)) & 255u);
        int pred = 0;
        if (ft == 1) pred = av;
        else if (ft == 2) pred = bv;
        else if (ft == 3) pred = (av + bv) >> 1;
        else if (ft == 4) {
            const int p = av + bv - cv, pa = abs(p - av), pb = abs(p - bv), pc = abs(p - cv);
            pred = (pa <= pb && pa <= pc) ? av : (pb <= pc ? bv : cv);
        }
        r |= (uint32_t)((xv + pred) & 255) << (8 * ch);
    }
    return r;
}

__device__ __forceinline__ void zero_bytes(uint8_t* p, long long n, int t, int nt) {     // threads t of nt; dwords where the alignment allows
    if (n <= 0) return;
    const long long head = min(n, (long long)((4 - ((uintptr_t)p & 3)) & 3));
    for (long long i = t; i < head; i += nt) p[i] = 0;
    const long long words = (n - head) >> 2;
    uint32_t* q = (uint32_t*)(p + head);
    for (long long i = t; i < words; i += nt) q[i] = 0u;
    for (long long i = head + 4 * words + t; i < n; i += nt) p[i] = 0;
}

struct UnfilterLds {
    unsigned fail, flt;
    unsigned long long a, b;
};

constexpr int kUnroll = 8;                 // pixels whose filtered bytes are fetched ahead of the dependent chain

__global__ __launch_bounds__(64) void png_dec_unfilter_kernel(const uint8_t* __restrict__ filt, long long fstride, long long filt_bytes,
                                                              const PngDecDesc* __restrict__ desc, const PngDecSeg* __restrict__ segs,
                                                              const uint32_t* __restrict__ seginfo, int n_segments, uint8_t* out,
                                                              int* __restrict__ status_out, int N, int Hmax, int Wmax) {
    WU_LDS(UnfilterLds, U);
    const int n = blockIdx.x, lane = threadIdx.x;
    if (n >= N || lane >= kWave) return;                              // uniform per workgroup
    const PngDecDesc d = desc[n];
    const Geo g = make_geo(d.h, d.w, Hmax, Wmax);
    const long long slot_bytes = (long long)Hmax * Wmax * 3;
    uint8_t* slot = out + (long long)n * slot_bytes;
    const uint8_t* fbase = filt + (long long)n * fstride;
    if (g.h == 0) {                                                   // not a native image: zeros, status 0
        zero_bytes(slot, slot_bytes, lane, kWave);
        if (lane == 0) status_out[n] = ST_OK;
        return;
    }
    if (lane == 0) { U.fail = 0xFFFFFFFFu; U.flt = 0u; U.a = 0ull; U.b = 0ull; }
    __syncthreads();
    const bool table_ok = d.nseg == g.nseg && d.first_seg >= 0 && (long long)d.first_seg + g.nseg <= (long long)n_segments &&
                          (long long)n * fstride + g.len <= filt_bytes && g.len <= fstride;
    if (table_ok) {
        unsigned long long a = 0ull, b = 0ull;
        unsigned fail = 0xFFFFFFFFu;
        for (int j = lane; j < g.nseg; j += kWave) {
            const PngDecSeg sg = segs[d.first_seg + j];
            const uint32_t* info = seginfo + 4ll * (d.first_seg + j);
            unsigned st = info[0];
            if (sg.image != n || sg.k != j) st = ST_STREAM;
            if (st != ST_OK) { fail = min(fail, ((unsigned)j << 3) | (st & 7u)); continue; }
            // A = 1 + sum d_i, B = len + sum (len - i) d_i, mod 65521, from the segments' sums (the encoder's frame kernel)
            const long long after = max(g.len - (long long)(j + 1) * kSeg, 0ll);
            a += info[1];
            b = (b + info[2] + (unsigned long long)(after % kAdlerMod) * info[1]) % kAdlerMod;
        }
        if (fail != 0xFFFFFFFFu) atomicMin(&U.fail, fail);
        if (a) atomicAdd(&U.a, a);
        if (b) atomicAdd(&U.b, b);
    }
    __syncthreads();
    int status = ST_OK;
    if (!table_ok) status = ST_STREAM;
    else if (U.fail != 0xFFFFFFFFu) status = (int)(U.fail & 7u);
    if (status == ST_OK) {                                            // uniform: every segment of the image was written
        unsigned f = 0u;
        for (int y = lane; y < g.h; y += kWave) f |= fbase[(long long)y * g.row] > 4 ? 1u : 0u;
        if (f) atomicOr(&U.flt, 1u);
    }
    __syncthreads();
    if (status == ST_OK) {
        const uint32_t adler = (uint32_t)(((U.b + (unsigned long long)(g.len % kAdlerMod)) % kAdlerMod) << 16) | (uint32_t)((1ull + U.a) % kAdlerMod);
        if (U.flt) status = ST_FILTER;
        else if (adler != seginfo[4ll * (d.first_seg + g.nseg - 1) + 3]) status = ST_ADLER;
    }
    if (lane == 0) status_out[n] = status;
    if (status != ST_OK) {                                            // uniform
        zero_bytes(slot, slot_bytes, lane, kWave);
        return;
    }
    {                                                                 // the padding right of and below the image
        const long long tail = 3ll * (Wmax - g.w);
        if (tail > 0)
            for (long long i = lane; i < tail * g.h; i += kWave) {
                const long long y = i / tail, x = i - y * tail;
                slot[(y * Wmax + g.w) * 3 + x] = 0;
            }
        zero_bytes(slot + (long long)g.h * Wmax * 3, (long long)(Hmax - g.h) * Wmax * 3, lane, kWave);
    }
    // 64 rows at a time, lane r at column t - r.  Every lane runs every step of every group, so the shuffles and barriers are uniform.
    for (int y0 = 0; y0 < g.h; y0 += kWave) {
        const int y = y0 + lane;
        const bool active = y < g.h;
        const uint8_t* frow = fbase + (long long)(active ? y : y0) * g.row;
        const int ft = active ? frow[0] : 0;
        uint8_t* orow = slot + (long long)(active ? y : y0) * Wmax * 3;
        const uint8_t* prow = orow - (long long)Wmax * 3;              // read by lane 0 only, and only below row 0
        const int steps = g.w + min(kWave, g.h - y0) - 1;
        uint32_t cur = 0u, ul = 0u;
        for (int t0 = 0; t0 < steps; t0 += kUnroll) {
            uint32_t xs[kUnroll], ups[kUnroll];
#pragma unroll
            for (int j = 0; j < kUnroll; ++j) {
                const int px = t0 + j - lane;
                const bool valid = active && px >= 0 && px < g.w;
                xs[j] = valid ? load3(frow + 1 + 3 * px) : 0u;
                ups[j] = (valid && lane == 0 && y > 0) ? load3(prow + 3 * px) : 0u;
            }
#pragma unroll
            for (int j = 0; j < kUnroll; ++j) {
                const int px = t0 + j - lane;
                const uint32_t got = __shfl_up(cur, 1);               // what the row above produced one step ago: its column px
                if (active && px >= 0 && px < g.w) {
                    const uint32_t up = lane == 0 ? ups[j] : got;
                    const uint32_t res = reconstruct(ft, xs[j], px > 0 ? cur : 0u, up, px > 0 ? ul : 0u);
                    orow[3 * px] = (uint8_t)res;
                    orow[3 * px + 1] = (uint8_t)(res >> 8);
                    orow[3 * px + 2] = (uint8_t)(res >> 16);
                    cur = res;
                    ul = up;
                }
            }
        }
        __syncthreads();                                              // lane 63's row is read back by lane 0 of the next 64 rows
    }
}

// ---- host: layout -------------------------------------------------------------------------------------------------------------------------
struct Layout {
    long long fstride, nseg_max;
    size_t off_filt, off_info, total;
};
size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
bool make_layout(int N, int Hmax, int Wmax, long long n_segments, Layout& L) {
    if (N <= 0 || Hmax <= 0 || Wmax <= 0 || Hmax > 65535 || Wmax > 65535 || n_segments < 0 || n_segments > 0x7FFFFFFFll) return false;
    const Geo g = make_geo(Hmax, Wmax, Hmax, Wmax);
    if (g.len >= (1ll << 30) || g.len * N >= (1ll << 36) || n_segments > (long long)N * g.nseg) return false;
    L.nseg_max = g.nseg;
    L.fstride = (long long)align256((size_t)g.nseg * kSeg);             // whole segments: the inflate kernel stores dwords
    size_t at = 0;
    L.off_filt = at; at = align256(at + (size_t)N * L.fstride);
    L.off_info = at; at = align256(at + (size_t)(n_segments > 0 ? n_segments : 1) * 16);
    L.total = at;
    return true;
}

}  // namespace

extern "C" size_t wu_png_dec_desc_bytes(void) { return sizeof(PngDecDesc); }
extern "C" size_t wu_png_dec_seg_bytes(void) { return sizeof(PngDecSeg); }

extern "C" size_t wu_png_dec_workspace_bytes(int N, int Hmax, int Wmax, long long n_segments) {
    Layout L;
    return make_layout(N, Hmax, Wmax, n_segments, L) ? L.total : 0;
}

extern "C" int wu_png_dec_decode(const uint8_t* src_dev, size_t src_bytes, const void* desc_dev, size_t desc_bytes, const void* seg_dev,
                                 size_t seg_bytes, int n_segments, void* workspace, size_t workspace_bytes, uint8_t* out_u8, size_t out_bytes,
                                 int* status_dev, size_t status_bytes, int N, int Hmax, int Wmax, void* stream) {
    WU_REQUIRE(src_dev && desc_dev && seg_dev && workspace && out_u8 && status_dev, "png_dec_decode: null argument");
    Layout L;
    WU_REQUIRE(make_layout(N, Hmax, Wmax, n_segments, L), "png_dec_decode: bad shape N=%d Hmax=%d Wmax=%d segments=%d", N, Hmax, Wmax, n_segments);
    // every IDAT chunk is twelve bytes of framing around its body
    WU_REQUIRE(src_bytes < ((size_t)1 << 40) && src_bytes >= (size_t)12 * (size_t)n_segments,
               "png_dec_decode: source of %zu bytes for %d segments", src_bytes, n_segments);
    WU_REQUIRE(desc_bytes >= (size_t)N * sizeof(PngDecDesc), "png_dec_decode: descriptor table too small (%zu of %zu bytes)", desc_bytes,
               (size_t)N * sizeof(PngDecDesc));
    WU_REQUIRE(seg_bytes >= (size_t)n_segments * sizeof(PngDecSeg), "png_dec_decode: segment table too small (%zu of %zu bytes)", seg_bytes,
               (size_t)n_segments * sizeof(PngDecSeg));
    WU_REQUIRE(workspace_bytes >= L.total, "png_dec_decode: workspace too small (%zu of %zu bytes)", workspace_bytes, L.total);
    WU_REQUIRE(out_bytes >= (size_t)N * Hmax * Wmax * 3, "png_dec_decode: output too small (%zu of %zu bytes)", out_bytes, (size_t)N * Hmax * Wmax * 3);
    WU_REQUIRE(status_bytes >= (size_t)N * sizeof(int), "png_dec_decode: status buffer too small (%zu of %zu bytes)", status_bytes,
               (size_t)N * sizeof(int));
    WU_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)desc_dev & 7) == 0 && ((uintptr_t)seg_dev & 3) == 0 && ((uintptr_t)status_dev & 3) == 0,
               "png_dec_decode: workspace must be 256-byte aligned, descriptors / segment table / status naturally aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    uint8_t* filt = ws + L.off_filt;
    const long long filt_bytes = (long long)N * L.fstride;
    uint32_t* info = (uint32_t*)(ws + L.off_info);
    const PngDecDesc* desc = (const PngDecDesc*)desc_dev;
    const PngDecSeg* segs = (const PngDecSeg*)seg_dev;
    if (n_segments > 0) {
        hipLaunchKernelGGL(png_dec_inflate_kernel, dim3((unsigned)n_segments), dim3(kWave), 0, s, src_dev, (long long)src_bytes, desc, segs,
                           n_segments, filt, L.fstride, filt_bytes, info, N, Hmax, Wmax);
        WU_LAUNCH_CHECK("png_dec_inflate_kernel");
    }
    hipLaunchKernelGGL(png_dec_unfilter_kernel, dim3((unsigned)N), dim3(kWave), 0, s, filt, L.fstride, filt_bytes, desc, segs, info, n_segments,
                       out_u8, status_dev, N, Hmax, Wmax);
    WU_LAUNCH_CHECK("png_dec_unfilter_kernel");
    return 0;
}
