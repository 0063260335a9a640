// PNG decoding, host side: the header parse that decides from chunk headers alone whether a file is one whose IDAT chunks are independent
// 32 KiB deflate segments -- 8-bit RGB, colour type 2, no interlace, IDAT chunk k the deflate data of bytes [32768 k, 32768 (k + 1)) of the
// filtered stream: what png_enc.hip writes, and what zlib's Z_FULL_FLUSH every 32 KiB or pigz -i produce -- and where its segments lie.
// Such a file can be inflated segment by segment in parallel; the segment boundaries are the chunk boundaries, found here from twelve
// bytes per chunk with no pass over the image bytes.  No GPU is needed or touched.  tests/_png_dec_ref.py restates the parse (and the
// per-segment inflate, its checks and the unfilter a device stage has to reproduce).
#include "wu_common.h"

namespace {

constexpr int kSeg = 32768;                // filtered bytes per deflate segment (wu_png_enc_segment_bytes)
constexpr int kMaxBody = 40960;            // largest IDAT body taken: a fixed-Huffman segment of 9-bit literals is 36 KiB + a few bytes
constexpr uint32_t kCrcPoly = 0xEDB88320u;

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
