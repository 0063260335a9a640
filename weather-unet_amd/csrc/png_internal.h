// What the PNG encoder (png_enc.hip) and decoder (png_dec.hip) share: the segment size of the filtered stream, the CRC-32 by
// slices -- per-thread CRCs combined by multiplication with x^(8 n) mod P -- and deflate's code-length order.
#pragma once
#include "wu_common.h"

namespace {

constexpr int kPngSeg = 32768;             // filtered bytes per deflate segment (wu_png_enc_segment_bytes)
constexpr uint32_t kAdlerMod = 65521u;

// ---- CRC-32 (reflected, polynomial EDB88320) --------------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t mulmodp(uint32_t a, uint32_t b) {          // a * b mod P; bit 31 is x^0
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
struct CrcTab {
    uint32_t byte[256];        // the usual byte-wise table
    uint32_t x8[32];           // x^(8 * 2^k) mod P
};
constexpr CrcTab make_crc_tab() {
    CrcTab t = {};
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        t.byte[i] = c;
    }
    t.x8[0] = 0x00800000u;     // x^8
    for (int k = 1; k < 32; ++k) t.x8[k] = mulmodp(t.x8[k - 1], t.x8[k - 1]);
    return t;
}
__device__ const CrcTab kCrcTab = make_crc_tab();

__device__ __forceinline__ uint32_t crc_bytes(const uint32_t* tab, const uint8_t* p, int n) {        // zlib's crc32(0, p, n); 0 for n = 0
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
    return n > 0 ? ~c : 0u;
}
// the CRC of a message followed by `after` more bytes, as far as this message contributes to it: crc * x^(8 after) mod P
__device__ __forceinline__ uint32_t crc_shift(uint32_t crc, unsigned after) {
    for (int k = 0; after; ++k, after >>= 1)
        if (after & 1u) crc = mulmodp(crc, kCrcTab.x8[k]);
    return crc;
}

// ---- deflate ----------------------------------------------------------------------------------------------------------------------
__device__ const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};      // RFC 1951 3.2.7: the order of the code-length code's lengths

}  // namespace
