// GIF encoding of the demo animation on the GPU: the last writer behind the inference drivers that ran on the host (Pillow's median-cut
// quantiser and LZW, single-threaded per frame, over frames fetched as raw RGB).
//
// T frames (uint8 interleaved RGB through arbitrary non-negative element strides) become T GIF89a image blocks -- graphic control
// extension, image descriptor, 256-entry local colour table, LZW data in 255-byte sub-blocks.  Frames are independent: no dithering, no
// inter-frame state.  All integer, deterministic; restated line by line in tests/_gif_enc_ref.py.  One memset and five launches:
//   1. histogram: 32768 bins over the top 5 bits of each channel, a count and three 64-bit channel sums per bin.  A thread walks 16
//      consecutive pixels and adds a run of equal bins at once; where a whole wave ends on the same bin (padding, flat cells) the wave adds
//      its runs together and one lane does the atomics.
//   2. median cut: one workgroup per frame, every thread keeping its 32 bins' counts and box numbers in registers, the boxes' counts and
//      tight bounds in LDS.  Up to 255 splits: the box with the largest count x extent (ties: the lowest index; only boxes with an extent)
//      is cut along its longest axis (ties: R, G, B) at the smallest coordinate k with 2 cumulative >= count, k <= max - 1; the bins above
//      k take the next box number; both boxes get tight bounds again.  Palette entry = (2 sum + n) / (2 n) per channel; the bin -> index
//      table goes to the workspace.
//   3. map + LZW: one wave per segment of 8192 pixels.  All lanes map the segment's pixels to indices in LDS and clear the dictionary (an
//      open-addressed hash of 32-bit entries, key (prefix << 8 | byte) << 12 | code, 8192 slots); the walk is wave-uniform, lane 0 stores.
//      Every segment starts from the fresh state (width 9, next code 258), so segments are independent; each ends in a Clear code -- the last
//      in the end-of-information code -- at the width the decoder has then: it adds one more entry for that code, so the width goes up if
//      next == 1 << width.  The bit string goes into the segment's own worst-case slot, its bit length into an array.
//   4. scan: exclusive prefix sum of the bit lengths per frame.
//   5. assemble: a gather.  Every 16 payload bytes find their segment by binary search and take their bits from at most two segments (a
//      segment has 18 bits or more); the same launch writes the fixed bytes in front, the sub-block lengths, the terminator and the count.
//
// A block never exceeds wu_gif_enc_block_stride: every pixel one 12-bit code, and per segment the table-full Clears (at most 2 in 8192
// pixels: 3838 codes are assigned between two), the trailing code and the leading Clear.  No overflow path, no fallback.
//
// The median cut, the LZW walk and the gather are written to compile as host C++ too (WU_GIF_ENC_EMU: scratch/gif_enc_emu.cpp runs them
// single-threaded under the address and undefined-behaviour sanitizers against the restatement's bytes).
#ifdef WU_GIF_ENC_EMU
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#define WU_HD inline
#define WU_SYNC() do {} while (0)
#define WU_UNIFORM(x) (x)
template <typename T> inline void lds_add(T* p, T v) { *p += v; }
template <typename T> inline void lds_min(T* p, T v) { if (v < *p) *p = v; }
template <typename T> inline void lds_max(T* p, T v) { if (v > *p) *p = v; }
#else
#include "wu_common.h"
#define WU_HD __device__ __forceinline__
#define WU_SYNC() __syncthreads()
#define WU_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
template <typename T> __device__ __forceinline__ void lds_add(T* p, T v) { atomicAdd(p, v); }
template <typename T> __device__ __forceinline__ void lds_min(T* p, T v) { atomicMin(p, v); }
template <typename T> __device__ __forceinline__ void lds_max(T* p, T v) { atomicMax(p, v); }
#endif

namespace {

constexpr int kSeg = 8192;                 // pixels per LZW segment
constexpr int kBins = 32768;               // histogram bins: 5 bits per channel
constexpr int kHash = 8192;                // dictionary slots (at most 3838 in use)
constexpr int kSlotWords = 3080;           // 32-bit words of a segment's slot: 12 (kSeg + 4) bits are 3074 words, the gather reads one past its word
constexpr int kFixed = 8 + 10 + 768 + 1;   // graphic control extension, image descriptor, local colour table, minimum code size
constexpr int kChunk = 16;                 // payload bytes per thread of the gather
constexpr long long kMaxPixels = 1ll << 26;
typedef unsigned long long u64;

struct GifGeo {
    long long npix, pmax, stride;          // pixels, worst-case payload bytes, worst-case block bytes
    int nseg;
};
inline bool gif_geo(int h, int w, GifGeo& g) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || (long long)h * w > kMaxPixels) return false;
    g.npix = (long long)h * w;
    g.nseg = (int)((g.npix + kSeg - 1) / kSeg);
    g.pmax = (12 * (g.npix + 4ll * g.nseg) + 7) / 8;
    g.stride = kFixed + g.pmax + (g.pmax + 254) / 255 + 1;
    return true;
}

// ---- 2. median cut ------------------------------------------------------------------------------------------------------------------------
struct McLds {
    u64 sum[256][3];
    u64 best;                  // (count x extent) << 8 | 255 - box: the maximum is the box to split, the lowest index among equals
    uint32_t n[256];
    uint32_t lo[256][3], hi[256][3];
    uint32_t marg[32];
};

// Thread `tid` of NT owns bins tid + NT j.  cnt: the frame's kBins counts; sums: [3][kBins]; writes table[kBins] and pal[768].
template <int NT>
WU_HD void median_cut(const uint32_t* cnt_g, const u64* sums_g, uint8_t* table_g, uint8_t* pal_g, McLds& L, int tid) {
    constexpr int kPer = kBins / NT;
    uint32_t cnt[kPer];
    uint8_t bx[kPer];
    for (int i = tid; i < 256; i += NT) {
        L.n[i] = 0u;
        for (int c = 0; c < 3; ++c) { L.lo[i][c] = 31u; L.hi[i][c] = 0u; L.sum[i][c] = 0ull; }
    }
    for (int i = tid; i < 32; i += NT) L.marg[i] = 0u;
    if (tid == 0) L.best = 0ull;
    WU_SYNC();
    {
        uint32_t ln = 0u, llo[3] = {31u, 31u, 31u}, lhi[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const uint32_t b = (uint32_t)(j * NT + tid);
            cnt[j] = cnt_g[b];
            bx[j] = 0;
            if (cnt[j]) {
                ln += cnt[j];
                const uint32_t co[3] = {b >> 10, (b >> 5) & 31u, b & 31u};
                for (int c = 0; c < 3; ++c) { llo[c] = co[c] < llo[c] ? co[c] : llo[c]; lhi[c] = co[c] > lhi[c] ? co[c] : lhi[c]; }
            }
        }
        if (ln) {
            lds_add(&L.n[0], ln);
            for (int c = 0; c < 3; ++c) { lds_min(&L.lo[0][c], llo[c]); lds_max(&L.hi[0][c], lhi[c]); }
        }
    }
    WU_SYNC();
    int nb = 1;
    while (nb < 256) {
        for (int i = tid; i < nb; i += NT) {
            uint32_t ext = 0u;
            for (int c = 0; c < 3; ++c) ext = L.hi[i][c] - L.lo[i][c] > ext ? L.hi[i][c] - L.lo[i][c] : ext;
            if (ext) lds_max(&L.best, ((u64)(L.n[i] * ext) << 8) | (u64)(255 - i));           // n <= 2^26, ext <= 31
        }
        WU_SYNC();
        const u64 key = L.best;
        if (key == 0ull) break;                                            // no box has an extent: every box is one bin
        const int sel = 255 - (int)(key & 255ull);
        const uint32_t nsel = L.n[sel];
        const uint32_t e0 = L.hi[sel][0] - L.lo[sel][0], e1 = L.hi[sel][1] - L.lo[sel][1], e2 = L.hi[sel][2] - L.lo[sel][2];
        const int axis = (e0 >= e1 && e0 >= e2) ? 0 : (e1 >= e2 ? 1 : 2);
        const int shift = 10 - 5 * axis;
        const uint32_t lo_a = L.lo[sel][axis], hi_a = L.hi[sel][axis];
#pragma unroll
        for (int j = 0; j < kPer; ++j)
            if (cnt[j] && bx[j] == sel) lds_add(&L.marg[((uint32_t)(j * NT + tid) >> shift) & 31u], cnt[j]);
        WU_SYNC();
        uint32_t k = lo_a, cum = L.marg[lo_a];
        while (2u * cum < nsel && k + 1u < hi_a) { ++k; cum += L.marg[k]; }
        WU_SYNC();                                                         // everyone has read the box and the marginal
        for (int i = tid; i < 32; i += NT) L.marg[i] = 0u;
        if (tid == 0) {
            L.best = 0ull;
            L.n[sel] = L.n[nb] = 0u;
            for (int c = 0; c < 3; ++c) { L.lo[sel][c] = L.lo[nb][c] = 31u; L.hi[sel][c] = L.hi[nb][c] = 0u; }
        }
        WU_SYNC();
        {
            uint32_t ln[2] = {0u, 0u}, llo[2][3] = {{31u, 31u, 31u}, {31u, 31u, 31u}}, lhi[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
#pragma unroll
            for (int j = 0; j < kPer; ++j) {
                if (cnt[j] && bx[j] == sel) {
                    const uint32_t b = (uint32_t)(j * NT + tid);
                    const uint32_t co[3] = {b >> 10, (b >> 5) & 31u, b & 31u};
                    const int side = ((b >> shift) & 31u) > k ? 1 : 0;
                    if (side) bx[j] = (uint8_t)nb;
                    ln[side] += cnt[j];
                    for (int c = 0; c < 3; ++c) {
                        llo[side][c] = co[c] < llo[side][c] ? co[c] : llo[side][c];
                        lhi[side][c] = co[c] > lhi[side][c] ? co[c] : lhi[side][c];
                    }
                }
            }
            for (int s = 0; s < 2; ++s) {
                if (ln[s]) {
                    const int i = s ? nb : sel;
                    lds_add(&L.n[i], ln[s]);
                    for (int c = 0; c < 3; ++c) { lds_min(&L.lo[i][c], llo[s][c]); lds_max(&L.hi[i][c], lhi[s][c]); }
                }
            }
        }
        WU_SYNC();
        ++nb;
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int b = j * NT + tid;
        table_g[b] = cnt[j] ? bx[j] : (uint8_t)0;
        if (cnt[j])
            for (int c = 0; c < 3; ++c) lds_add(&L.sum[bx[j]][c], sums_g[c * kBins + b]);
    }
    WU_SYNC();
    for (int i = tid; i < 256; i += NT) {
        const u64 n = L.n[i];
        for (int c = 0; c < 3; ++c) pal_g[3 * i + c] = i < nb ? (uint8_t)((2ull * L.sum[i][c] + n) / (2ull * n)) : (uint8_t)0;
    }
}

// ---- 3. LZW -----------------------------------------------------------------------------------------------------------------------------------
struct LzwLds {
    uint32_t hash[kHash];      // 0: empty; else key << 12 | code, key = prefix << 8 | byte (20 bits), code >= 258
    uint32_t idx[kSeg / 4];    // the segment's indices, one byte each
};

// One segment of `npx` indices (already in L.idx, not yet published by a barrier) by NL lanes in step; returns its bit length.  Every value
// of the walk is the same in all lanes; lane 0 stores.  slot: kSlotWords words; the last word written is zero above the last bit.
template <int NL>
WU_HD uint32_t lzw_segment(LzwLds& L, int npx, bool first, bool last, uint32_t* slot, int lane) {
    for (int i = lane; i < kHash; i += NL) L.hash[i] = 0u;
    WU_SYNC();
    u64 acc = 0ull;
    int nacc = 0;
    uint32_t nw = 0u;
    auto emit = [&](uint32_t code, int nbits) {
        acc |= (u64)code << nacc;
        nacc += nbits;
        if (nacc >= 32) {
            if (lane == 0) slot[nw] = (uint32_t)acc;
            ++nw;
            acc >>= 32;
            nacc -= 32;
        }
    };
    int width = 9;
    uint32_t next = 258u;
    if (first) emit(256u, 9);
    uint32_t four = WU_UNIFORM(L.idx[0]);
    uint32_t prefix = four & 255u;
    for (int p = 1; p < npx; ++p) {
        if ((p & 3) == 0) four = WU_UNIFORM(L.idx[p >> 2]);
        const uint32_t b = (four >> (8 * (p & 3))) & 255u;
        const uint32_t key = (prefix << 8) | b;
        uint32_t h = (key * 2654435761u) >> 19;
        uint32_t found = 0u;
        for (;;) {
            const uint32_t e = WU_UNIFORM(L.hash[h]);
            if (e == 0u) break;
            if ((e >> 12) == key) { found = e & 4095u; break; }
            h = (h + 1u) & (uint32_t)(kHash - 1);
        }
        if (found) { prefix = found; continue; }
        emit(prefix, width);
        if (next < 4096u) {
            if (lane == 0) L.hash[h] = (key << 12) | next;
            if (next == (1u << width) && width < 12) ++width;
            ++next;
        } else {                                                           // table full: Clear, and the fresh state
            emit(256u, width);
            WU_SYNC();
            for (int i = lane; i < kHash; i += NL) L.hash[i] = 0u;
            WU_SYNC();
            width = 9;
            next = 258u;
        }
        prefix = b;
    }
    emit(prefix, width);
    if (next < 4096u && next == (1u << width) && width < 12) ++width;     // the decoder adds an entry for the code just sent
    emit(last ? 257u : 256u, width);
    if (nacc > 0 && lane == 0) slot[nw] = (uint32_t)acc;
    return nw * 32u + (uint32_t)nacc;
}

// ---- 5. assemble --------------------------------------------------------------------------------------------------------------------------------
// off[0 .. nseg]: the exclusive scan of the segments' bit lengths.  The largest s < nseg with off[s] <= bit.
WU_HD int find_segment(const uint32_t* off, int nseg, uint32_t bit) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= bit) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Payload byte j: bits [8 j, 8 j + 8) of the concatenated bit strings, zeros past the end.  s: a segment at or before the byte's, advanced.
WU_HD uint32_t payload_byte(const uint32_t* off, const uint32_t* slots, int nseg, uint32_t j, int& s) {
    const uint32_t bit = 8u * j;
    while (s + 1 < nseg && off[s + 1] <= bit) ++s;
    const uint32_t q = bit - off[s], avail = off[s + 1] - bit;           // avail >= 1
    const uint32_t* w = slots + (size_t)s * kSlotWords + (q >> 5);
    const int sh = (int)(q & 31u);
    u64 win = w[0];
    if (sh + 8 > 32 && avail > (uint32_t)(32 - sh)) win |= (u64)w[1] << 32;
    uint32_t v = (uint32_t)(win >> sh) & 255u;
    if (avail < 8u) {
        v &= (1u << avail) - 1u;
        if (s + 1 < nseg) v |= (slots[(size_t)(s + 1) * kSlotWords] << avail) & 255u;      // a segment has 18 bits or more
    }
    return v;
}

WU_HD uint32_t fixed_byte(int i, int h, int w, int delay_cs, const uint8_t* pal) {
    if (i >= 18) return i < 18 + 768 ? pal[i - 18] : 8u;                  // the colour table, then the minimum code size
    switch (i) {
        case 0: return 0x21u;
        case 1: return 0xF9u;
        case 2: return 4u;
        case 3: return 4u;                                                // disposal 1: leave the frame in place
        case 4: return (uint32_t)delay_cs & 255u;
        case 5: return ((uint32_t)delay_cs >> 8) & 255u;
        case 8: return 0x2Cu;
        case 13: return (uint32_t)w & 255u;
        case 14: return ((uint32_t)w >> 8) & 255u;
        case 15: return (uint32_t)h & 255u;
        case 16: return ((uint32_t)h >> 8) & 255u;
        case 17: return 0x87u;                                            // local colour table of 256 entries
        default: return 0u;
    }
}

// Work item g of a frame's block: g < nchunk gathers payload bytes [16 g, 16 g + 16) with their sub-block length bytes; the kFixed + 1 items
// behind write one fixed byte each, the last of them the terminator and the byte count.
WU_HD void assemble_item(long long g, long long nchunk, const uint32_t* off, const uint32_t* slots, int nseg, const uint8_t* pal, int h, int w,
                         int delay_cs, uint8_t* out, int* result) {
    const uint32_t P = (off[nseg] + 7u) >> 3;
    if (g < nchunk) {
        const uint32_t j0 = (uint32_t)g * kChunk;
        if (j0 >= P) return;
        const uint32_t j1 = j0 + kChunk < P ? j0 + kChunk : P;
        int s = find_segment(off, nseg, 8u * j0);
        for (uint32_t j = j0; j < j1; ++j) {
            const size_t pos = (size_t)kFixed + j + j / 255u + 1u;
            if (j % 255u == 0u) out[pos - 1] = (uint8_t)(P - j < 255u ? P - j : 255u);
            out[pos] = (uint8_t)payload_byte(off, slots, nseg, j, s);
        }
        return;
    }
    const long long i = g - nchunk;
    if (i < kFixed) {
        out[i] = (uint8_t)fixed_byte((int)i, h, w, delay_cs, pal);
    } else if (i == kFixed) {
        const size_t end = (size_t)kFixed + P + (P + 254u) / 255u;
        out[end] = 0;
        *result = (int)(end + 1);
    }
}

struct Layout {
    size_t off_sums, off_cnt, off_table, off_pal, off_len, off_off, off_slots, total;
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool make_layout(int T, int h, int w, GifGeo& g, Layout& L) {
    if (T < 1 || T > 65535 || !gif_geo(h, w, g)) return false;
    size_t at = 0;
    L.off_sums = at;  at += (size_t)T * 3 * kBins * sizeof(u64);          // sums and counts are one region: one memset
    L.off_cnt = at;   at = align256(at + (size_t)T * kBins * sizeof(uint32_t));
    L.off_table = at; at = align256(at + (size_t)T * kBins);
    L.off_pal = at;   at = align256(at + (size_t)T * 768);
    L.off_len = at;   at = align256(at + (size_t)T * g.nseg * sizeof(uint32_t));
    L.off_off = at;   at = align256(at + (size_t)T * (g.nseg + 1) * sizeof(uint32_t));
    L.off_slots = at; at = align256(at + (size_t)T * g.nseg * kSlotWords * sizeof(uint32_t));
    L.total = at;
    return true;
}

#ifndef WU_GIF_ENC_EMU
// ---- 1. histogram ---------------------------------------------------------------------------------------------------------------------------
constexpr int kRun = 16;       // consecutive pixels per thread

__device__ __forceinline__ void hist_flush(uint32_t* cnt, u64* sums, int bin, uint32_t c, uint32_t sr, uint32_t sg, uint32_t sb) {
    atomicAdd(cnt + bin, c);
    atomicAdd(sums + bin, (u64)sr);
    atomicAdd(sums + kBins + bin, (u64)sg);
    atomicAdd(sums + 2 * kBins + bin, (u64)sb);
}

__global__ __launch_bounds__(256) void gif_hist_kernel(const uint8_t* __restrict__ frames, long long st, long long sy, long long sx, long long sc,
                                                       uint32_t* __restrict__ cnt, u64* __restrict__ sums, int H, int W) {
    const int t = blockIdx.y;
    const int npix = H * W;
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * kRun;
    cnt += (size_t)t * kBins;
    sums += (size_t)t * 3 * kBins;
    int cur = -1;
    uint32_t c = 0u, sr = 0u, sg = 0u, sb = 0u;
    if (first < npix) {
        const int p0 = (int)first, n = min(kRun, npix - p0);
        int y = p0 / W, x = p0 - y * W;
        const uint8_t* base = frames + (long long)t * st;
        for (int i = 0; i < n; ++i) {
            const uint8_t* px = base + (long long)y * sy + (long long)x * sx;
            const uint32_t r = px[0], g = px[sc], b = px[2 * sc];
            const int bin = (int)(((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3));
            if (bin != cur) {
                if (c) hist_flush(cnt, sums, cur, c, sr, sg, sb);
                cur = bin;
                c = sr = sg = sb = 0u;
            }
            ++c; sr += r; sg += g; sb += b;
            if (++x == W) { x = 0; ++y; }
        }
    }
    // the run every thread still holds: where the whole wave holds the same bin, one set of atomics for the wave
    const int lead = __builtin_amdgcn_readfirstlane(cur);
    if (__all(cur == lead) && lead >= 0) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            c += __shfl_xor(c, d);
            sr += __shfl_xor(sr, d);
            sg += __shfl_xor(sg, d);
            sb += __shfl_xor(sb, d);
        }
        if ((threadIdx.x & 63) == 0) hist_flush(cnt, sums, lead, c, sr, sg, sb);      // 64 x 16 x 255 fits 32 bits
    } else if (c) {
        hist_flush(cnt, sums, cur, c, sr, sg, sb);
    }
}

// ---- 2. median cut ---------------------------------------------------------------------------------------------------------------------------
constexpr int kMcThreads = 1024;
__global__ __launch_bounds__(kMcThreads) void gif_median_cut_kernel(const uint32_t* __restrict__ cnt, const u64* __restrict__ sums,
                                                                     uint8_t* __restrict__ table, uint8_t* __restrict__ pal) {
    __shared__ McLds L;
    const int t = blockIdx.x;
    median_cut<kMcThreads>(cnt + (size_t)t * kBins, sums + (size_t)t * 3 * kBins, table + (size_t)t * kBins, pal + (size_t)t * 768, L, threadIdx.x);
}

// ---- 3. map + LZW ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gif_lzw_kernel(const uint8_t* __restrict__ frames, long long st, long long sy, long long sx, long long sc,
                                                     const uint8_t* __restrict__ table, uint32_t* __restrict__ slots, uint32_t* __restrict__ seglen,
                                                     int H, int W, int nseg) {
    __shared__ LzwLds L;
    const int seg = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const int npix = H * W, p0 = seg * kSeg, npx = min(kSeg, npix - p0);
    const uint8_t* base = frames + (long long)t * st;
    const uint8_t* tab = table + (size_t)t * kBins;
    uint8_t* idx = (uint8_t*)L.idx;
    for (int i = lane; i < npx; i += 64) {
        const int p = p0 + i, y = p / W, x = p - y * W;
        const uint8_t* px = base + (long long)y * sy + (long long)x * sx;
        const uint32_t r = px[0], g = px[sc], b = px[2 * sc];
        idx[i] = tab[((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)];
    }
    const uint32_t bits = lzw_segment<64>(L, npx, seg == 0, seg == nseg - 1, slots + ((size_t)t * nseg + seg) * kSlotWords, lane);
    if (lane == 0) seglen[(size_t)t * nseg + seg] = bits;
}

// ---- 4. scan -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gif_scan_kernel(const uint32_t* __restrict__ seglen, uint32_t* __restrict__ off, int nseg) {
    __shared__ uint32_t sm[256];
    __shared__ uint32_t carry;
    const int t = blockIdx.x, tid = threadIdx.x;
    seglen += (size_t)t * nseg;
    off += (size_t)t * (nseg + 1);
    if (tid == 0) { carry = 0u; off[0] = 0u; }
    __syncthreads();
    for (int at = 0; at < nseg; at += 256) {
        sm[tid] = at + tid < nseg ? seglen[at + tid] : 0u;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t add = tid >= d ? sm[tid - d] : 0u;
            __syncthreads();
            sm[tid] += add;
            __syncthreads();
        }
        const uint32_t base = carry;
        if (at + tid < nseg) off[at + tid + 1] = base + sm[tid];         // at most 12 (2^26 + 4 * 2^13) bits: fits 32
        __syncthreads();
        if (tid == 255) carry = base + sm[255];
        __syncthreads();
    }
}

// ---- 5. assemble --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gif_assemble_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ slots,
                                                           const uint8_t* __restrict__ pal, uint8_t* __restrict__ out, long long out_stride,
                                                           int* __restrict__ result, long long nchunk, int nseg, int H, int W, int delay_cs) {
    const int t = blockIdx.y;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g > nchunk + kFixed) return;
    assemble_item(g, nchunk, off + (size_t)t * (nseg + 1), slots + (size_t)t * nseg * kSlotWords, nseg, pal + (size_t)t * 768, H, W, delay_cs,
                  out + (size_t)t * out_stride, result + t);
}
#endif  // WU_GIF_ENC_EMU

}  // namespace

extern "C" size_t wu_gif_enc_segment_pixels(void) { return kSeg; }

extern "C" size_t wu_gif_enc_workspace_bytes(int T, int H, int W) {
    GifGeo g;
    Layout L;
    return make_layout(T, H, W, g, L) ? L.total : 0;
}

extern "C" size_t wu_gif_enc_block_stride(int H, int W) {
    GifGeo g;
    return gif_geo(H, W, g) ? (size_t)g.stride : 0;
}

#ifndef WU_GIF_ENC_EMU
extern "C" int wu_gif_enc_encode(const uint8_t* frames, long long st, long long sy, long long sx, long long sc, void* workspace,
                                 size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int T, int H, int W, int delay_cs,
                                 void* stream) {
    WU_REQUIRE(frames && workspace && out && result_dev, "gif_enc_encode: null argument");
    GifGeo g;
    Layout L;
    WU_REQUIRE(make_layout(T, H, W, g, L), "gif_enc_encode: bad shape T=%d H=%d W=%d", T, H, W);
    WU_REQUIRE(st >= 0 && sy >= 0 && sx >= 0 && sc >= 0, "gif_enc_encode: negative strides");
    WU_REQUIRE(delay_cs >= 0 && delay_cs <= 65535, "gif_enc_encode: delay %d outside 0..65535", delay_cs);
    WU_REQUIRE(workspace_bytes >= L.total, "gif_enc_encode: workspace too small (%zu of %zu bytes)", workspace_bytes, L.total);
    WU_REQUIRE(out_bytes >= (size_t)T * g.stride, "gif_enc_encode: output too small (%zu of %zu bytes)", out_bytes, (size_t)T * (size_t)g.stride);
    WU_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)result_dev & 3) == 0,
               "gif_enc_encode: workspace must be 256-byte aligned, results naturally aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    u64* sums = (u64*)(ws + L.off_sums);
    uint32_t* cnt = (uint32_t*)(ws + L.off_cnt);
    uint8_t* table = ws + L.off_table;
    uint8_t* pal = ws + L.off_pal;
    uint32_t* seglen = (uint32_t*)(ws + L.off_len);
    uint32_t* off = (uint32_t*)(ws + L.off_off);
    uint32_t* slots = (uint32_t*)(ws + L.off_slots);
    const hipError_t e = hipMemsetAsync(ws + L.off_sums, 0, L.off_table - L.off_sums, s);
    if (e != hipSuccess) WU_FAIL((int)e, "gif_enc_encode: memset: %s", hipGetErrorString(e));
    const unsigned hist_blocks = (unsigned)((g.npix + 256ll * kRun - 1) / (256ll * kRun));
    hipLaunchKernelGGL(gif_hist_kernel, dim3(hist_blocks, T), dim3(256), 0, s, frames, st, sy, sx, sc, cnt, sums, H, W);
    WU_LAUNCH_CHECK("gif_hist_kernel");
    hipLaunchKernelGGL(gif_median_cut_kernel, dim3(T), dim3(kMcThreads), 0, s, cnt, sums, table, pal);
    WU_LAUNCH_CHECK("gif_median_cut_kernel");
    hipLaunchKernelGGL(gif_lzw_kernel, dim3((unsigned)g.nseg, T), dim3(64), 0, s, frames, st, sy, sx, sc, table, slots, seglen, H, W, g.nseg);
    WU_LAUNCH_CHECK("gif_lzw_kernel");
    hipLaunchKernelGGL(gif_scan_kernel, dim3(T), dim3(256), 0, s, seglen, off, g.nseg);
    WU_LAUNCH_CHECK("gif_scan_kernel");
    const long long nchunk = (g.pmax + kChunk - 1) / kChunk;
    const unsigned asm_blocks = (unsigned)((nchunk + kFixed + 1 + 255) / 256);
    hipLaunchKernelGGL(gif_assemble_kernel, dim3(asm_blocks, T), dim3(256), 0, s, off, slots, pal, out, g.stride, result_dev, nchunk, g.nseg, H, W,
                       delay_cs);
    WU_LAUNCH_CHECK("gif_assemble_kernel");
    return 0;
}
#endif
