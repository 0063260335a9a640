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
// Quality options (wu_gif_enc_encode_ex; flags == 0 is everything above, byte for byte; restated in tests/_gif_quality_ref.py), in the same
// five launches:
//   exact    launch 1 also keeps the distinct 24-bit colours in an open-addressed set (atomicCAS, a counter, an overflow flag at the 257th);
//            launch 2 sorts and ranks a set of at most 256 into the palette instead of cutting, and launch 3 finds a pixel's rank in it.
//   nearest  launch 3 maps a pixel to the nearest palette entry in use -- a brute-force search over the palette in LDS, eight pixels per lane
//            at a time -- instead of the box of its bin.
//   ordered  ... after an 8 x 8 ordered dither from the pixel's position in the frame, one step of the box at most (launch 2 exports the
//            boxes' bounds) and 16 levels at most.
//   global   one histogram, one set, one palette for all frames; the blocks carry no local colour table.
//
// The median cut, the LZW walk, the gather, the set's insert, the ranking and the pixel map are written to compile as host C++ too
// (WU_GIF_ENC_EMU: scratch/gif_enc_emu.cpp runs them single-threaded under the address and undefined-behaviour sanitizers against the
// restatements' bytes).
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
template <typename T> inline T lds_inc(T* p) { return (*p)++; }
inline uint32_t mem_load(const uint32_t* p) { return *p; }
inline uint32_t mem_cas(uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t old = *p; if (old == expect) *p = v; return old; }
inline uint32_t mem_add(uint32_t* p, uint32_t v) { const uint32_t old = *p; *p += v; return old; }
inline void mem_set(uint32_t* p, uint32_t v) { *p = v; }
#else
#include "wu_common.h"
#define WU_HD __device__ __forceinline__
#define WU_SYNC() __syncthreads()
#define WU_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
template <typename T> __device__ __forceinline__ void lds_add(T* p, T v) { atomicAdd(p, v); }
template <typename T> __device__ __forceinline__ void lds_min(T* p, T v) { atomicMin(p, v); }
template <typename T> __device__ __forceinline__ void lds_max(T* p, T v) { atomicMax(p, v); }
template <typename T> __device__ __forceinline__ T lds_inc(T* p) { return atomicAdd(p, (T)1); }
// global memory shared by all workgroups of a launch: relaxed, device scope
__device__ __forceinline__ uint32_t mem_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t mem_cas(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
__device__ __forceinline__ uint32_t mem_add(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
__device__ __forceinline__ void mem_set(uint32_t* p, uint32_t v) { atomicExch(p, v); }
#endif

namespace {

constexpr int kSeg = 8192;                 // pixels per LZW segment
constexpr int kBins = 32768;               // histogram bins: 5 bits per channel
constexpr int kHash = 8192;                // dictionary slots (at most 3838 in use)
constexpr int kSlotWords = 3080;           // 32-bit words of a segment's slot: 12 (kSeg + 4) bits are 3074 words, the gather reads one past its word
constexpr int kFixed = 8 + 10 + 768 + 1;   // graphic control extension, image descriptor, local colour table, minimum code size
constexpr int kChunk = 16;                 // payload bytes per thread of the gather
constexpr int kFixedGlobal = 8 + 10 + 1;   // ... under a global palette: no local colour table
constexpr long long kMaxPixels = 1ll << 26;
constexpr long long kMaxPixelsGlobal = (1ll << 32) - 1;      // all frames of a global palette: one 32-bit count per bin and per box
constexpr int kSetSlots = 1024;            // exact palettes: slots of the colour set (at most 257 + the inserts in flight in use)
constexpr uint32_t kSetUsed = 1u << 24;    // a slot: the 24-bit colour | kSetUsed; 0: empty
enum { kNearest = 1, kDither = 2, kExact = 4, kGlobal = 8, kAllFlags = 15 };
typedef unsigned long long u64;

struct GifGeo {
    long long npix, pmax, stride;          // pixels, worst-case payload bytes, worst-case block bytes
    int nseg, fixed;                       // segments; the fixed bytes in front of the payload
};
inline bool gif_geo(int h, int w, GifGeo& g, int flags = 0) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || (long long)h * w > kMaxPixels) return false;
    if (flags & ~kAllFlags || ((flags & kDither) && !(flags & kNearest))) return false;
    g.npix = (long long)h * w;
    g.nseg = (int)((g.npix + kSeg - 1) / kSeg);
    g.pmax = (12 * (g.npix + 4ll * g.nseg) + 7) / 8;
    g.fixed = flags & kGlobal ? kFixedGlobal : kFixed;
    g.stride = g.fixed + g.pmax + (g.pmax + 254) / 255 + 1;
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

// Thread `tid` of NT owns bins tid + NT j.  cnt: the frame's kBins counts; sums: [3][kBins]; writes table[kBins] and pal[768]; where given,
// bounds[256] (a box's final tight bounds, 5 bits each: lo R, hi R, lo G, hi G, lo B, hi B from bit 0; 0 past the boxes in use) and
// pinfo[2] = {boxes in use, 0}.  The counts of one box stay below 2^32 (kMaxPixelsGlobal).
template <int NT>
WU_HD void median_cut(const uint32_t* cnt_g, const u64* sums_g, uint8_t* table_g, uint8_t* pal_g, McLds& L, int tid, uint32_t* bounds_g = nullptr,
                      int* pinfo = nullptr) {
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
            if (ext) lds_max(&L.best, (((u64)L.n[i] * ext) << 8) | (u64)(255 - i));           // n < 2^32, ext <= 31
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
        uint32_t k = lo_a;
        u64 cum = L.marg[lo_a];
        while (2ull * cum < nsel && k + 1u < hi_a) { ++k; cum += L.marg[k]; }
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
        if (bounds_g)
            bounds_g[i] = i < nb ? L.lo[i][0] | (L.hi[i][0] << 5) | (L.lo[i][1] << 10) | (L.hi[i][1] << 15) | (L.lo[i][2] << 20) | (L.hi[i][2] << 25) : 0u;
    }
    if (pinfo && tid == 0) { pinfo[0] = nb; pinfo[1] = 0; }
}

// ---- 2b. exact palette ------------------------------------------------------------------------------------------------------------------------
// The colour set (kSetSlots slots, each 0 or colour | kSetUsed; ctl[0]: entries, ctl[1]: overflow) is filled by set_insert, one call per
// pixel that differs from its left neighbour in the thread's run.  No loop here waits for anyone: a probe ends at the colour, at an empty
// slot it then takes (or loses to the same colour: done; to another: goes on), or after kSetProbe steps: 256 colours or fewer leave an
// empty slot within any 257, so a longer run means overflow.  A set that has counted its 257th colour sets the overflow flag too.  Every
// thread reads the flag before its first insert, and again every 8 steps of a long probe, and stops inserting for good (`live`) once it
// is set: a photograph stops inserting almost at once.
constexpr int kSetProbe = 257;
WU_HD uint32_t set_hash(uint32_t colour) { return (colour * 2654435761u) >> 22; }                     // 10 bits: kSetSlots

WU_HD void set_insert(uint32_t* set, uint32_t* ctl, uint32_t colour, bool& live) {
    const uint32_t mine = colour | kSetUsed;
    uint32_t h = set_hash(colour);
    for (int step = 0; step < kSetProbe; ++step) {
        if ((step & 7) == 7 && mem_load(ctl + 1)) { live = false; return; }
        uint32_t e = mem_load(set + h);
        if (e == 0u) {
            e = mem_cas(set + h, 0u, mine);
            if (e == 0u) {                                                 // a new colour: the 257th is one too many
                if (mem_add(ctl, 1u) >= 256u) { mem_set(ctl + 1, 1u); live = false; }
                return;
            }
        }
        if (e == mine) return;
        h = (h + 1u) & (uint32_t)(kSetSlots - 1);
    }
    mem_set(ctl + 1, 1u);
    live = false;
}

struct ExLds {
    uint32_t key[256];
    uint32_t n;
};
// A set of at most 256 colours -> pal[768]: the colours in ascending order of r << 16 | g << 8 | b, zeros behind; pinfo = {colours, 1}.
// The rank of a colour is the number of smaller ones, so the order the slots are read in does not matter.
template <int NT>
WU_HD void exact_rank(const uint32_t* set_g, uint8_t* pal_g, int* pinfo, ExLds& L, int tid) {
    if (tid == 0) L.n = 0u;
    WU_SYNC();
    for (int i = tid; i < kSetSlots; i += NT) {
        const uint32_t e = set_g[i];
        if (e) {
            const uint32_t at = lds_inc(&L.n);
            if (at < 256u) L.key[at] = e & 0xFFFFFFu;
        }
    }
    WU_SYNC();
    const int n = L.n < 256u ? (int)L.n : 256;
    for (int i = tid; i < 256; i += NT) {
        if (i < n) {
            const uint32_t k = L.key[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += L.key[j] < k ? 1 : 0;
            pal_g[3 * rank] = (uint8_t)(k >> 16);
            pal_g[3 * rank + 1] = (uint8_t)(k >> 8);
            pal_g[3 * rank + 2] = (uint8_t)k;
        } else {
            pal_g[3 * i] = pal_g[3 * i + 1] = pal_g[3 * i + 2] = 0;
        }
    }
    if (tid == 0) { pinfo[0] = n; pinfo[1] = 1; }
}

// ---- 3a. pixel -> index under the options ------------------------------------------------------------------------------------------------------
struct alignas(16) MapLds {
    int pal[256][4];           // r, g, b, r << 16 | g << 8 | b
    uint32_t amp[256];         // dither amplitudes of a box: A_r | A_g << 8 | A_b << 16, A_c = min(16, 8 (hi_c - lo_c + 1))
};

// The 8 x 8 ordered-dither threshold of a position, 0 .. 63: bit b of x and y gives the digit ((x_b ^ y_b) << 1 | y_b) at 2 (2 - b).
WU_HD int dither_m(int x, int y) {
    int m = 0;
    for (int b = 0; b < 3; ++b) {
        const int xb = (x >> b) & 1, yb = (y >> b) & 1;
        m |= (((xb ^ yb) << 1) | yb) << (2 * (2 - b));
    }
    return m;
}

WU_HD void map_load(MapLds& M, const uint8_t* pal_g, const uint32_t* bounds_g, int tid, int nt) {
    for (int i = tid; i < 256; i += nt) {
        const int r = pal_g[3 * i], g = pal_g[3 * i + 1], b = pal_g[3 * i + 2];
        M.pal[i][0] = r; M.pal[i][1] = g; M.pal[i][2] = b; M.pal[i][3] = (r << 16) | (g << 8) | b;
        uint32_t a = 0u;
        if (bounds_g) {
            const uint32_t v = bounds_g[i];
            for (int c = 0; c < 3; ++c) {
                const uint32_t step = 8u * (((v >> (10 * c + 5)) & 31u) - ((v >> (10 * c)) & 31u) + 1u);
                a |= (step < 16u ? step : 16u) << (8 * c);
            }
        }
        M.amp[i] = a;
    }
}

constexpr int kGroup = 8;      // pixels a lane searches side by side: one read of a palette entry serves all of them

// The rank of a colour among the n sorted colours of an exact palette (the colour is one of them).
WU_HD uint32_t exact_index(const MapLds& M, int n, int r, int g, int b) {
    const int key = (r << 16) | (g << 8) | b;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (M.pal[mid][3] < key) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

// The colour searched for a pixel at (x, y) whose bin lies in `box`: one step of the box at most, from the position only.
WU_HD void dither_colour(const MapLds& M, uint32_t box, int x, int y, int& r, int& g, int& b) {
    const int t = 2 * dither_m(x, y) + 1 - 64;
    const uint32_t a = M.amp[box];
    r += (t * (int)(a & 255u)) >> 7;                                        // an arithmetic shift: the floor
    g += (t * (int)((a >> 8) & 255u)) >> 7;
    b += (t * (int)((a >> 16) & 255u)) >> 7;
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    g = g < 0 ? 0 : (g > 255 ? 255 : g);
    b = b < 0 ? 0 : (b > 255 ? 255 : b);
}

// at[u] = the entry among 0 .. n - 1 (n >= 1) at the smallest squared distance from colour u: brute force, ascending and strict, so ties go
// to the lowest index.  The next entry is read while this one is compared.
WU_HD void nearest_entries(const MapLds& M, int n, const int (&r)[kGroup], const int (&g)[kGroup], const int (&b)[kGroup], uint32_t (&at)[kGroup]) {
    int best[kGroup];
#pragma unroll
    for (int u = 0; u < kGroup; ++u) { best[u] = 0x7FFFFFFF; at[u] = 0u; }
    int er = M.pal[0][0], eg = M.pal[0][1], eb = M.pal[0][2];
    for (int j = 0; j < n; ++j) {
        const int jn = j + 1 < n ? j + 1 : j;
        const int nr = M.pal[jn][0], ng = M.pal[jn][1], nb = M.pal[jn][2];
#pragma unroll
        for (int u = 0; u < kGroup; ++u) {
            const int dr = r[u] - er, dg = g[u] - eg, db = b[u] - eb;
            const int d = dr * dr + dg * dg + db * db;
            if (d < best[u]) { best[u] = d; at[u] = (uint32_t)j; }
        }
        er = nr; eg = ng; eb = nb;
    }
}

// The indices of the npx pixels of a segment that starts at pixel p0 of its frame, by NL lanes, kGroup pixels per lane at a time.  n: palette
// entries in use; exact: the palette is the sorted colours of the frame (FLAGS & kExact only); tab: bin -> median-cut box.
template <int FLAGS, int NL>
WU_HD void map_segment(const MapLds& M, int n, bool exact, const uint8_t* tab, const uint8_t* base, long long sy, long long sx, long long sc, int W,
                       int p0, int npx, uint8_t* idx, int lane) {
    const bool ranked = (FLAGS & kExact) && exact;
    for (int i0 = lane; i0 < npx; i0 += NL * kGroup) {
        int r[kGroup], g[kGroup], b[kGroup];
        uint32_t at[kGroup];
#pragma unroll
        for (int u = 0; u < kGroup; ++u) {
            const int i = i0 + NL * u;
            r[u] = g[u] = b[u] = 0;
            at[u] = 0u;
            if (i < npx) {
                const int p = p0 + i, y = p / W, x = p - y * W;
                const uint8_t* px = base + (long long)y * sy + (long long)x * sx;
                r[u] = px[0]; g[u] = px[sc]; b[u] = px[2 * sc];
                if (ranked) {
                    at[u] = exact_index(M, n, r[u], g[u], b[u]);
                } else {
                    at[u] = tab[((r[u] >> 3) << 10) | ((g[u] >> 3) << 5) | (b[u] >> 3)];
                    if (FLAGS & kDither) dither_colour(M, at[u], x, y, r[u], g[u], b[u]);
                }
            }
        }
        if ((FLAGS & kNearest) && !ranked) nearest_entries(M, n, r, g, b, at);
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
            if (i0 + NL * u < npx) idx[i0 + NL * u] = (uint8_t)at[u];
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

WU_HD uint32_t fixed_byte(int i, int h, int w, int delay_cs, const uint8_t* pal) {                  // pal == nullptr: no local colour table
    if (i >= 18) return pal && i < 18 + 768 ? pal[i - 18] : 8u;           // the colour table, then the minimum code size
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
        case 17: return pal ? 0x87u : 0u;                                 // local colour table of 256 entries
        default: return 0u;
    }
}

// Work item g of a frame's block: g < nchunk gathers payload bytes [16 g, 16 g + 16) with their sub-block length bytes; the fixed + 1 items
// behind write one fixed byte each, the last of them the terminator and the byte count.  fixed: kFixed with a local colour table `pal`,
// kFixedGlobal with pal == nullptr.
WU_HD void assemble_item(long long g, long long nchunk, const uint32_t* off, const uint32_t* slots, int nseg, const uint8_t* pal, int h, int w,
                         int delay_cs, uint8_t* out, int* result, int fixed = kFixed) {
    const uint32_t P = (off[nseg] + 7u) >> 3;
    if (g < nchunk) {
        const uint32_t j0 = (uint32_t)g * kChunk;
        if (j0 >= P) return;
        const uint32_t j1 = j0 + kChunk < P ? j0 + kChunk : P;
        int s = find_segment(off, nseg, 8u * j0);
        for (uint32_t j = j0; j < j1; ++j) {
            const size_t pos = (size_t)fixed + j + j / 255u + 1u;
            if (j % 255u == 0u) out[pos - 1] = (uint8_t)(P - j < 255u ? P - j : 255u);
            out[pos] = (uint8_t)payload_byte(off, slots, nseg, j, s);
        }
        return;
    }
    const long long i = g - nchunk;
    if (i < fixed) {
        out[i] = (uint8_t)fixed_byte((int)i, h, w, delay_cs, pal);
    } else if (i == fixed) {
        const size_t end = (size_t)fixed + P + (P + 254u) / 255u;
        out[end] = 0;
        *result = (int)(end + 1);
    }
}

struct Layout {
    size_t off_sums, off_cnt, off_set, off_table, off_pal, off_bounds, off_pinfo, off_len, off_off, off_slots, total;
    int npal;                                                              // palettes: T, or 1 under a global palette
};
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// Without `ex` (flags == 0) the layout of wu_gif_enc_encode as it always was; with it, the regions of the options in use and the palettes' info.
inline bool make_layout(int T, int h, int w, GifGeo& g, Layout& L, int flags = 0, bool ex = false) {
    if (T < 1 || T > 65535 || !gif_geo(h, w, g, flags)) return false;
    if ((flags & kGlobal) && (long long)T * g.npix > kMaxPixelsGlobal) return false;
    const size_t np = flags & kGlobal ? 1 : (size_t)T;
    L.npal = (int)np;
    size_t at = 0;
    L.off_sums = at;  at += np * 3 * kBins * sizeof(u64);                 // sums, counts and colour sets are one region: one memset
    L.off_cnt = at;   at = align256(at + np * kBins * sizeof(uint32_t));
    L.off_set = at;   at = align256(at + (flags & kExact ? np * (kSetSlots + 2) * sizeof(uint32_t) : 0));      // per palette: slots, entries, overflow
    L.off_table = at; at = align256(at + np * kBins);
    L.off_pal = at;   at = align256(at + np * 768);
    L.off_bounds = at; at = align256(at + (flags & kDither ? np * 256 * sizeof(uint32_t) : 0));
    L.off_pinfo = at; at = align256(at + (ex ? np * 2 * sizeof(int) : 0));
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

// SET: the distinct colours go into the colour set as well.  GLOBAL: all frames add to one histogram and one set.
template <bool SET, bool GLOBAL>
__global__ __launch_bounds__(256) void gif_hist_kernel(const uint8_t* __restrict__ frames, long long st, long long sy, long long sx, long long sc,
                                                       uint32_t* __restrict__ cnt, u64* __restrict__ sums, uint32_t* __restrict__ set, int H, int W) {
    const int t = blockIdx.y;
    const int npix = H * W;
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * kRun;
    if (!GLOBAL) {
        cnt += (size_t)t * kBins;
        sums += (size_t)t * 3 * kBins;
        if (SET) set += (size_t)t * (kSetSlots + 2);
    }
    int cur = -1;
    uint32_t last = 0xFFFFFFFFu;                                           // the colour of the pixel before: a run is inserted once
    bool live = SET && first < npix && mem_load(set + kSetSlots + 1) == 0u;
    uint32_t c = 0u, sr = 0u, sg = 0u, sb = 0u;
    if (first < npix) {
        const int p0 = (int)first, n = min(kRun, npix - p0);
        int y = p0 / W, x = p0 - y * W;
        const uint8_t* base = frames + (long long)t * st;
        for (int i = 0; i < n; ++i) {
            const uint8_t* px = base + (long long)y * sy + (long long)x * sx;
            const uint32_t r = px[0], g = px[sc], b = px[2 * sc];
            const int bin = (int)(((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3));
            if (SET) {
                const uint32_t colour = (r << 16) | (g << 8) | b;
                if (live && colour != last) set_insert(set, set + kSetSlots, colour, live);
                last = colour;
            }
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

// One workgroup per palette under the options: the sorted colours where the set holds at most 256 (no median cut then), else the median cut
// with its boxes' bounds.  set / bounds: nullptr without the exact / dither option.
__global__ __launch_bounds__(kMcThreads) void gif_palette_kernel(const uint32_t* __restrict__ cnt, const u64* __restrict__ sums,
                                                                  const uint32_t* __restrict__ set, uint8_t* __restrict__ table,
                                                                  uint8_t* __restrict__ pal, uint32_t* __restrict__ bounds, int* __restrict__ pinfo) {
    __shared__ McLds L;
    __shared__ ExLds E;
    const int t = blockIdx.x;
    if (set) {
        const uint32_t* s = set + (size_t)t * (kSetSlots + 2);
        if (s[kSetSlots] <= 256u && s[kSetSlots + 1] == 0u) {              // the same for the whole workgroup: the histogram kernel has ended
            exact_rank<kMcThreads>(s, pal + (size_t)t * 768, pinfo + 2 * t, E, threadIdx.x);
            return;
        }
    }
    median_cut<kMcThreads>(cnt + (size_t)t * kBins, sums + (size_t)t * 3 * kBins, table + (size_t)t * kBins, pal + (size_t)t * 768, L, threadIdx.x,
                           bounds ? bounds + (size_t)t * 256 : nullptr, pinfo + 2 * t);
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

// The same walk behind the map of the options (FLAGS: kNearest, kDither, kExact; the pixel's position is its position in the frame, so a
// segment that starts inside a row dithers like its neighbours).  pt: the frame's palette, 0 under a global one.
template <int FLAGS>
__global__ __launch_bounds__(64) void gif_lzw_map_kernel(const uint8_t* __restrict__ frames, long long st, long long sy, long long sx, long long sc,
                                                         const uint8_t* __restrict__ table, const uint8_t* __restrict__ pal,
                                                         const uint32_t* __restrict__ bounds, const int* __restrict__ pinfo, int per_frame,
                                                         uint32_t* __restrict__ slots, uint32_t* __restrict__ seglen, int H, int W, int nseg) {
    __shared__ alignas(16) LzwLds L;
    static_assert(sizeof(MapLds) <= sizeof(L.hash), "the palette of the map phase lives where the dictionary is built afterwards");
    MapLds& M = *reinterpret_cast<MapLds*>(L.hash);
    const int seg = blockIdx.x, t = blockIdx.y, lane = threadIdx.x, pt = t * per_frame;
    const int npix = H * W, p0 = seg * kSeg, npx = min(kSeg, npix - p0);
    const uint8_t* base = frames + (long long)t * st;
    const uint8_t* tab = table + (size_t)pt * kBins;
    const int n = pinfo[2 * pt];
    const bool exact = (FLAGS & kExact) && pinfo[2 * pt + 1] != 0;
    map_load(M, pal + (size_t)pt * 768, (FLAGS & kDither) && !exact ? bounds + (size_t)pt * 256 : nullptr, lane, 64);
    __syncthreads();
    map_segment<FLAGS, 64>(M, n, exact, tab, base, sy, sx, sc, W, p0, npx, (uint8_t*)L.idx, lane);
    __syncthreads();                                                       // the palette has been read: the dictionary takes its place
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
// Under the options: pal == nullptr under a global palette (no local table, `fixed` = kFixedGlobal); the item that writes the byte count also
// writes info[2 t] = palette entries in use, info[2 t + 1] = 1 where the frame took the exact path.
__global__ __launch_bounds__(256) void gif_assemble_ex_kernel(const uint32_t* __restrict__ off, const uint32_t* __restrict__ slots,
                                                              const uint8_t* __restrict__ pal, const int* __restrict__ pinfo, int per_frame,
                                                              uint8_t* __restrict__ out, long long out_stride, int* __restrict__ result,
                                                              int* __restrict__ info, long long nchunk, int nseg, int H, int W, int delay_cs,
                                                              int fixed) {
    const int t = blockIdx.y;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g > nchunk + fixed) return;
    assemble_item(g, nchunk, off + (size_t)t * (nseg + 1), slots + (size_t)t * nseg * kSlotWords, nseg, pal ? pal + (size_t)t * 768 : nullptr, H, W,
                  delay_cs, out + (size_t)t * out_stride, result + t, fixed);
    if (g == nchunk + fixed) {
        info[2 * t] = pinfo[2 * t * per_frame];
        info[2 * t + 1] = pinfo[2 * t * per_frame + 1];
    }
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

extern "C" size_t wu_gif_enc_workspace_bytes_ex(int T, int H, int W, int flags) {
    GifGeo g;
    Layout L;
    return make_layout(T, H, W, g, L, flags, true) ? L.total : 0;
}

extern "C" size_t wu_gif_enc_block_stride_ex(int H, int W, int flags) {
    GifGeo g;
    return gif_geo(H, W, g, flags) ? (size_t)g.stride : 0;
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
    hipLaunchKernelGGL((gif_hist_kernel<false, false>), dim3(hist_blocks, T), dim3(256), 0, s, frames, st, sy, sx, sc, cnt, sums, (uint32_t*)nullptr, H, W);
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

namespace {
template <int FLAGS>
void launch_lzw_map(hipStream_t s, dim3 grid, const uint8_t* frames, long long st, long long sy, long long sx, long long sc, const uint8_t* table,
                    const uint8_t* pal, const uint32_t* bounds, const int* pinfo, int per_frame, uint32_t* slots, uint32_t* seglen, int H, int W,
                    int nseg) {
    hipLaunchKernelGGL((gif_lzw_map_kernel<FLAGS>), grid, dim3(64), 0, s, frames, st, sy, sx, sc, table, pal, bounds, pinfo, per_frame, slots, seglen,
                       H, W, nseg);
}
}  // namespace

extern "C" int wu_gif_enc_encode_ex(const uint8_t* frames, long long st, long long sy, long long sx, long long sc, void* workspace,
                                    size_t workspace_bytes, uint8_t* out, size_t out_bytes, int* result_dev, int T, int H, int W, int delay_cs,
                                    int flags, uint8_t* palette_dev, int* info_dev, void* stream) {
    WU_REQUIRE(frames && workspace && out && result_dev && info_dev, "gif_enc_encode_ex: null argument");
    WU_REQUIRE((flags & ~kAllFlags) == 0 && (!(flags & kDither) || (flags & kNearest)),
               "gif_enc_encode_ex: bad flags %d (1 nearest, 2 ordered dither -- with nearest only --, 4 exact, 8 global palette)", flags);
    WU_REQUIRE(!(flags & kGlobal) || palette_dev, "gif_enc_encode_ex: a global palette needs palette_dev");
    GifGeo g;
    Layout L;
    WU_REQUIRE(make_layout(T, H, W, g, L, flags, true), "gif_enc_encode_ex: bad shape T=%d H=%d W=%d flags=%d", T, H, W, flags);
    WU_REQUIRE(st >= 0 && sy >= 0 && sx >= 0 && sc >= 0, "gif_enc_encode_ex: negative strides");
    WU_REQUIRE(delay_cs >= 0 && delay_cs <= 65535, "gif_enc_encode_ex: delay %d outside 0..65535", delay_cs);
    WU_REQUIRE(workspace_bytes >= L.total, "gif_enc_encode_ex: workspace too small (%zu of %zu bytes)", workspace_bytes, L.total);
    WU_REQUIRE(out_bytes >= (size_t)T * g.stride, "gif_enc_encode_ex: output too small (%zu of %zu bytes)", out_bytes, (size_t)T * (size_t)g.stride);
    WU_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)result_dev & 3) == 0 && ((uintptr_t)info_dev & 3) == 0,
               "gif_enc_encode_ex: workspace must be 256-byte aligned, results and info naturally aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    u64* sums = (u64*)(ws + L.off_sums);
    uint32_t* cnt = (uint32_t*)(ws + L.off_cnt);
    uint32_t* set = flags & kExact ? (uint32_t*)(ws + L.off_set) : nullptr;
    uint8_t* table = ws + L.off_table;
    uint8_t* pal = flags & kGlobal ? palette_dev : ws + L.off_pal;
    uint32_t* bounds = flags & kDither ? (uint32_t*)(ws + L.off_bounds) : nullptr;
    int* pinfo = (int*)(ws + L.off_pinfo);
    uint32_t* seglen = (uint32_t*)(ws + L.off_len);
    uint32_t* off = (uint32_t*)(ws + L.off_off);
    uint32_t* slots = (uint32_t*)(ws + L.off_slots);
    const int per_frame = flags & kGlobal ? 0 : 1;
    const hipError_t e = hipMemsetAsync(ws + L.off_sums, 0, L.off_table - L.off_sums, s);
    if (e != hipSuccess) WU_FAIL((int)e, "gif_enc_encode_ex: memset: %s", hipGetErrorString(e));
    const dim3 hist_grid((unsigned)((g.npix + 256ll * kRun - 1) / (256ll * kRun)), T);
#define WU_GIF_HIST(SET, GLOBAL) \
    hipLaunchKernelGGL((gif_hist_kernel<SET, GLOBAL>), hist_grid, dim3(256), 0, s, frames, st, sy, sx, sc, cnt, sums, set, H, W)
    if (flags & kExact) { if (flags & kGlobal) WU_GIF_HIST(true, true); else WU_GIF_HIST(true, false); }
    else { if (flags & kGlobal) WU_GIF_HIST(false, true); else WU_GIF_HIST(false, false); }
#undef WU_GIF_HIST
    WU_LAUNCH_CHECK("gif_hist_kernel");
    hipLaunchKernelGGL(gif_palette_kernel, dim3(L.npal), dim3(kMcThreads), 0, s, cnt, sums, set, table, pal, bounds, pinfo);
    WU_LAUNCH_CHECK("gif_palette_kernel");
    const dim3 lzw_grid((unsigned)g.nseg, T);
    switch (flags & (kNearest | kDither | kExact)) {
#define WU_GIF_LZW(F) \
        case F: launch_lzw_map<F>(s, lzw_grid, frames, st, sy, sx, sc, table, pal, bounds, pinfo, per_frame, slots, seglen, H, W, g.nseg); break;
        WU_GIF_LZW(0)
        WU_GIF_LZW(kNearest)
        WU_GIF_LZW(kNearest | kDither)
        WU_GIF_LZW(kExact)
        WU_GIF_LZW(kExact | kNearest)
        WU_GIF_LZW(kExact | kNearest | kDither)
#undef WU_GIF_LZW
        default: WU_FAIL(-1, "gif_enc_encode_ex: bad flags %d", flags);
    }
    WU_LAUNCH_CHECK("gif_lzw_map_kernel");
    hipLaunchKernelGGL(gif_scan_kernel, dim3(T), dim3(256), 0, s, seglen, off, g.nseg);
    WU_LAUNCH_CHECK("gif_scan_kernel");
    const long long nchunk = (g.pmax + kChunk - 1) / kChunk;
    const unsigned asm_blocks = (unsigned)((nchunk + g.fixed + 1 + 255) / 256);
    hipLaunchKernelGGL(gif_assemble_ex_kernel, dim3(asm_blocks, T), dim3(256), 0, s, off, slots, flags & kGlobal ? (const uint8_t*)nullptr : pal,
                       pinfo, per_frame, out, g.stride, result_dev, info_dev, nchunk, g.nseg, H, W, delay_cs, g.fixed);
    WU_LAUNCH_CHECK("gif_assemble_ex_kernel");
    return 0;
}
#endif
