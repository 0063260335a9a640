// Stand-alone CPU run of the GIF encoder's device functions (csrc/gif_enc.hip compiled as host C++ under WU_GIF_ENC_EMU): the median cut,
// the LZW walk of a segment and the gather that assembles a block, single-threaded (one "thread" owns every bin, one "lane" walks), so it
// checks their arithmetic and every index they form, not their barriers.  The histogram, the pixel -> index map and the scan of the bit
// lengths are three-line loops here; on the device they are kernels of their own.  CPU only: no GPU, no HIP runtime, nothing loaded into
// an interpreter.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include scratch/gif_enc_emu.cpp -o gif_enc_emu
//   python -c "import sys; sys.path.insert(0, 'tests'); import _gif_enc_cases as C; print(C.dump('DIR'))"
//   ./gif_enc_emu DIR
//
// DIR/NAME.in: int32 T, h, w, delay_cs, then the frames; DIR/NAME.want: per frame int32 n and the n bytes of the restatement's image block
// (tests/_gif_enc_cases.py dump()).  Every buffer is a heap block of EXACTLY the size the library's own layout gives it, poisoned, the
// "LDS" structs included.  Exit status 1 if a byte differs.
//
// The quality options (wu_gif_enc_encode_ex: exact palettes, nearest-colour mapping, ordered dither, a global palette) run the same way over
// their own cases: the colour set's insert, the rank, the palette load, the pixel map and the gather without a local table, against the
// palette, the info and the blocks of tests/_gif_quality_ref.py.
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import _gif_quality_cases as C; print(C.dump('QDIR'))"
//   ./gif_enc_emu --quality QDIR
//
// QDIR/NAME.OPTIONS.in: int32 T, h, w, delay_cs, flags, then the frames; QDIR/NAME.OPTIONS.want: the 768 bytes of the global palette (zeros
// under local ones), then per frame int32 entries, exact, n and the n bytes of the block (tests/_gif_quality_cases.py dump()).
#define WU_GIF_ENC_EMU 1
#include "../weather-unet_amd/csrc/gif_enc.hip"

#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

static std::vector<uint8_t> slurp(const std::string& p) {
    std::vector<uint8_t> b;
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return b;
    uint8_t t[4096];
    size_t g;
    while ((g = fread(t, 1, sizeof(t), f)) > 0) b.insert(b.end(), t, t + g);
    fclose(f);
    return b;
}

template <typename T> static T* poisoned(size_t n) {
    T* p = (T*)malloc(n * sizeof(T));
    memset(p, 0xA5, n * sizeof(T));
    return p;
}

// One frame through the device functions; returns the block's byte count, the block in `out` (wu_gif_enc_block_stride bytes).
static int encode_frame(const uint8_t* px, int h, int w, int delay_cs, uint8_t* out, const GifGeo& g) {
    uint32_t* cnt = (uint32_t*)calloc(kBins, sizeof(uint32_t));
    u64* sums = (u64*)calloc(3 * kBins, sizeof(u64));
    for (long long p = 0; p < g.npix; ++p) {
        const uint32_t r = px[3 * p], gr = px[3 * p + 1], b = px[3 * p + 2];
        const uint32_t bin = ((r >> 3) << 10) | ((gr >> 3) << 5) | (b >> 3);
        ++cnt[bin];
        sums[bin] += r; sums[kBins + bin] += gr; sums[2 * kBins + bin] += b;
    }
    uint8_t* table = poisoned<uint8_t>(kBins);
    uint8_t* pal = poisoned<uint8_t>(768);
    McLds* mc = poisoned<McLds>(1);
    median_cut<1>(cnt, sums, table, pal, *mc, 0);
    uint32_t* slots = poisoned<uint32_t>((size_t)g.nseg * kSlotWords);
    uint32_t* off = poisoned<uint32_t>((size_t)g.nseg + 1);
    LzwLds* lz = poisoned<LzwLds>(1);
    off[0] = 0;
    for (int s = 0; s < g.nseg; ++s) {
        const long long p0 = (long long)s * kSeg;
        const int npx = (int)std::min<long long>(kSeg, g.npix - p0);
        memset(lz, 0xA5, sizeof(LzwLds));
        uint8_t* idx = (uint8_t*)lz->idx;
        for (int i = 0; i < npx; ++i) {
            const uint8_t* q = px + 3 * (p0 + i);
            idx[i] = table[((q[0] >> 3) << 10) | ((q[1] >> 3) << 5) | (q[2] >> 3)];
        }
        off[s + 1] = off[s] + lzw_segment<1>(*lz, npx, s == 0, s == g.nseg - 1, slots + (size_t)s * kSlotWords, 0);
    }
    int result = -1;
    const long long nchunk = (g.pmax + kChunk - 1) / kChunk;
    for (long long item = 0; item <= nchunk + kFixed; ++item) assemble_item(item, nchunk, off, slots, g.nseg, pal, h, w, delay_cs, out, &result);
    free(lz); free(off); free(slots); free(mc); free(pal); free(table); free(sums); free(cnt);
    return result;
}

// One palette group (all T frames under a global palette, else one frame) through the device functions of the options; frame t's block goes
// to out + t * stride, its byte count to result[t]; pal (768) and info (2) describe the group's palette.
static void encode_group_ex(const uint8_t* px, int nt, int h, int w, int delay_cs, int flags, uint8_t* out, int* result, uint8_t* pal, int* pinfo,
                            const GifGeo& g) {
    uint32_t* cnt = (uint32_t*)calloc(kBins, sizeof(uint32_t));
    u64* sums = (u64*)calloc(3 * kBins, sizeof(u64));
    uint32_t* set = (uint32_t*)calloc(kSetSlots + 2, sizeof(uint32_t));
    bool live = true;
    for (long long p = 0; p < g.npix * nt; ++p) {
        const uint32_t r = px[3 * p], gr = px[3 * p + 1], b = px[3 * p + 2];
        const uint32_t bin = ((r >> 3) << 10) | ((gr >> 3) << 5) | (b >> 3);
        ++cnt[bin];
        sums[bin] += r; sums[kBins + bin] += gr; sums[2 * kBins + bin] += b;
        if ((flags & kExact) && live) set_insert(set, set + kSetSlots, (r << 16) | (gr << 8) | b, live);
    }
    uint8_t* table = poisoned<uint8_t>(kBins);
    uint32_t* bounds = poisoned<uint32_t>(256);
    McLds* mc = poisoned<McLds>(1);
    ExLds* ex = poisoned<ExLds>(1);
    if ((flags & kExact) && set[kSetSlots] <= 256u && set[kSetSlots + 1] == 0u) exact_rank<1>(set, pal, pinfo, *ex, 0);
    else median_cut<1>(cnt, sums, table, pal, *mc, 0, flags & kDither ? bounds : nullptr, pinfo);
    const bool exact = (flags & kExact) && pinfo[1] != 0;
    MapLds* mp = poisoned<MapLds>(1);
    map_load(*mp, pal, (flags & kDither) && !exact ? bounds : nullptr, 0, 1);
    for (int t = 0; t < nt; ++t) {
        const uint8_t* fpx = px + (size_t)t * g.npix * 3;
        uint32_t* slots = poisoned<uint32_t>((size_t)g.nseg * kSlotWords);
        uint32_t* off = poisoned<uint32_t>((size_t)g.nseg + 1);
        LzwLds* lz = poisoned<LzwLds>(1);
        off[0] = 0;
        for (int s = 0; s < g.nseg; ++s) {
            const long long p0 = (long long)s * kSeg;
            const int npx = (int)std::min<long long>(kSeg, g.npix - p0);
            memset(lz, 0xA5, sizeof(LzwLds));
            uint8_t* idx = (uint8_t*)lz->idx;
            switch (flags & (kNearest | kDither | kExact)) {
                case 0: map_segment<0, 1>(*mp, pinfo[0], exact, table, fpx, 3ll * w, 3, 1, w, (int)p0, npx, idx, 0); break;
                case kNearest: map_segment<kNearest, 1>(*mp, pinfo[0], exact, table, fpx, 3ll * w, 3, 1, w, (int)p0, npx, idx, 0); break;
                case kNearest | kDither: map_segment<kNearest | kDither, 1>(*mp, pinfo[0], exact, table, fpx, 3ll * w, 3, 1, w, (int)p0, npx, idx, 0); break;
                case kExact: map_segment<kExact, 1>(*mp, pinfo[0], exact, table, fpx, 3ll * w, 3, 1, w, (int)p0, npx, idx, 0); break;
                case kExact | kNearest: map_segment<kExact | kNearest, 1>(*mp, pinfo[0], exact, table, fpx, 3ll * w, 3, 1, w, (int)p0, npx, idx, 0); break;
                default: map_segment<kExact | kNearest | kDither, 1>(*mp, pinfo[0], exact, table, fpx, 3ll * w, 3, 1, w, (int)p0, npx, idx, 0); break;
            }
            off[s + 1] = off[s] + lzw_segment<1>(*lz, npx, s == 0, s == g.nseg - 1, slots + (size_t)s * kSlotWords, 0);
        }
        result[t] = -1;
        const long long nchunk = (g.pmax + kChunk - 1) / kChunk;
        for (long long item = 0; item <= nchunk + g.fixed; ++item)
            assemble_item(item, nchunk, off, slots, g.nseg, flags & kGlobal ? nullptr : pal, h, w, delay_cs, out + (size_t)t * g.stride, result + t, g.fixed);
        free(lz); free(off); free(slots);
    }
    free(mp); free(ex); free(mc); free(bounds); free(table); free(set); free(sums); free(cnt);
}

static int quality_main(const std::string& dir, const std::vector<std::string>& names) {
    int fails = 0, blocks = 0;
    for (const auto& name : names) {
        const std::vector<uint8_t> in = slurp(dir + "/" + name + ".in"), want = slurp(dir + "/" + name + ".want");
        int hd[5];
        if (in.size() < 20) { fprintf(stderr, "%s: no header\n", name.c_str()); return 2; }
        memcpy(hd, in.data(), 20);
        const int T = hd[0], h = hd[1], w = hd[2], delay = hd[3], flags = hd[4];
        GifGeo g;
        if (!gif_geo(h, w, g, flags) || in.size() != 20 + (size_t)T * g.npix * 3) { fprintf(stderr, "%s: bad input file\n", name.c_str()); return 2; }
        if (wu_gif_enc_block_stride_ex(h, w, flags) != (size_t)g.stride || wu_gif_enc_workspace_bytes_ex(T, h, w, flags) == 0) {
            fprintf(stderr, "%s: sizes\n", name.c_str());
            return 2;
        }
        uint8_t* out = poisoned<uint8_t>((size_t)T * g.stride);
        uint8_t* pal = poisoned<uint8_t>(768);
        std::vector<int> result(T), info(2 * T);
        const bool global = flags & kGlobal;
        if (global) {
            int pinfo[2];
            encode_group_ex(in.data() + 20, T, h, w, delay, flags, out, result.data(), pal, pinfo, g);
            for (int t = 0; t < T; ++t) { info[2 * t] = pinfo[0]; info[2 * t + 1] = pinfo[1]; }
        } else {
            for (int t = 0; t < T; ++t)
                encode_group_ex(in.data() + 20 + (size_t)t * g.npix * 3, 1, h, w, delay, flags, out + (size_t)t * g.stride, result.data() + t, pal,
                                info.data() + 2 * t, g);
        }
        size_t at = 768;
        bool pal_ok = want.size() >= 768 && (!global || memcmp(pal, want.data(), 768) == 0);
        if (!pal_ok) { printf("  %s: global palette   <-- WRONG\n", name.c_str()); ++fails; }
        for (int t = 0; t < T; ++t) {
            int wv[3] = {-1, -1, -1};
            if (at + 12 <= want.size()) memcpy(wv, want.data() + at, 12);
            at += 12;
            const int n = result[t], wn = wv[2];
            bool ok = n == wn && n > 0 && (long long)n <= g.stride && at + (size_t)n <= want.size() && info[2 * t] == wv[0] && info[2 * t + 1] == wv[1];
            size_t diff = 0;
            if (ok) {
                while (diff < (size_t)n && out[(size_t)t * g.stride + diff] == want[at + diff]) ++diff;
                ok = diff == (size_t)n;
            }
            printf("  %s frame %d: %d x %d flags %d, entries %d (want %d) exact %d (want %d), block %d bytes (want %d, bound %lld)%s\n", name.c_str(), t, h,
                   w, flags, info[2 * t], wv[0], info[2 * t + 1], wv[1], n, wn, g.stride, ok ? "" : "   <-- WRONG");
            if (!ok && n == wn) printf("    first difference at byte %zu\n", diff);
            fails += !ok;
            ++blocks;
            at += wn > 0 ? (size_t)wn : 0;
        }
        free(pal); free(out);
    }
    printf("%zu cases, %d blocks, %d wrong\n", names.size(), blocks, fails);
    return fails ? 1 : 0;
}

int main(int argc, char** argv) {
    const bool quality = argc >= 3 && std::string(argv[1]) == "--quality";
    if (argc < 2 || (argc >= 3 && !quality)) { fprintf(stderr, "usage: gif_enc_emu DIR | gif_enc_emu --quality QDIR\n"); return 2; }
    const std::string dir = argv[quality ? 2 : 1];
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 3 && n.substr(n.size() - 3) == ".in") names.push_back(n.substr(0, n.size() - 3));
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    if (names.empty()) { fprintf(stderr, "no cases in %s\n", dir.c_str()); return 2; }
    if (quality) return quality_main(dir, names);
    int fails = 0, blocks = 0;
    for (const auto& name : names) {
        const std::vector<uint8_t> in = slurp(dir + "/" + name + ".in"), want = slurp(dir + "/" + name + ".want");
        int hd[4];
        if (in.size() < 16) { fprintf(stderr, "%s: no header\n", name.c_str()); return 2; }
        memcpy(hd, in.data(), 16);
        const int T = hd[0], h = hd[1], w = hd[2], delay = hd[3];
        GifGeo g;
        if (!gif_geo(h, w, g) || in.size() != 16 + (size_t)T * g.npix * 3) { fprintf(stderr, "%s: bad input file\n", name.c_str()); return 2; }
        if (wu_gif_enc_block_stride(h, w) != (size_t)g.stride || wu_gif_enc_workspace_bytes(T, h, w) == 0) { fprintf(stderr, "%s: sizes\n", name.c_str()); return 2; }
        size_t at = 0;
        for (int t = 0; t < T; ++t) {
            uint8_t* out = poisoned<uint8_t>((size_t)g.stride);
            const int n = encode_frame(in.data() + 16 + (size_t)t * g.npix * 3, h, w, delay, out, g);
            int wn = -1;
            if (at + 4 <= want.size()) memcpy(&wn, want.data() + at, 4);
            at += 4;
            bool ok = n == wn && n > 0 && (long long)n <= g.stride && at + (size_t)n <= want.size();
            size_t diff = 0;
            if (ok) {
                while (diff < (size_t)n && out[diff] == want[at + diff]) ++diff;
                ok = diff == (size_t)n;
            }
            printf("  %s frame %d: %d x %d, %d segments, block %d bytes (want %d, bound %lld)%s\n", name.c_str(), t, h, w, g.nseg, n, wn, g.stride,
                   ok ? "" : "   <-- WRONG");
            if (!ok && n == wn) printf("    first difference at byte %zu\n", diff);
            fails += !ok;
            ++blocks;
            at += wn > 0 ? (size_t)wn : 0;
            free(out);
        }
    }
    printf("%zu cases, %d blocks, %d wrong\n", names.size(), blocks, fails);
    return fails ? 1 : 0;
}
