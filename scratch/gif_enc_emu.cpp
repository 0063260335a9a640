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

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: gif_enc_emu DIR\n"); return 2; }
    const std::string dir = argv[1];
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
