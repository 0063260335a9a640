// Stand-alone CPU emulation of the two PNG decoder kernels (csrc/png_dec.hip) under the shim scratch/png_dec_emu.h: 64 independent host
// threads per workgroup, __syncthreads() the only ordering between them, LDS poisoned before every workgroup.  Built by
// scratch/png_dec_emu_build.sh once with -fsanitize=address,undefined and once with -fsanitize=thread; CPU only, no HIP runtime.
//
//   png_dec_emu [--batch K] [--fuzz M] DIR      every DIR/NAME.png with its DIR/NAME.want (scratch/png_dec_emu_fixtures.py writes both)
//
// NAME.want: int32 status -- 0 and then int32 h, int32 w, h*w*3 pixel bytes; or the device status the restatement gives.  Every file is
// decoded alone, then all of them again K at a time in one batch (default 5), so corrupt files sit next to good ones of other sizes.  Every
// buffer is a heap block of EXACTLY its size, poisoned.  --fuzz M: every file M more times with one byte of an IDAT body replaced and the
// chunk's CRC made right again, so that the damage reaches the inflate: any status may come out, but a rejected slot must be all zeros and
// no sanitizer may speak.  Exit status 1 if a status, a pixel or a padding byte is wrong.
#include "png_dec.hip"

#include <dirent.h>

#include <string>

extern "C" const char* wu_last_error(void) { return g_wu_err; }

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

struct Item {
    std::string name;
    std::vector<uint8_t> file, want;
};

constexpr int kAnyStatus = -100;     // a fuzzed file: whatever the decoder says, as long as a rejected slot is zero
static int want_status(const Item& it) { int s; memcpy(&s, it.want.data(), 4); return s; }

static int run_batch(const std::vector<const Item*>& items, int* hist = nullptr) {
    const int N = (int)items.size();
    std::vector<PngDecDesc> desc(N);
    std::vector<PngDecSeg> segs;
    std::vector<uint8_t> src;
    int Hmax = 1, Wmax = 1;
    for (int i = 0; i < N; ++i) {
        const Item& it = *items[i];
        wu_png_dec_info info;
        std::vector<long long> idat(2 * 4096);
        wu_png_dec_parse(it.file.data(), it.file.size(), 89478485, &info, idat.data(), 4096);
        memset(&desc[i], 0, sizeof(PngDecDesc));
        if (!info.supported) { printf("  %s: refused by the parser (%d)\n", it.name.c_str(), info.reason); return 1; }
        while (src.size() % 16) src.push_back(0xA5);
        desc[i].src_off = (long long)src.size();
        desc[i].file_bytes = (int)it.file.size();
        desc[i].h = info.height;
        desc[i].w = info.width;
        desc[i].first_seg = (int)segs.size();
        desc[i].nseg = info.n_segments;
        src.insert(src.end(), it.file.begin(), it.file.end());
        for (int k = 0; k < info.n_segments; ++k) segs.push_back(PngDecSeg{i, k, (uint32_t)idat[2 * k], (uint32_t)idat[2 * k + 1]});
        Hmax = std::max(Hmax, info.height);
        Wmax = std::max(Wmax, info.width);
    }
    const int nseg = (int)segs.size();
    const size_t wsb = wu_png_dec_workspace_bytes(N, Hmax, Wmax, nseg);
    if (!wsb) { printf("  no workspace size\n"); return 1; }
    uint8_t* ws = (uint8_t*)aligned_alloc(256, wsb);
    memset(ws, 0xCC, wsb);
    const size_t outb = (size_t)N * Hmax * Wmax * 3;
    uint8_t* out = (uint8_t*)malloc(outb);
    memset(out, 0x77, outb);
    int* status = (int*)malloc(sizeof(int) * N);
    for (int i = 0; i < N; ++i) status[i] = -1;
    uint8_t* srcp = (uint8_t*)malloc(src.size());
    memcpy(srcp, src.data(), src.size());
    PngDecDesc* descp = (PngDecDesc*)malloc(sizeof(PngDecDesc) * N);
    memcpy(descp, desc.data(), sizeof(PngDecDesc) * N);
    PngDecSeg* segp = (PngDecSeg*)malloc(sizeof(PngDecSeg) * nseg);
    memcpy(segp, segs.data(), sizeof(PngDecSeg) * nseg);
    const int rc = wu_png_dec_decode(srcp, src.size(), descp, sizeof(PngDecDesc) * N, segp, sizeof(PngDecSeg) * nseg, nseg, ws, wsb, out, outb,
                                     status, sizeof(int) * N, N, Hmax, Wmax, nullptr);
    int fails = 0;
    if (rc) { printf("  decode rc %d: %s\n", rc, g_wu_err); fails = 1; }
    for (int i = 0; i < N && !rc; ++i) {
        const Item& it = *items[i];
        const int want = want_status(it);
        const uint8_t* slot = out + (size_t)i * Hmax * Wmax * 3;
        const int h = desc[i].h, w = desc[i].w;
        long long bad = 0, padbad = 0;
        const uint8_t* px = it.want.data() + 12;
        if (want == 0) {
            int wh, ww;
            memcpy(&wh, it.want.data() + 4, 4);
            memcpy(&ww, it.want.data() + 8, 4);
            if (wh != h || ww != w || it.want.size() != 12 + (size_t)h * w * 3) { printf("  %s: .want does not fit\n", it.name.c_str()); ++fails; continue; }
        }
        for (int y = 0; y < Hmax; ++y)
            for (int x = 0; x < Wmax; ++x)
                for (int c = 0; c < 3; ++c) {
                    const uint8_t v = slot[((size_t)y * Wmax + x) * 3 + c];
                    if (status[i] == 0 && y < h && x < w) bad += want == 0 && v != px[((size_t)y * w + x) * 3 + c];
                    else padbad += v != 0;
                }
        const bool ok = (status[i] == want || (want == kAnyStatus && status[i] >= 0 && status[i] <= 6)) && !bad && !padbad;
        if (hist && status[i] >= 0 && status[i] <= 6) ++hist[status[i]];
        if (!ok || (N == 1 && !hist))
            printf("  %s: status %d (want %d), %d x %d, pixel diffs %lld, nonzero padding %lld%s\n", it.name.c_str(), status[i], want, h, w, bad,
                   padbad, ok ? "" : "   <-- WRONG");
        fails += !ok;
    }
    free(segp); free(descp); free(srcp); free(status); free(out); free(ws);
    return fails;
}

int main(int argc, char** argv) {
    int batch = 5, fuzz = 0, at = 1;
    while (at + 1 < argc && argv[at][0] == '-') {
        if (!strcmp(argv[at], "--batch")) batch = atoi(argv[at + 1]);
        else if (!strcmp(argv[at], "--fuzz")) fuzz = atoi(argv[at + 1]);
        at += 2;
    }
    if (at >= argc) { fprintf(stderr, "usage: png_dec_emu [--batch K] [--fuzz M] DIR\n"); return 2; }
    const std::string dir = argv[at];
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".png") names.push_back(n.substr(0, n.size() - 4));
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    std::vector<Item> items;
    for (const auto& n : names) {
        Item it{n, slurp(dir + "/" + n + ".png"), slurp(dir + "/" + n + ".want")};
        if (it.want.size() < 4) { fprintf(stderr, "%s: no .want\n", n.c_str()); return 2; }
        items.push_back(std::move(it));
    }
    if (items.empty()) { fprintf(stderr, "no fixtures in %s\n", dir.c_str()); return 2; }
    int fails = 0;
    printf("each file alone:\n");
    for (const auto& it : items) fails += run_batch({&it});
    if (batch > 1) {
        printf("batches of %d:\n", batch);
        // neighbours in a batch differ in kind: stride through the sorted list
        const size_t n = items.size(), stride = n / (size_t)batch + 1;
        for (size_t b = 0; b < stride; ++b) {
            std::vector<const Item*> group;
            for (size_t i = b; i < n; i += stride) group.push_back(&items[i]);
            if (!group.empty()) fails += run_batch(group);
        }
    }
    if (fuzz > 0) {
        printf("%d damaged copies of each file:\n", fuzz);
        uint64_t rng = 0x9E3779B97F4A7C15ull;
        int hist[7] = {0};
        for (const auto& it : items) {
            wu_png_dec_info info;
            std::vector<long long> idat(2 * 4096);
            wu_png_dec_parse(it.file.data(), it.file.size(), 89478485, &info, idat.data(), 4096);
            for (int m = 0; m < fuzz && info.supported; ++m) {
                Item bad{it.name + " (damaged)", it.file, std::vector<uint8_t>(4)};
                const int any = kAnyStatus;
                memcpy(bad.want.data(), &any, 4);
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                const int k = (int)((rng >> 33) % (uint64_t)info.n_idat);
                const long long off = idat[2 * k], len = idat[2 * k + 1];
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                const long long pos = off + (k == 0 ? 2 : 0) + (long long)((rng >> 33) % (uint64_t)std::max(1ll, len - (k == 0 ? 2 : 0)));
                if (pos >= off + len) continue;
                bad.file[(size_t)pos] = (uint8_t)(rng >> 24);
                const uint32_t c = host_crc(bad.file.data() + off - 4, (size_t)len + 4);
                for (int j = 0; j < 4; ++j) bad.file[(size_t)(off + len) + j] = (uint8_t)(c >> (24 - 8 * j));
                fails += run_batch({&bad}, hist);
            }
        }
        printf("  statuses 0..6:");
        for (int h : hist) printf(" %d", h);
        printf("\n");
    }
    printf("%zu files, %d wrong\n", items.size(), fails);
    return fails ? 1 : 0;
}
