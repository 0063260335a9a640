// Stand-alone CPU emulation of the device Huffman decoder (csrc/jpeg_huff.hip) under the shim scratch/jpeg_huff_emu.h: 256 independent
// host threads per workgroup, __syncthreads() the only ordering between them, LDS poisoned before every workgroup.  Built by
// scratch/jpeg_huff_emu_build.sh once with -fsanitize=address,undefined and once with -fsanitize=thread; CPU only, no HIP runtime.
// The reference is the host decoder of csrc/jpeg.hip (wu_jpeg_entropy_decode), compiled into the same program.
//
//   jpeg_huff_emu [--batch K] [--fuzz M] [--subseq "64 128 1024"] DIR        every DIR/*.jpg
//
// Every file the parser supports is staged and decoded alone at every subsequence size, then all of them K at a time in one call
// (default 5) at the first size.  Every buffer is a heap block of EXACTLY its size; the coefficient buffer has 32 guard blocks of 0x7777
// in front of, between and behind the images.  Asked of every stream:
//   host accepts (0 / 1 = over the magnitude bound)  ->  status 0 / WU_JPEG_MAGNITUDE and blocks and tables equal the host's
//   status 0                                         ->  the host accepts, or refuses ONLY the restart sequence (-3: fewer than 64 junk
//                                                        bits in front of RSTn, which its prefetch may or may not have stepped over)
//   host refuses                                     ->  the staging refuses too, or the status is not 0 (exception as above)
//   guards intact, no sanitizer report.
// --fuzz M: every file M more times with one bit of its entropy-coded data flipped and M more times cut short inside it.
// Exit status 1 if anything is wrong.
#include "jpeg.hip"
#include "jpeg_huff.hip"

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
    std::vector<uint8_t> file;
};

static long long g_streams, g_lenient, g_rejected, g_magnitude, g_stage_refused, g_max_rounds_barriers;
constexpr int kGuard = 32;

// exact-size heap copies: an access one byte past any of them is a report
template <typename T> static T* exact(const T* src, size_t count) {
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);            // malloc's blocks are 16-byte aligned, as the ABI asks
    if (count) memcpy(p, src, count * sizeof(T));
    return p;
}

static int run_batch(const std::vector<const Item*>& items, int S, bool verbose) {
    struct Staged {
        wu_jpeg_info info;
        int rc_host;
        std::vector<int16_t> want;
        uint16_t qwant[192];
        std::vector<uint8_t> scan;
        std::vector<int> segs;
        uint8_t dht[kDhtImage];
        uint16_t qtab[192];
        wu_jpeg_scan res;
        bool on_device;
    };
    const int N = (int)items.size();
    std::vector<Staged> st((size_t)N);
    int fails = 0;
    std::vector<uint8_t> scan_all;
    std::vector<int> seg_all;
    std::vector<HuffDesc> hd((size_t)N);
    std::vector<uint8_t> dht_all((size_t)N * kDhtImage, 0);
    std::vector<uint16_t> qtab_all((size_t)N * 192, 1);
    long long blocks = kGuard;
    for (int i = 0; i < N; ++i) {
        const Item& it = *items[i];
        Staged& s = st[i];
        s.on_device = false;
        memset(&hd[i], 0, sizeof(HuffDesc));
        wu_jpeg_parse(it.file.data(), it.file.size(), &s.info);
        if (!s.info.supported) continue;
        s.want.assign((size_t)s.info.total_blocks * 64, 0);
        wu_jpeg_info copy = s.info;
        uint8_t* fcopy = exact(it.file.data(), it.file.size());      // the file itself at its exact size, for the host functions
        s.rc_host = wu_jpeg_entropy_decode(fcopy, it.file.size(), &copy, s.want.data(), s.want.size() * 2, s.qwant);
        const size_t bound = wu_jpeg_scan_stage_bytes(&s.info, it.file.size(), S);
        const int nseg = wu_jpeg_scan_segments(&s.info);
        if (!bound || nseg <= 0) { printf("  %s: no staging bound\n", it.name.c_str()); free(fcopy); ++fails; continue; }
        uint8_t* scan = (uint8_t*)malloc(bound);
        int* segs = (int*)malloc((size_t)nseg * 16);
        memset(scan, 0xEE, bound);
        const int rc = wu_jpeg_scan_stage(fcopy, it.file.size(), &s.info, S, scan, bound, segs, (size_t)nseg * 16, s.dht, s.qtab, &s.res);
        free(fcopy);
        ++g_streams;
        if (rc < 0) {
            ++g_stage_refused;
            if (s.rc_host >= 0) { printf("  %s: staging refused (%d: %s) what the host decodes\n", it.name.c_str(), rc, g_wu_err); ++fails; }
            free(scan); free(segs);
            continue;
        }
        if ((size_t)s.res.scan_bytes > bound || s.res.n_segments != nseg) { printf("  %s: staging result outside its bound\n", it.name.c_str()); ++fails; }
        s.on_device = true;
        while (scan_all.size() % 16) scan_all.push_back(0xEE);
        hd[i].scan_off = (int)scan_all.size();
        hd[i].scan_bytes = s.res.scan_bytes;
        hd[i].first_seg = (int)seg_all.size() / 4;
        hd[i].nseg = nseg;
        hd[i].nsub = s.res.n_subseq;
        hd[i].first_block = (int)blocks;
        hd[i].nblocks = s.info.total_blocks;
        hd[i].ncomp = s.info.ncomp;
        hd[i].hs0 = s.info.hs[0];
        hd[i].vs0 = s.info.vs[0];
        hd[i].mcus_x = s.info.mcus_x;
        hd[i].total_mcus = s.info.mcus_x * s.info.mcus_y;
        hd[i].restart_interval = s.info.restart_interval;
        blocks += s.info.total_blocks + kGuard;
        scan_all.insert(scan_all.end(), scan, scan + s.res.scan_bytes);
        seg_all.insert(seg_all.end(), segs, segs + 4 * nseg);
        memcpy(&dht_all[(size_t)i * kDhtImage], s.dht, kDhtImage);
        memcpy(&qtab_all[(size_t)i * 192], s.qtab, 384);
        free(scan); free(segs);
    }
    uint8_t* scan_dev = exact(scan_all.data(), scan_all.size());
    int* seg_dev = exact(seg_all.data(), seg_all.size());
    uint8_t* dht_dev = exact(dht_all.data(), dht_all.size());
    uint16_t* qtab_dev = exact(qtab_all.data(), qtab_all.size());
    HuffDesc* hd_dev = exact(hd.data(), hd.size());
    std::vector<int16_t> fill((size_t)blocks * 64, 0x7777);
    int16_t* coef = exact(fill.data(), fill.size());
    std::vector<int> minus((size_t)N, -1);
    int* status = exact(minus.data(), minus.size());
    const long long b0 = g_emu_barriers;
    const int rc = wu_jpeg_huff_decode(scan_dev, seg_dev, dht_dev, hd_dev, qtab_dev, coef, status, N, S, nullptr);
    g_max_rounds_barriers = std::max(g_max_rounds_barriers, g_emu_barriers - b0);
    if (rc) { printf("  decode rc %d: %s\n", rc, g_wu_err); ++fails; }
    // guards: everything outside the images' own blocks
    std::vector<char> owned((size_t)blocks, 0);
    for (int i = 0; i < N; ++i)
        if (st[i].on_device)
            for (int b = 0; b < hd[i].nblocks; ++b) owned[(size_t)hd[i].first_block + b] = 1;
    long long guard_bad = 0;
    for (long long b = 0; b < blocks; ++b)
        if (!owned[(size_t)b])
            for (int k = 0; k < 64; ++k) guard_bad += coef[b * 64 + k] != 0x7777;
    if (guard_bad) { printf("  %lld guard coefficients overwritten\n", guard_bad); ++fails; }
    for (int i = 0; i < N && !rc; ++i) {
        const Item& it = *items[i];
        const Staged& s = st[i];
        if (!s.info.supported) {
            if (verbose) printf("  %s: not supported by the parser (%d)\n", it.name.c_str(), s.info.reason);
            continue;
        }
        if (!s.on_device) continue;
        const int got = status[i];
        const int16_t* mine = coef + (size_t)hd[i].first_block * 64;
        const bool same = memcmp(mine, s.want.data(), s.want.size() * 2) == 0 && memcmp(s.qtab, s.qwant, 384) == 0;
        bool ok;
        if (s.rc_host == 0) ok = got == 0 && same;
        else if (s.rc_host == 1) ok = got == WU_JPEG_MAGNITUDE && same;
        else if (got == 0 && s.rc_host == -3) { ok = true; ++g_lenient; }
        else ok = got != 0 && (got & ~0xff) != 0;
        if (got == WU_JPEG_MAGNITUDE) ++g_magnitude;
        else if (got) ++g_rejected;
        if (!ok || verbose)
            printf("  %s S=%d: host %d, status 0x%x, blocks %s%s\n", it.name.c_str(), S, s.rc_host, got, same ? "equal" : "differ", ok ? "" : "   <-- WRONG");
        fails += !ok;
    }
    free(status); free(coef); free(hd_dev); free(qtab_dev); free(dht_dev); free(seg_dev); free(scan_dev);
    return fails;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    int batch = 5, fuzz = 0, at = 1;
    std::vector<int> sizes = {64, 128, 1024};
    while (at + 1 < argc && argv[at][0] == '-') {
        if (!strcmp(argv[at], "--batch")) batch = atoi(argv[at + 1]);
        else if (!strcmp(argv[at], "--fuzz")) fuzz = atoi(argv[at + 1]);
        else if (!strcmp(argv[at], "--subseq")) {
            sizes.clear();
            for (char* tok = strtok(argv[at + 1], " ,"); tok; tok = strtok(nullptr, " ,")) sizes.push_back(atoi(tok));
        }
        at += 2;
    }
    if (at >= argc || sizes.empty()) { fprintf(stderr, "usage: jpeg_huff_emu [--batch K] [--fuzz M] [--subseq \"64 128 1024\"] DIR\n"); return 2; }
    const std::string dir = argv[at];
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".jpg") names.push_back(n);
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    std::vector<Item> items;
    for (const auto& n : names) items.push_back(Item{n, slurp(dir + "/" + n)});
    if (items.empty()) { fprintf(stderr, "no .jpg files in %s\n", dir.c_str()); return 2; }
    int fails = 0;
    for (int S : sizes) {
        printf("each file alone, S = %d:\n", S);
        for (const auto& it : items) fails += run_batch({&it}, S, false);
    }
    if (batch > 1) {
        printf("batches of %d, S = %d:\n", batch, sizes[0]);
        const size_t n = items.size(), stride = n / (size_t)batch + 1;      // neighbours in a batch differ in kind
        for (size_t b = 0; b < stride; ++b) {
            std::vector<const Item*> group;
            for (size_t i = b; i < n; i += stride) group.push_back(&items[i]);
            if (!group.empty()) fails += run_batch(group, sizes[0], false);
        }
    }
    if (fuzz > 0) {
        printf("%d bit-flipped and %d truncated copies of each file:\n", fuzz, fuzz);
        uint64_t rng = 0x9E3779B97F4A7C15ull;
        size_t si = 0;
        for (const auto& it : items) {
            wu_jpeg_info info;
            wu_jpeg_parse(it.file.data(), it.file.size(), &info);
            if (!info.supported || (size_t)info.scan_offset + 2 >= it.file.size()) continue;
            const uint64_t span = it.file.size() - (size_t)info.scan_offset;
            for (int m = 0; m < 2 * fuzz; ++m) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                const size_t pos = (size_t)info.scan_offset + (size_t)((rng >> 33) % span);
                Item bad{it.name + (m < fuzz ? " (bit flipped)" : " (cut short)"), it.file};
                if (m < fuzz) bad.file[pos] ^= (uint8_t)(1u << ((rng >> 20) & 7));
                else bad.file.resize(pos + 1);
                fails += run_batch({&bad}, sizes[si++ % sizes.size()], false);
            }
        }
    }
    printf("%zu files, %lld streams staged (%lld refused by the staging, %lld rejected by the device, %lld over the magnitude bound, "
           "%lld accepted past junk in front of RSTn), most barriers in one call %lld, %d wrong\n",
           items.size(), g_streams, g_stage_refused, g_rejected, g_magnitude, g_lenient, g_max_rounds_barriers, fails);
    return fails ? 1 : 0;
}
