// Host-only AddressSanitizer / UBSan driver for the PNG decoder's parser (csrc/png_dec.hip: wu_png_dec_parse).  CPU only: the
// sanitizers instrument the HOST pass alone (-Xarch_host); the device code object is embedded as usual and never launched -- no GPU is
// needed or touched.  Every input is copied into a heap buffer of EXACTLY its size, and the IDAT list has EXACTLY the capacity passed, so
// an over-read or over-write of either is a report.
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -std=c++17 -I include \
//         -c weather-unet_amd/csrc/png_dec.hip -o png_dec_asan.o
//   clang++ -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -std=c++17 -I include -c scratch/png_parse_asan.cpp -o driver.o
//   hipcc -fsanitize=address,undefined png_dec_asan.o driver.o -o png_parse_asan
//   ./png_parse_asan good.png corrupt.png ...
//
// Per file: the whole file with list capacities 0, 1, 3 and 4096; every truncation length (every 7th for files over 64 KiB); 4000
// single-byte corruptions at seeded pseudo-random offsets and every 32-bit chunk length replaced by hostile values.  Prints how each
// class of input ended; a crash or a sanitizer report is the failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wu_kernels.h"

thread_local char g_wu_err[256] = {0};
extern "C" const char* wu_last_error(void) { return g_wu_err; }
int g_wu_opt[16];
void* g_wu_dbg_ptr;

static int counts[16];   // by reason; 0 = supported

static void one(const uint8_t* src, size_t n, int cap) {
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(data, src, n);
    long long* idat = (long long*)malloc(sizeof(long long) * 2 * (cap ? cap : 1));
    wu_png_dec_info info;
    if (wu_png_dec_parse(data, n, 89478485, &info, cap ? idat : nullptr, cap) != 0) abort();
    if (info.supported) {
        if (info.n_idat != info.n_segments) abort();
        for (int i = 0; i < info.n_idat && i < cap; ++i)      // what the caller would hand to the device must lie inside the file
            if (idat[2 * i] < 8 || idat[2 * i + 1] < 0 || (unsigned long long)idat[2 * i] + idat[2 * i + 1] + 4 > n) abort();
    }
    ++counts[info.supported ? 0 : (info.reason & 15)];
    free(idat);
    free(data);
}

int main(int argc, char** argv) {
    for (int f = 1; f < argc; ++f) {
        FILE* fh = fopen(argv[f], "rb");
        if (!fh) continue;
        std::vector<uint8_t> buf;
        uint8_t tmp[4096];
        size_t got;
        while ((got = fread(tmp, 1, sizeof(tmp), fh)) > 0) buf.insert(buf.end(), tmp, tmp + got);
        fclose(fh);
        memset(counts, 0, sizeof(counts));
        for (int cap : {0, 1, 3, 4096}) one(buf.data(), buf.size(), cap);
        const size_t step = buf.size() > 65536 ? 7 : 1;
        for (size_t cut = 0; cut < buf.size(); cut += step) one(buf.data(), cut, 8);
        uint64_t s = 0x9E3779B97F4A7C15ull + f;
        std::vector<uint8_t> bad(buf);
        for (int k = 0; k < 4000 && !buf.empty(); ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((s >> 33) % buf.size());
            const uint8_t old = bad[at];
            bad[at] = (uint8_t)(s >> 24);
            one(bad.data(), bad.size(), 8);
            bad[at] = old;
        }
        // every chunk's length field, found by walking the intact file
        const uint32_t hostile[] = {0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, (uint32_t)buf.size(), (uint32_t)buf.size() - 12u, 1u, 0u};
        for (size_t at = 8; at + 12 <= buf.size();) {
            const uint32_t len = ((uint32_t)buf[at] << 24) | ((uint32_t)buf[at + 1] << 16) | ((uint32_t)buf[at + 2] << 8) | buf[at + 3];
            for (uint32_t h : hostile) {
                uint8_t keep[4];
                memcpy(keep, &bad[at], 4);
                bad[at] = (uint8_t)(h >> 24); bad[at + 1] = (uint8_t)(h >> 16); bad[at + 2] = (uint8_t)(h >> 8); bad[at + 3] = (uint8_t)h;
                one(bad.data(), bad.size(), 8);
                memcpy(&bad[at], keep, 4);
            }
            if ((unsigned long long)len + 12 > buf.size() - at) break;
            at += 12 + (size_t)len;
        }
        printf("%s: %zu bytes: supported %d; refused by reason 1..8:", argv[f], buf.size(), counts[0]);
        for (int r = 1; r <= 8; ++r) printf(" %d", counts[r]);
        printf("\n");
    }
    return 0;
}
