// Host-only AddressSanitizer driver for the JPEG host stage (csrc/jpeg.hip: wu_jpeg_parse, wu_jpeg_entropy_decode).  CPU only: ASan
// instruments the HOST pass alone (-Xarch_host); the device code object is embedded as usual and never launched -- no GPU is needed or
// touched.  Every input is copied into a heap buffer of EXACTLY its size and decoded into a coefficient buffer of EXACTLY
// info.coef_bytes, so an over-read or over-write of either is an ASan report.
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer -std=c++17 -I include \
//         -c weather-unet_amd/csrc/jpeg.hip -o jpeg_asan.o
//   clang++ -O1 -g -fsanitize=address -fno-omit-frame-pointer -std=c++17 -I include -c scratch/jpeg_host_asan.cpp -o driver.o
//   hipcc -fsanitize=address jpeg_asan.o driver.o -o jpeg_host_asan
//   ./jpeg_host_asan tests/golden/jpeg/*.jpg more.jpg ...
//
// Per file: the whole file; ~400 truncation lengths; 4000 single-byte corruptions at seeded pseudo-random offsets (header and scan
// alike).  Prints how each class of input ended; a crash or an ASan report is the failure.
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

static int counts[4];   // 0 decoded, 1 unsupported, 2 error, 3 magnitude

static void one(const uint8_t* src, size_t n) {
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    memcpy(data, src, n);
    wu_jpeg_info info;
    wu_jpeg_parse(data, n, &info);
    if (!info.supported) {
        ++counts[1];
        free(data);
        return;
    }
    int16_t* coef = (int16_t*)malloc((size_t)info.coef_bytes);
    uint16_t q[192];
    const int rc = wu_jpeg_entropy_decode(data, n, &info, coef, (size_t)info.coef_bytes, q);
    ++counts[rc == 0 ? 0 : (rc == 1 ? 3 : 2)];
    free(coef);
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
        one(buf.data(), buf.size());
        const size_t step = buf.size() / 400 + 1;
        for (size_t cut = 0; cut < buf.size(); cut += step) one(buf.data(), cut);
        uint64_t s = 0x9E3779B97F4A7C15ull + f;
        std::vector<uint8_t> bad(buf);
        for (int k = 0; k < 4000; ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const size_t at = (size_t)((s >> 33) % buf.size());
            const uint8_t old = bad[at];
            bad[at] = (uint8_t)(s >> 24);
            one(bad.data(), bad.size());
            bad[at] = old;
        }
        printf("%s: %zu bytes: decoded %d, unsupported %d, error %d, magnitude %d\n", argv[f], buf.size(), counts[0], counts[1], counts[2], counts[3]);
    }
    return 0;
}
