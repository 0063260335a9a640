// Host-only sanitizer driver for the JPEG host stage with the extended coverage (csrc/jpeg_host.h: wu_jpeg_parse_ex, the progressive
// scans of wu_jpeg_entropy_decode, 4:4:0).  The header is plain C++, so no HIP compiler, no GPU and no LD_PRELOAD is involved:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
//       scratch/jpeg_prog_asan.cpp -o jpeg_prog_asan                                        (one command line)
//   ./jpeg_prog_asan [--flips K] tests/golden/jpeg/progressive.jpg tests/golden/jpeg/s440.jpg more.jpg ...
//
// (tests/test_jpeg_prog_cpu.py builds and runs exactly this over its grid.)  Every input is copied into a heap buffer of EXACTLY its
// size and decoded into a coefficient buffer of EXACTLY info.coef_bytes, so an over-read or over-write of either is a report.  Per file
// and per flag set (0 and ALLOW_PROGRESSIVE | ALLOW_H1V2): the whole file; ~200 truncation lengths; K (default 2000) single-byte
// corruptions at seeded pseudo-random offsets, header, tables between scans and scans alike.  Prints how each class of input ended; a
// crash or a sanitizer report is the failure (non-zero exit).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../weather-unet_amd/csrc/jpeg_host.h"

thread_local char g_wu_err[256] = {0};

static int counts[4];   // 0 decoded, 1 unsupported, 2 error, 3 refused by the entropy stage (magnitude, incomplete)

static void one(const uint8_t* src, size_t n, int flags) {
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    memcpy(data, src, n);
    wu_jpeg_info info;
    wu_jpeg_parse_ex(data, n, &info, flags);
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
    int flips = 2000, first = 1;
    if (argc > 2 && strcmp(argv[1], "--flips") == 0) {
        flips = atoi(argv[2]);
        first = 3;
    }
    int whole_ok = 0, files = 0;
    for (int f = first; f < argc; ++f) {
        FILE* fh = fopen(argv[f], "rb");
        if (!fh) {
            fprintf(stderr, "cannot open %s\n", argv[f]);
            return 2;
        }
        std::vector<uint8_t> buf;
        uint8_t tmp[4096];
        size_t got;
        while ((got = fread(tmp, 1, sizeof(tmp), fh)) > 0) buf.insert(buf.end(), tmp, tmp + got);
        fclose(fh);
        if (buf.empty()) continue;
        ++files;
        for (int flags = 0; flags <= 3; flags += 3) {
            memset(counts, 0, sizeof(counts));
            one(buf.data(), buf.size(), flags);
            if (flags && counts[0] == 1) ++whole_ok;
            const size_t step = buf.size() / 200 + 1;
            for (size_t cut = 0; cut < buf.size(); cut += step) one(buf.data(), cut, flags);
            uint64_t s = 0x9E3779B97F4A7C15ull + (uint64_t)f;
            std::vector<uint8_t> bad(buf);
            for (int k = 0; k < flips; ++k) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const size_t at = (size_t)((s >> 33) % buf.size());
                const uint8_t old = bad[at];
                bad[at] = (uint8_t)(s >> 24);
                one(bad.data(), bad.size(), flags);
                bad[at] = old;
            }
            printf("%s flags %d: %zu bytes: decoded %d, unsupported %d, error %d, refused %d\n", argv[f], flags, buf.size(), counts[0], counts[1],
                   counts[2], counts[3]);
        }
    }
    printf("files %d, decoded whole with the extended flags %d\n", files, whole_ok);
    return 0;
}
