// Stand-alone CPU run of the resampler's device functions (csrc/resample.hip compiled as host C++ under WU_RESAMPLE_EMU): a workgroup is a
// loop over its threads per step (stage the row, filter it, accumulate), so the run checks the arithmetic and every index the kernel
// forms -- into the staged row, the tables, the source and the output -- not its barriers.  CPU only: no GPU, no HIP runtime, nothing
// loaded into an interpreter.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include scratch/resample_emu.cpp -o resample_emu
//   python -c "import sys; sys.path[:0] = ['tests', 'weather-unet_amd']; import _resample_cases as C; print(C.dump('DIR'))"
//   ./resample_emu DIR
//
// DIR/NAME.in and DIR/NAME.want: tests/_resample_cases.py dump().  Every buffer is a heap block of EXACTLY the size the launch gives it
// (the workspace image, the padded source, the staged row of the widest image that takes a horizontal pass, the output).  Each case runs
// at band heights 1, 3 and the default; exit status 1 if a byte differs from Pillow's.
#define WU_RESAMPLE_EMU 1
#include "../weather-unet_amd/csrc/resample.hip"

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

template <int MODE> struct Thread {
    typename Acc<MODE>::type acc[3][kBandMax];
    int xmin, xn;
};

// resample_kernel<MODE, SRC_U8>, one workgroup (band b of image n), thread by thread
template <int MODE>
static void workgroup(const uint8_t* src, const uint8_t* ws, int Hout, int Wout, int band, int n, int b, uint8_t* stage, int max_stage_w, Out out) {
    typedef typename Acc<MODE>::type A;
    typedef typename Acc<MODE>::mid M;
    const int oy0 = b * band, nthreads = (Wout + 63) / 64 * 64;
    ResDesc d;
    memcpy(&d, ws + (size_t)n * sizeof(ResDesc), sizeof(d));
    if (d.kx > 0 && d.src_w > max_stage_w) abort();
    const int nrows = Hout - oy0 < band ? Hout - oy0 : band;
    int ymin[kBandMax], ycnt[kBandMax], ylo, yhi;
    band_rows(d, (const int*)(ws + d.vb), oy0, nrows, ymin, ycnt, ylo, yhi);
    std::vector<Thread<MODE>> th(Wout);
    for (int ox = 0; ox < Wout; ++ox) {
        th[ox].xmin = th[ox].xn = 0;
        if (d.kx > 0) column_taps(d, (const int*)(ws + d.hb), ox, th[ox].xmin, th[ox].xn);
        for (int j = 0; j < kBandMax; ++j) th[ox].acc[0][j] = th[ox].acc[1][j] = th[ox].acc[2][j] = MODE == MODE_U8 && d.ky > 0 ? (A)(1 << (kPrec - 1)) : (A)0;
    }
    const A* vk = (const A*)(ws + d.vk);
    for (int sy = ylo; sy < yhi; ++sy) {
        if (d.kx > 0)
            for (int tid = 0; tid < nthreads; ++tid) stage_row<MODE, SRC_U8>(stage, src, d, sy, 0, tid, nthreads);
        for (int ox = 0; ox < Wout; ++ox) {
            M v[3] = {0, 0, 0};
            if (d.kx > 0) {
                filter_row<MODE, uint8_t>(stage, (const A*)(ws + d.hk) + ox, Wout, th[ox].xmin, th[ox].xn, v);
            } else {
                const long long base = d.src_off + (long long)sy * d.s_row + (long long)ox * d.s_col;
                for (int c = 0; c < 3; ++c) v[c] = (M)sample<MODE, SRC_U8>(src, base + (long long)c * d.s_ch, 0);
            }
            accumulate<MODE>(th[ox].acc, v, sy, ymin, ycnt, vk, d.ky, oy0);
        }
    }
    for (int ox = 0; ox < Wout; ++ox)
        for (int j = 0; j < nrows; ++j) {
            float val[3];
            finish<MODE>(th[ox].acc, j, d.ky, val);
            epilogue(out, val, n, oy0 + j, ox, Hout, Wout);
        }
}

static int run_case(const std::string& base) {
    const std::vector<uint8_t> in = slurp(base + ".in"), want = slurp(base + ".want");
    if (in.size() < 28) { printf("%s: unreadable\n", base.c_str()); return 1; }
    int head[7];
    memcpy(head, in.data(), sizeof(head));
    const int N = head[0], Hout = head[1], Wout = head[2], mode = head[3], Hm = head[4], Wm = head[5], ws_bytes = head[6];
    const size_t src_bytes = (size_t)N * Hm * Wm * 3;
    if (in.size() != 28 + (size_t)ws_bytes + src_bytes) { printf("%s: bad size\n", base.c_str()); return 1; }
    uint8_t* ws = (uint8_t*)malloc(ws_bytes);
    memcpy(ws, in.data() + 28, ws_bytes);
    uint8_t* src = (uint8_t*)malloc(src_bytes);
    memcpy(src, in.data() + 28 + ws_bytes, src_bytes);
    int max_stage_w = 0;
    for (int n = 0; n < N; ++n) {
        ResDesc d;
        memcpy(&d, ws + (size_t)n * sizeof(ResDesc), sizeof(d));
        if (d.kx > 0) max_stage_w = std::max(max_stage_w, d.src_w);
    }
    uint8_t* stage = (uint8_t*)malloc((size_t)max_stage_w * 3 + 1);     // +1: malloc(0) may return NULL
    const size_t out_bytes = (size_t)N * Hout * Wout * 3 * (mode ? 1 : sizeof(float));
    int bad = want.size() != out_bytes;
    const int bands[3] = {1, 3, kBandMax};
    for (int bi = 0; bi < 3 && !bad; ++bi) {
        uint8_t* dst = (uint8_t*)malloc(out_bytes);
        memset(dst, 0xA5, out_bytes);
        Out o;
        o.dst = dst; o.epi = mode ? EPI_NHWC_U8 : EPI_RAW; o.normalize = 0; o.ldy = 0; o.cpad = 0; o.bf16 = 0;
        const int band = bands[bi];
        for (int n = 0; n < N; ++n)
            for (int b = 0; b * band < Hout; ++b) {
                if (mode) workgroup<MODE_U8>(src, ws, Hout, Wout, band, n, b, stage, max_stage_w, o);
                else workgroup<MODE_F32>(src, ws, Hout, Wout, band, n, b, stage, max_stage_w, o);
            }
        if (mode) {
            bad = memcmp(dst, want.data(), out_bytes) != 0;
        } else {                                                       // RAW is (N, 3, Hout, Wout); Pillow's answer (N, Hout, Wout, 3)
            const float* g = (const float*)dst;
            const size_t plane = (size_t)Hout * Wout;
            for (int n = 0; n < N && !bad; ++n)
                for (size_t p = 0; p < plane && !bad; ++p)
                    for (int c = 0; c < 3; ++c)
                        if (memcmp(g + ((size_t)n * 3 + c) * plane + p, want.data() + (((size_t)n * plane + p) * 3 + c) * 4, 4) != 0) bad = 1;
        }
        if (bad) printf("%s: band %d differs from Pillow\n", base.c_str(), band);
        free(dst);
    }
    free(stage);
    free(src);
    free(ws);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    std::vector<std::string> names;
    DIR* dir = opendir(argv[1]);
    if (!dir) { perror(argv[1]); return 2; }
    while (dirent* e = readdir(dir)) {
        const std::string f = e->d_name;
        if (f.size() > 3 && f.substr(f.size() - 3) == ".in") names.push_back(std::string(argv[1]) + "/" + f.substr(0, f.size() - 3));
    }
    closedir(dir);
    std::sort(names.begin(), names.end());
    int bad = 0;
    for (const std::string& b : names) bad += run_case(b);
    printf("%zu cases, %d differ\n", names.size(), bad);
    return bad || names.empty() ? 1 : 0;
}
