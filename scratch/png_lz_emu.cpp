// Stand-alone CPU run of the PNG encoder's segment kernels (csrc/png_enc.hip compiled as host C++ under WU_PNG_ENC_EMU): the literal-only
// deflate, the LZ77 match-and-parse kernel (head-table rounds, match extension, the chunked greedy parse) and the LZ77 coding kernel, as
// they are -- a workgroup is 256 host threads, __syncthreads() a barrier, the atomics the host's, __shared__ a static -- against the
// segments of tests/_png_lz_ref.py.  CPU only: no GPU, no HIP runtime, nothing loaded into an interpreter.
//
//   clang++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined scratch/png_lz_emu.cpp -o png_lz_emu
//   python -c "import sys; sys.path.insert(0, 'tests'); import _png_lz_cases as C; print(C.dump('DIR'))"
//   ./png_lz_emu DIR
//
// DIR/NAME.in: int32 h, w, then the filtered stream; DIR/NAME.want: per segment int32 mode (0 literal-only, 1 stored, 2 LZ77), int32 n and
// the n bytes of the restatement's segment (tests/_png_lz_cases.py dump()).  Every buffer is a heap block of EXACTLY the size the
// library's layout gives it, poisoned.  The kernels run twice per case, the second time over the first run's workspace: the bytes must
// not depend on what a launch finds there.  Exit status 1 if a byte differs.
#include <dirent.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

// ---- the HIP names the kernels use -----------------------------------------------------------------------------------------------------
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct Idx3 { int x, y, z; };
static thread_local Idx3 threadIdx;
static Idx3 blockIdx;
static pthread_barrier_t g_barrier;
static inline void __syncthreads() { pthread_barrier_wait(&g_barrier); }
struct uint4 { uint32_t x, y, z, w; };
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
using std::max;
using std::min;
template <typename T> static inline T atomicAdd(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <typename T> static inline T atomicOr(T* p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline uint32_t atomicMax(uint32_t* p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline uint32_t __brev(uint32_t v) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline int __ffs(int v) { return __builtin_ffs(v); }

// what the kernels take from png_internal.h and codec_internal.h
namespace {
constexpr int kPngSeg = 32768;
constexpr uint32_t kAdlerMod = 65521u;
const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
inline unsigned block_scan_inclusive(unsigned v, unsigned* sm, int tid) {
    sm[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned add = tid >= off ? sm[tid - off] : 0u;
        __syncthreads();
        sm[tid] += add;
        __syncthreads();
    }
    return sm[tid];
}
}  // namespace
#define WU_PNG_ENC_LZ77 1

#define WU_PNG_ENC_EMU 1
#include "../weather-unet_amd/csrc/png_enc.hip"

// one workgroup after the other, 256 threads each
template <typename F> static void launch(int nblocks, F kernel) {
    for (int b = 0; b < nblocks; ++b) {
        blockIdx = Idx3{b, 0, 0};
        pthread_barrier_init(&g_barrier, nullptr, 256);
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t)
            th.emplace_back([&, t] {
                threadIdx = Idx3{t, 0, 0};
                kernel();
                // a thread that left early (a segment that keeps its block) no longer takes part: the others have left by the same test
            });
        for (auto& t : th) t.join();
        pthread_barrier_destroy(&g_barrier);
    }
}

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
    T* p = (T*)aligned_alloc(256, (n * sizeof(T) + 255) / 256 * 256);
    memset(p, 0xA5, n * sizeof(T));
    return p;
}

static int run_case(const std::string& dir, const std::string& name) {
    const std::vector<uint8_t> in = slurp(dir + "/" + name + ".in"), want = slurp(dir + "/" + name + ".want");
    if (in.size() < 8) { printf("%s: no input\n", name.c_str()); return 1; }
    int h, w;
    memcpy(&h, in.data(), 4);
    memcpy(&w, in.data() + 4, 4);
    const Geo g = make_geo(h, w, h, w);
    if (in.size() != 8 + (size_t)g.len) { printf("%s: %zu bytes for %d x %d\n", name.c_str(), in.size(), h, w); return 1; }
    const long long fstride = (long long)g.nseg * kSeg;
    uint8_t* filt = poisoned<uint8_t>((size_t)fstride);
    memcpy(filt, in.data() + 8, (size_t)g.len);
    PngEncDesc* desc = poisoned<PngEncDesc>(1);
    desc->h = h; desc->w = w;
    uint8_t* slots = poisoned<uint8_t>((size_t)g.nseg * kSlot);
    uint32_t* info = poisoned<uint32_t>((size_t)g.nseg * 4);
    uint32_t* toks = poisoned<uint32_t>((size_t)g.nseg * kSeg);
    int bad = 0;
    for (int pass = 0; pass < 2 && !bad; ++pass) {
        launch(g.nseg, [&] { png_enc_deflate_kernel(filt, fstride, desc, slots, info, g.nseg, h, w); });
        launch(g.nseg, [&] { png_enc_match_kernel(filt, fstride, desc, toks, g.nseg, h, w); });
        launch(g.nseg, [&] { png_enc_lzcode_kernel(toks, desc, slots, info, g.nseg, h, w); });
        size_t at = 0;
        for (int s = 0; s < g.nseg && !bad; ++s) {
            int mode, n;
            if (at + 8 > want.size()) { bad = 1; break; }
            memcpy(&mode, want.data() + at, 4);
            memcpy(&n, want.data() + at + 4, 4);
            at += 8;
            const uint32_t got_n = info[4 * s], got_mode = info[4 * s + 3];
            if (got_n != (uint32_t)n || got_mode != (uint32_t)mode || at + n > want.size() ||
                memcmp(slots + (size_t)s * kSlot, want.data() + at, (size_t)n) != 0) {
                size_t d = 0;
                while (d < (size_t)n && d < got_n && slots[(size_t)s * kSlot + d] == want[at + d]) ++d;
                printf("%s pass %d segment %d: %u bytes mode %u, the restatement has %d bytes mode %d; first difference at %zu\n", name.c_str(),
                       pass, s, got_n, got_mode, n, mode, d);
                bad = 1;
            }
            at += (size_t)n;
        }
    }
    if (!bad) printf("%s: %d segment(s) equal, twice\n", name.c_str(), g.nseg);
    free(filt); free(desc); free(slots); free(info); free(toks);
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: png_lz_emu DIR\n"); return 2; }
    std::vector<std::string> names;
    DIR* d = opendir(argv[1]);
    if (!d) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    while (dirent* e = readdir(d)) {
        const std::string f = e->d_name;
        if (f.size() > 3 && f.substr(f.size() - 3) == ".in") names.push_back(f.substr(0, f.size() - 3));
    }
    closedir(d);
    std::sort(names.begin(), names.end());
    int bad = 0;
    for (const auto& n : names) bad |= run_case(argv[1], n);
    printf("%zu cases, %s\n", names.size(), bad ? "DIFFERENCES" : "all equal");
    return bad || names.empty();
}
