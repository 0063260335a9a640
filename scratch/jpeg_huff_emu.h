// CPU emulation shim for csrc/jpeg_huff.hip (and csrc/jpeg.hip, whose host half is the reference), installed by
// jpeg_huff_emu_build.sh in place of wu_common.h.  The shim of scratch/png_dec_emu.h with the workgroup size taken from the launch
// (256 here), a two-dimensional grid and the vector types the JPEG files use.  A workgroup is block.x free-running host threads;
// __syncthreads() is a barrier over them and the ONLY thing that orders them, as in the kernels.  Nothing runs in lockstep, so a barrier
// the kernels lack between a write and another thread's read is a data race (ThreadSanitizer) or a wrong result.  LDS (WU_LDS) is heap
// memory of exactly the struct's size, filled with 0xA5 before every workgroup: an index past the struct is an AddressSanitizer report,
// past a member array an UBSan bounds report, and nothing can lean on LDS being zero or left over.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "wu_kernels.h"

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
#define __shared__ static          // only in kernels the emulation never launches (csrc/jpeg.hip's device half)
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct uint2 { unsigned x, y; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
inline uint2 make_uint2(unsigned x, unsigned y) { return uint2{x, y}; }
inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return uint4{x, y, z, w}; }
inline thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
using std::max;
using std::min;
typedef void* hipStream_t;
inline thread_local char g_wu_err[256];
#define WU_FAIL(code, ...) do { snprintf(g_wu_err, sizeof(g_wu_err), __VA_ARGS__); return (code); } while (0)
#define WU_REQUIRE(cond, ...) do { if (!(cond)) WU_FAIL(-1, __VA_ARGS__); } while (0)
#define WU_LAUNCH_CHECK(name) do {} while (0)

struct EmuBarrier {            // mutex + condition variable: nothing a sanitizer has to guess at
    std::mutex m;
    std::condition_variable cv;
    int expected = 0, waiting = 0;
    unsigned gen = 0;
    void arrive_and_wait() {
        std::unique_lock<std::mutex> lk(m);
        if (++waiting == expected) { waiting = 0; ++gen; cv.notify_all(); }
        else { const unsigned g = gen; cv.wait(lk, [&] { return gen != g; }); }
    }
    void drop() {              // a thread that left the kernel no longer counts
        std::unique_lock<std::mutex> lk(m);
        --expected;
        if (waiting > 0 && waiting == expected) { waiting = 0; ++gen; cv.notify_all(); }
    }
};
struct EmuBlock {
    EmuBarrier barrier;
    std::once_flag lds_once;
    void* lds = nullptr;
    ~EmuBlock() { free(lds); }
};
inline EmuBlock* g_emu;
inline long long g_emu_barriers;       // barrier rounds of all workgroups so far (thread 0 counts)
template <typename T> T* emu_lds() {
    std::call_once(g_emu->lds_once, [] {
        g_emu->lds = malloc(sizeof(T));
        memset(g_emu->lds, 0xA5, sizeof(T));
    });
    return (T*)g_emu->lds;
}
#define WU_LDS(type, name) type& name = *emu_lds<type>()
inline void __syncthreads() {
    if (threadIdx.x == 0) ++g_emu_barriers;
    g_emu->barrier.arrive_and_wait();
}
template <typename T, typename U> inline T atomicOr(T* p, U v) { return __atomic_fetch_or(p, (T)v, __ATOMIC_RELAXED); }
template <typename F> void emu_launch(dim3 grid, dim3 block, F body) {
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            EmuBlock eb;
            eb.barrier.expected = (int)block.x;
            g_emu = &eb;
            std::vector<std::thread> ts;
            for (unsigned t = 0; t < block.x; ++t)
                ts.emplace_back([&eb, &body, t, bx, by, grid, block] {
                    threadIdx = dim3(t);
                    blockIdx = dim3(bx, by);
                    blockDim = block;
                    gridDim = grid;
                    body();
                    eb.barrier.drop();
                });
            for (auto& t : ts) t.join();
        }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(grid, block, [&] { kernel(__VA_ARGS__); })
