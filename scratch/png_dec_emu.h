// CPU emulation shim for csrc/png_dec.hip, installed by png_dec_emu_build.sh in place of wu_common.h.  A workgroup is 64 free-running
// host threads; __syncthreads() is a barrier over them and the ONLY thing that orders them, as in the kernels.  Nothing runs in lockstep,
// so a barrier the kernels lack between a write and another lane's read is a data race (ThreadSanitizer) or a wrong result.  __shared__
// data (WU_LDS) is heap memory of exactly the struct's size, filled with 0xA5 before every workgroup: an index past the struct is an
// AddressSanitizer report, past a member array an UBSan bounds report, and nothing can lean on LDS being zero or left over.
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
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
inline thread_local dim3 threadIdx, blockIdx;
using std::max;
using std::min;
typedef void* hipStream_t;
inline thread_local char g_wu_err[256];
#define WU_FAIL(code, ...) do { snprintf(g_wu_err, sizeof(g_wu_err), __VA_ARGS__); return (code); } while (0)
#define WU_REQUIRE(cond, ...) do { if (!(cond)) WU_FAIL(-1, __VA_ARGS__); } while (0)
#define WU_LAUNCH_CHECK(name) do {} while (0)

constexpr int kEmuThreads = 64;
struct EmuBarrier {            // mutex + condition variable: nothing a sanitizer has to guess at
    std::mutex m;
    std::condition_variable cv;
    int expected = kEmuThreads, waiting = 0;
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
    uint32_t shfl[kEmuThreads];
    ~EmuBlock() { free(lds); }
};
inline EmuBlock* g_emu;
inline long long g_emu_barriers;
template <typename T> T* emu_lds() {
    std::call_once(g_emu->lds_once, [] {
        g_emu->lds = malloc(sizeof(T));
        memset(g_emu->lds, 0xA5, sizeof(T));
    });
    return (T*)g_emu->lds;
}
#define WU_LDS(type, name) type& name = *emu_lds<type>()
inline void __syncthreads() { g_emu->barrier.arrive_and_wait(); }
inline uint32_t __shfl_up(uint32_t v, int d) {         // a wave-wide exchange of register values: two rendezvous around a mailbox
    const int l = (int)threadIdx.x;
    g_emu->shfl[l] = v;
    g_emu->barrier.arrive_and_wait();
    const uint32_t r = l >= d ? g_emu->shfl[l - d] : v;
    g_emu->barrier.arrive_and_wait();
    return r;
}
inline uint32_t __brev(uint32_t v) { uint32_t r = 0; for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i); return r; }
template <typename T, typename U> inline T atomicAdd(T* p, U v) { return __atomic_fetch_add(p, (T)v, __ATOMIC_RELAXED); }
template <typename T, typename U> inline T atomicXor(T* p, U v) { return __atomic_fetch_xor(p, (T)v, __ATOMIC_RELAXED); }
template <typename T, typename U> inline T atomicOr(T* p, U v) { return __atomic_fetch_or(p, (T)v, __ATOMIC_RELAXED); }
template <typename T> inline T atomicMin(T* p, T v) {
    T o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
template <typename F> void emu_launch(dim3 grid, dim3 block, F body) {
    if (block.x != (unsigned)kEmuThreads) abort();
    for (unsigned b = 0; b < grid.x; ++b) {
        EmuBlock eb;
        g_emu = &eb;
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t)
            ts.emplace_back([&eb, &body, t, b] {
                threadIdx = dim3(t);
                blockIdx = dim3(b);
                body();
                eb.barrier.drop();
            });
        for (auto& t : ts) t.join();
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(grid, block, [&] { kernel(__VA_ARGS__); })
