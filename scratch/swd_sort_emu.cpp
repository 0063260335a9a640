// Stand-alone CPU walk of the index arithmetic of the segmented sort in csrc/swd.hip: the plain bitonic block sort, the full-block path
// (16 keys per thread in "registers", swizzled LDS index) and the LDS-tiled merge pass, restated thread by thread with every barrier phase
// as a loop over the workgroup's threads.  It is a restatement, not the kernel's source: it checks the algorithm and every index it forms
// (each "LDS" and global array is a heap block of exactly the kernel's size, so AddressSanitizer sees a step outside), not the barriers.
// CPU only: no GPU, no HIP runtime, nothing loaded into an interpreter.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined scratch/swd_sort_emu.cpp -o swd_sort_emu
//   ./swd_sort_emu            (exit status 1 if a column is not sorted or not a permutation of its input)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

static const int kBlock = 8192, kThreads = 512, kPer = 8, kTile = 256 * kPer;

static void cmpswap(double& x, double& y, bool asc) {
    const bool sw = (x > y) == asc;
    const double nx = sw ? y : x, ny = sw ? x : y;
    x = nx;
    y = ny;
}

static int phys(int i) { return i ^ ((i >> 4) & 15); }

static void sort_block_plain(double* base, int cnt) {
    int n2 = 2;
    while (n2 < cnt) n2 <<= 1;
    std::vector<double> s(n2);                                  // the kernel's array has kBlock entries; n2 <= kBlock is the tighter check
    for (int i = 0; i < n2; ++i) s[i] = i < cnt ? base[i] : INFINITY;
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
            for (int tid = 0; tid < kThreads; ++tid)
                for (int p = tid; p < (n2 >> 1); p += kThreads) {
                    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    cmpswap(s.at(i), s.at(i + j), (i & k) == 0);
                }
    for (int i = 0; i < cnt; ++i) base[i] = s[i];
}

static void sort_block_full(double* base) {
    std::vector<double> s(kBlock), v((size_t)kThreads * 16);
    std::vector<char> written(kBlock);
    for (int tid = 0; tid < kThreads; ++tid) {
        double* r = &v[(size_t)tid * 16];
        for (int q = 0; q < 16; ++q) r[q] = base[16 * tid + q];
        for (int k = 2; k <= 16; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1)
                for (int q = 0; q < 16; ++q)
                    if (!(q & j)) cmpswap(r[q], r[q | j], ((16 * tid + q) & k) == 0);
    }
    for (int k = 32; k <= kBlock; k <<= 1) {
        std::fill(written.begin(), written.end(), 0);
        for (int tid = 0; tid < kThreads; ++tid)
            for (int q = 0; q < 16; ++q) {
                const int a = phys(16 * tid + q);
                if (written.at(a)) { printf("phys() maps two keys to %d\n", a); exit(1); }
                written[a] = 1;
                s.at(a) = v[(size_t)tid * 16 + q];
            }
        for (int j = k >> 1; j >= 16; j >>= 1)
            for (int tid = 0; tid < kThreads; ++tid)
                for (int u = 0; u < kBlock / 2 / kThreads; ++u) {
                    const int p = tid + kThreads * u;
                    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    cmpswap(s.at(phys(i)), s.at(phys(i + j)), (i & k) == 0);
                }
        for (int tid = 0; tid < kThreads; ++tid) {
            double* r = &v[(size_t)tid * 16];
            for (int q = 0; q < 16; ++q) r[q] = s.at(phys(16 * tid + q));
            const bool asc = ((16 * tid) & k) == 0;
            for (int j = 8; j > 0; j >>= 1)
                for (int q = 0; q < 16; ++q)
                    if (!(q & j)) cmpswap(r[q], r[q | j], asc);
        }
    }
    for (int tid = 0; tid < kThreads; ++tid)
        for (int q = 0; q < 16; ++q) base[16 * tid + q] = v[(size_t)tid * 16 + q];
}

static int merge_path(const double* A, int nA, const double* B, int nB, int d) {
    int lo = std::max(0, d - nB), hi = std::min(d, nA);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mid >= nA || d - 1 - mid < 0 || d - 1 - mid >= nB) { printf("merge_path reads outside a run\n"); exit(1); }
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one workgroup of the merge pass; src and dst are the column's m keys exactly
static void merge_tile(const std::vector<double>& src, std::vector<double>& dst, int m, int L, int block) {
    std::vector<double> sIn(kTile), sOut(kTile);
    const long long o0 = (long long)block * kTile;
    const long long two = 2ll * L, s0 = o0 / two * two;
    const int nA = (int)std::min((long long)L, m - s0), nB = (int)std::min((long long)L, std::max(0ll, m - s0 - L));
    const int d0 = (int)(o0 - s0), d1 = std::min(d0 + kTile, nA + nB);
    // the runs as exact copies, so that a read past one is seen even where the next run follows it in memory
    std::vector<double> A(src.begin() + s0, src.begin() + s0 + nA), B(src.begin() + s0 + nA, src.begin() + s0 + nA + nB);
    const int i0 = merge_path(A.data(), nA, B.data(), nB, d0), i1 = merge_path(A.data(), nA, B.data(), nB, d1);
    const int j0 = d0 - i0, cnt = d1 - d0, cntA = i1 - i0, cntB = cnt - cntA;
    for (int e = 0; e < cnt; ++e) sIn.at(e) = e < cntA ? A.at(i0 + e) : B.at(j0 + e - cntA);
    for (int tid = 0; tid < 256; ++tid) {
        const int dl = tid * kPer;
        if (dl >= cnt) continue;
        std::vector<double> lA(sIn.begin(), sIn.begin() + cntA), lB(sIn.begin() + cntA, sIn.begin() + cnt);
        int i = merge_path(lA.data(), cntA, lB.data(), cntB, dl), j = dl - i;
        const int n = std::min(kPer, cnt - dl);
        for (int t = 0; t < n; ++t) {
            if (j >= cntB || (i < cntA && lA.at(i) <= lB.at(j))) sOut.at(dl + t) = lA.at(i++);
            else sOut.at(dl + t) = lB.at(j++);
        }
    }
    for (int e = 0; e < cnt; ++e) dst.at(o0 + e) = sOut.at(e);
}

static bool sort_column(std::vector<double> keys, const char* what) {
    const int m = (int)keys.size();
    std::vector<double> want(keys), tmp(m, NAN);
    std::sort(want.begin(), want.end());
    for (int first = 0; first < m; first += kBlock) {
        const int cnt = std::min(kBlock, m - first);
        if (cnt == kBlock) sort_block_full(keys.data() + first);
        else sort_block_plain(keys.data() + first, cnt);
    }
    std::vector<double>*src = &keys, *dst = &tmp;
    for (int L = kBlock; L < m; L <<= 1) {
        for (int b = 0; b < (m + kTile - 1) / kTile; ++b) merge_tile(*src, *dst, m, L, b);
        std::swap(src, dst);
    }
    const bool ok = *src == want;
    printf("%-28s m %7d  %s\n", what, m, ok ? "ok" : "WRONG");
    return ok;
}

int main() {
    bool ok = true;
    srand(1);
    const int sizes[] = {1, 2, 3, 63, 64, 65, 1000, kBlock - 1, kBlock, kBlock + 1, 2 * kBlock + 17, 5 * kBlock + 3, 8 * kBlock, 9 * kBlock - 1};
    for (int m : sizes) {
        std::vector<double> a(m), b(m), c(m), d(m);
        for (int i = 0; i < m; ++i) {
            a[i] = rand() / (double)RAND_MAX - 0.5;
            b[i] = i - m / 2;
            c[i] = m / 3 - i;
            d[i] = rand() % 5 - 2;
        }
        ok &= sort_column(a, "random");
        ok &= sort_column(b, "ascending");
        ok &= sort_column(c, "descending");
        ok &= sort_column(d, "duplicates");
        ok &= sort_column(std::vector<double>(m, -7.0), "all equal");
    }
    return ok ? 0 : 1;
}
