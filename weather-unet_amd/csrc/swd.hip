// Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018): wu/swd.py, tests/_swd_ref.py states the arithmetic.
//   * swd_down_kernel      one thread per pixel of G_{l+1} = B(G_l)[2y, 2x]: the five column sums it needs (along H), then the row sum (along
//                          W); level 0 is read through the input's strides and mapped on the way, G_1.. live in the workspace as fp64;
//   * swd_gather_kernel    a workgroup per descriptor: the 11 x 11 neighbourhood of the zero-stuffed G_{l+1} per channel goes to LDS, the
//                          column pass with taps 2 f leaves 7 x 11, the row pass 7 x 7, and G_l - U_l is formed at those 147 pixels only --
//                          no Laplacian level and no fp64 copy of level 0 ever reaches global memory;
//   * swd_sum_kernel / swd_fold_kernel / swd_normalize_kernel
//                          per-channel sums of the 49 m values (then of the squared deviations) as per-workgroup partials folded by one
//                          workgroup, all in one fixed order; then (v - mu_c) / sigma_c, 0 where sigma_c is 0;
//   * swd_project_kernel   64 x 64 tiles of <descriptor row, direction row> (gram_tile_f64, D = 147), transposed through LDS so that the
//                          direction-major columns (dirs, m) are written 512 contiguous bytes at a time;
//   * swd_sort_block_kernel / swd_merge_kernel
//                          the segmented ascending sort of every column: a bitonic network over an LDS-resident block of kSwdSortBlock keys
//                          (a full block keeps 16 keys per thread in registers for the short-distance stages; short blocks are padded
//                          with +inf up to the next power of two only), then merge passes over global memory in
//                          which a workgroup finds its tile of the merge path by bisection, stages it in LDS, and every thread merges
//                          kSwdMergePer keys there;
//   * swd_distance_kernel  a workgroup per direction: mean_i |a_i - b_i| from a fixed-order tree sum;
//   * swd_distance_unequal_kernel
//                          the same for two columns of unequal length: the exact W1 of the two empirical distributions as a closed-form
//                          walk over the longer column, at most two keys of the shorter one per key, the same fixed-order sum.
// No atomics anywhere, every sum in one order that depends on the sizes alone: the same inputs give the same bits, whatever dir_chunk.
#include <math.h>

#include "gram_f64.h"

// every product, sum and quotient is rounded on its own, as the numpy restatement does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kSwdD = 147;                 // 3 x 7 x 7
constexpr int kSwdMaxLevels = 12;
constexpr int kSwdMaxDim = 1 << 15;
constexpr int kSwdMaxM = 1 << 21, kSwdMaxDirs = 4096;
constexpr int kSwdF64 = 3;                 // the Gaussian levels in the workspace (after WU_F32 / WU_BF16 / WU_SSIM_U8)
constexpr int kSwdSortBlock = 8192;        // keys one workgroup sorts in LDS: 64 KiB of doubles
constexpr int kSwdSortThreads = 512;
constexpr int kSwdMergePer = 8;            // keys a thread emits in a merge pass
constexpr int kSwdMergeTile = 256 * kSwdMergePer;   // keys a workgroup emits; divides kSwdSortBlock, so a tile never straddles two pairs
static_assert(kSwdSortBlock % kSwdMergeTile == 0, "a merge tile must not straddle two pairs of runs");
constexpr int kSwdSumGroups = 1024;        // partial sums of the statistics, at most
constexpr size_t kSwdAutoChunkBytes = 256ull << 20;   // dir_chunk = 0: as many directions as fit a temporary of this size

template <int DT> __device__ __forceinline__ double swd_load(const void* p, long long at, double scale, double shift) {
    if (DT == kSwdF64) return ((const double*)p)[at];
    double v;
    if (DT == WU_BF16) v = (double)bf16_to_f32(((const bf16_t*)p)[at]);
    else if (DT == WU_SSIM_U8) v = (double)((const unsigned char*)p)[at];
    else v = (double)((const float*)p)[at];
    v = v * scale;
    return v + shift;
}

// mirror without repeating the edge sample; |offset| <= 5 and n >= 7, so one reflection is enough
__device__ __forceinline__ int swd_mirror(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

struct SwdDownArgs {
    const void* x;               // element strides (n, c, h, w)
    long long xs[4];
    int N, H, W;                 // the SOURCE level's size, both even
    double scale, shift;
    double* out;                 // (N, 3, H / 2, W / 2)
};

template <int DT> __global__ __launch_bounds__(256) void swd_down_kernel(const SwdDownArgs a) {
    const int Ho = a.H / 2, Wo = a.W / 2;
    const long long per = (long long)Ho * Wo, total = (long long)a.N * 3 * per;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int xo = (int)(idx % Wo), yo = (int)((idx / Wo) % Ho);
    const long long img = idx / per;
    const int c = (int)(img % 3);
    const long long n = img / 3;
    const long long base = n * a.xs[0] + c * a.xs[1];
    const double f[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    long long ro[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) ro[s] = base + swd_mirror(2 * yo - 2 + s, a.H) * a.xs[2];
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const long long co = swd_mirror(2 * xo - 2 + t, a.W) * a.xs[3];
        double col = f[0] * swd_load<DT>(a.x, ro[0] + co, a.scale, a.shift);
#pragma unroll
        for (int s = 1; s < 5; ++s) col = col + f[s] * swd_load<DT>(a.x, ro[s] + co, a.scale, a.shift);
        acc = t == 0 ? f[0] * col : acc + f[t] * col;
    }
    a.out[idx] = acc;
}

struct SwdGatherArgs {
    const void* g;               // G_l, element strides (n, c, h, w)
    long long gs[4];
    const double* up;            // G_{l+1} (N, 3, H / 2, W / 2), or NULL at the last level (L = G)
    const int* pos;              // (N, P, 2): cy, cx
    int P, H, W;
    double scale, shift;
    float* out;                  // (N P, 147)
};

template <int DT> __global__ __launch_bounds__(256) void swd_gather_kernel(const SwdGatherArgs a) {
    __shared__ double sZ[3 * 11 * 11];
    __shared__ double sC[3 * 7 * 11];
    const int tid = threadIdx.x;
    const long long d = blockIdx.x;
    const long long n = d / a.P;
    // the host has checked the bounds; the clamp only keeps a bad device array from reading outside the image
    const int cy = min(max(a.pos[2 * d], 3), a.H - 4), cx = min(max(a.pos[2 * d + 1], 3), a.W - 4);
    const double f2[5] = {0.125, 0.5, 0.75, 0.5, 0.125};
    if (a.up) {
        const int Hh = a.H / 2, Wh = a.W / 2;
        for (int e = tid; e < 3 * 121; e += 256) {
            const int c = e / 121, r = (e % 121) / 11, q = e % 11;
            const int i = swd_mirror(cy - 5 + r, a.H), j = swd_mirror(cx - 5 + q, a.W);
            sZ[e] = !(i & 1) && !(j & 1) ? a.up[((n * 3 + c) * Hh + (i >> 1)) * Wh + (j >> 1)] : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < 3 * 77; e += 256) {
            const int c = e / 77, r = (e % 77) / 11, q = e % 11;
            const double* z = sZ + c * 121 + r * 11 + q;
            double v = f2[0] * z[0];
#pragma unroll
            for (int t = 1; t < 5; ++t) v = v + f2[t] * z[t * 11];
            sC[e] = v;
        }
        __syncthreads();
    }
    if (tid < kSwdD) {
        const int c = tid / 49, dy = (tid % 49) / 7, dx = tid % 7;
        double v = swd_load<DT>(a.g, n * a.gs[0] + c * a.gs[1] + (cy - 3 + dy) * a.gs[2] + (cx - 3 + dx) * a.gs[3], a.scale, a.shift);
        if (a.up) {
            const double* q = sC + c * 77 + dy * 11 + dx;
            double u = f2[0] * q[0];
#pragma unroll
            for (int t = 1; t < 5; ++t) u = u + f2[t] * q[t];
            v = v - u;
        }
        a.out[d * kSwdD + tid] = (float)v;
    }
}

// the workgroup's three sums: lanes in wave_sum_f64's order, then the four waves in wave order; valid in thread 0
__device__ __forceinline__ void swd_block_sum3(double (&s)[3], double (*sW)[3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        s[c] = wave_sum_f64(s[c]);
        if (lane == 0) sW[wave][c] = s[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = ((sW[0][c] + sW[1][c]) + sW[2][c]) + sW[3][c];
}

// workgroup b sums rows [b rows_per, (b + 1) rows_per) per channel: v, or (v - mu_c)^2 when mu is given; thread t takes elements t, t + 256, ..
__global__ __launch_bounds__(256) void swd_sum_kernel(const float* d, int m, int rows_per, const double* mu, double* partial) {
    __shared__ double sW[4][3];
    const long long lo = (long long)blockIdx.x * rows_per * kSwdD;
    long long hi = lo + (long long)rows_per * kSwdD;
    if (hi > (long long)m * kSwdD) hi = (long long)m * kSwdD;
    double s[3] = {0.0, 0.0, 0.0};
    double mu0 = 0.0, mu1 = 0.0, mu2 = 0.0;
    if (mu) mu0 = mu[0], mu1 = mu[1], mu2 = mu[2];
    for (long long e = lo + threadIdx.x; e < hi; e += 256) {
        const int k = (int)(e % kSwdD);
        double v = (double)d[e];
        if (mu) {
            v = v - (k < 49 ? mu0 : k < 98 ? mu1 : mu2);
            v = v * v;
        }
        if (k < 49) s[0] = s[0] + v;
        else if (k < 98) s[1] = s[1] + v;
        else s[2] = s[2] + v;
    }
    swd_block_sum3(s, sW);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partial[blockIdx.x * 3 + c] = s[c];
}

// one workgroup: thread t adds partials t, t + 256, .. in order; stats[c] = sum / count, or its square root
__global__ __launch_bounds__(256) void swd_fold_kernel(const double* partial, int groups, double count, int root, double* stats) {
    __shared__ double sW[4][3];
    double s[3] = {0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < groups; t += 256)
        for (int c = 0; c < 3; ++c) s[c] = s[c] + partial[t * 3 + c];
    swd_block_sum3(s, sW);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) {
            const double v = s[c] / count;
            stats[c] = root ? sqrt(v) : v;
        }
}

__global__ __launch_bounds__(256) void swd_normalize_kernel(const float* d, long long total, const double* stats, float* out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % kSwdD) / 49;
    const double sigma = stats[3 + c];
    const double v = ((double)d[e] - stats[c]) / sigma;
    out[e] = sigma == 0.0 ? 0.f : (float)v;
}

// grid (row tiles, direction tiles): out[j][i] = <desc_i, dir_j> for the k directions of the pass, out is (k, m)
__global__ __launch_bounds__(256) void swd_project_kernel(const float* desc, int m, const float* dirs, int k, double* out) {
    __shared__ double sm[2 * kGramTile * kGramLd];      // sP, sQ of the tile; then the transposed 64 x 64 result at row stride 65
    static_assert(2 * kGramTile * kGramLd >= kGramTile * (kGramTile + 1), "the transposed tile must fit the staging buffers");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * kGramTile, j0 = blockIdx.y * kGramTile;
    f64x4_t acc[2][2];
    gram_tile_f64([&](int r) { return desc + (long long)min(r0 + r, m - 1) * kSwdD; },
                  [&](int r) { return dirs + (long long)min(j0 + r, k - 1) * kSwdD; }, kSwdD, sm, sm + kGramTile * kGramLd, acc);
    __syncthreads();
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                sm[(wc + 16 * b + (lane & 15)) * (kGramTile + 1) + wr + 16 * a + (lane >> 4) + 4 * reg] = acc[a][b][reg];
    __syncthreads();
    for (int e = tid; e < kGramTile * kGramTile; e += 256) {
        const int col = e >> 6, row = e & 63;
        if (j0 + col < k && r0 + row < m) out[(long long)(j0 + col) * m + r0 + row] = sm[col * (kGramTile + 1) + row];
    }
}

// compare-exchange by selection: the two values are only ever permuted, whatever their signs of zero
__device__ __forceinline__ void swd_cmpswap(double& x, double& y, bool asc) {
    const bool sw = (x > y) == asc;
    const double nx = sw ? y : x, ny = sw ? x : y;
    x = nx;
    y = ny;
}

// where key i of a full block lives in LDS: the low four index bits are XORed with the next four, so that the 16 consecutive keys a thread
// owns (below) spread over the banks -- lanes t and t + 16 still share one (2-way), against 16-way unswizzled -- while 32 consecutive keys
// read by 32 lanes stay a permutation of one 256-byte bank row
__device__ __forceinline__ int swd_phys(int i) { return i ^ ((i >> 4) & 15); }

// a full block of kSwdSortBlock keys: thread t owns keys 16 t .. 16 t + 15 in registers.  The stages of the bitonic network whose partner
// distance j is below 16 run there without touching LDS; the others run in LDS as pairs (i, i + j).  Per k = 32 .. 8192: one write of the
// registers, log2(k) - 4 pair stages, one read -- 54 barriers in all against the plain network's 91.
__device__ __forceinline__ void swd_sort_full_block(double* base, double* s) {
    const int tid = threadIdx.x;
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = base[16 * tid + q];
#pragma unroll
    for (int k = 2; k <= 16; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (!(q & j)) swd_cmpswap(v[q], v[q | j], ((16 * tid + q) & k) == 0);
    for (int k = 32; k <= kSwdSortBlock; k <<= 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) s[swd_phys(16 * tid + q)] = v[q];
        __syncthreads();
        for (int j = k >> 1; j >= 16; j >>= 1) {
#pragma unroll
            for (int u = 0; u < kSwdSortBlock / 2 / kSwdSortThreads; ++u) {
                const int p = tid + kSwdSortThreads * u;
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int a = swd_phys(i), b = swd_phys(i + j);
                double x = s[a], y = s[b];
                swd_cmpswap(x, y, (i & k) == 0);
                s[a] = x;
                s[b] = y;
            }
            __syncthreads();
        }
        // after the barrier a thread reads and, in the next round, rewrites only its own 16 keys: no barrier in between
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = s[swd_phys(16 * tid + q)];
        const bool asc = ((16 * tid) & k) == 0;
#pragma unroll
        for (int j = 8; j > 0; j >>= 1)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (!(q & j)) swd_cmpswap(v[q], v[q | j], asc);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) base[16 * tid + q] = v[q];
}

// grid (blocks of a column, columns): bitonic sort of keys [block * kSwdSortBlock, ..) of one column, in place
__global__ __launch_bounds__(kSwdSortThreads) void swd_sort_block_kernel(double* keys, int m) {
    __shared__ double s[kSwdSortBlock];
    static_assert(kSwdSortBlock == 16 * kSwdSortThreads, "a thread of a full block owns 16 keys");
    const int tid = threadIdx.x;
    const int first = blockIdx.x * kSwdSortBlock;
    double* base = keys + (long long)blockIdx.y * m + first;
    const int cnt = min(kSwdSortBlock, m - first);
    if (cnt == kSwdSortBlock) {            // uniform over the workgroup
        swd_sort_full_block(base, s);
        return;
    }
    int n2 = 2;
    while (n2 < cnt) n2 <<= 1;
    for (int i = tid; i < n2; i += kSwdSortThreads) s[i] = i < cnt ? base[i] : INFINITY;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += kSwdSortThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const double x = s[i], y = s[i + j];
                if ((x > y) == ((i & k) == 0)) {
                    s[i] = y;
                    s[i + j] = x;
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < cnt; i += kSwdSortThreads) base[i] = s[i];
}

// how many of the first d keys of the merge of A (nA keys) and B (nB keys) come from A; ties go to A
__device__ __forceinline__ int swd_merge_path(const double* A, int nA, const double* B, int nB, int d) {
    int lo = max(0, d - nB), hi = min(d, nA);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (tiles of a column, columns): sorted runs of L keys are merged in pairs into runs of 2 L, src -> dst.  A workgroup owns
// kSwdMergeTile consecutive outputs (2 L is a multiple of the tile: a tile never straddles two pairs): two threads bisect the merge path at
// the tile's two ends in global memory, the keys between them come to LDS in two coalesced pieces, every thread bisects its own diagonal
// there, merges kSwdMergePer keys into a second LDS buffer, and the tile leaves coalesced.
__global__ __launch_bounds__(256) void swd_merge_kernel(const double* src, double* dst, int m, int L) {
    __shared__ double sIn[kSwdMergeTile], sOut[kSwdMergeTile];
    __shared__ int sPart[2];
    const int tid = threadIdx.x;
    const long long o0 = (long long)blockIdx.x * kSwdMergeTile;
    src += (long long)blockIdx.y * m;
    dst += (long long)blockIdx.y * m;
    const long long two = 2ll * L;
    const long long s0 = o0 / two * two;
    const int nA = (int)min((long long)L, m - s0);
    const int nB = (int)min((long long)L, max(0ll, m - s0 - L));
    const int d0 = (int)(o0 - s0), d1 = min(d0 + kSwdMergeTile, nA + nB);
    const double* A = src + s0;
    const double* B = A + L;
    if (tid < 2) sPart[tid] = swd_merge_path(A, nA, B, nB, tid ? d1 : d0);
    __syncthreads();
    const int i0 = sPart[0], j0 = d0 - i0;
    const int cnt = d1 - d0, cntA = sPart[1] - i0, cntB = cnt - cntA;
    for (int e = tid; e < cnt; e += 256) sIn[e] = e < cntA ? A[i0 + e] : B[j0 + e - cntA];
    __syncthreads();
    const int dl = tid * kSwdMergePer;
    if (dl < cnt) {
        const double* lA = sIn;
        const double* lB = sIn + cntA;
        int i = swd_merge_path(lA, cntA, lB, cntB, dl), j = dl - i;
        const int n = min(kSwdMergePer, cnt - dl);
        double av = i < cntA ? lA[i] : 0.0, bv = j < cntB ? lB[j] : 0.0;
        for (int t = 0; t < n; ++t) {
            if (j >= cntB || (i < cntA && av <= bv)) {
                sOut[dl + t] = av;
                ++i;
                if (i < cntA) av = lA[i];
            } else {
                sOut[dl + t] = bv;
                ++j;
                if (j < cntB) bv = lB[j];
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < cnt; e += 256) dst[o0 + e] = sOut[e];
}

// one workgroup per direction: thread t adds |a_i - b_i| for i = t, t + 256, .. in order, then lanes and waves in a fixed order
__global__ __launch_bounds__(256) void swd_distance_kernel(const double* a, const double* b, int m, double* w) {
    __shared__ double sW[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* pa = a + (long long)blockIdx.x * m;
    const double* pb = b + (long long)blockIdx.x * m;
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s = s + fabs(pa[i] - pb[i]);
    s = wave_sum_f64(s);
    if (lane == 0) sW[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) w[blockIdx.x] = (((sW[0] + sW[1]) + sW[2]) + sW[3]) / (double)m;
}

// one workgroup per direction, two columns of unequal length: x is the LONGER one (ml keys), y the shorter (ms <= ml).  W1 is the integral
// of |Fx^-1(t) - Fy^-1(t)| over t; with t in units of 1 / (ml ms), x_i owns [i ms, (i + 1) ms) and y_j owns [j ml, (j + 1) ml), and an
// interval of length ms <= ml meets at most two of y's: j0 = i ms / ml over the first w0 = min(ms, ml - i ms % ml) units, j0 + 1 over the
// other w1 = ms - w0.  Thread t takes i = t, t + 256, ..: quotient and remainder of i ms by ml are carried from one i to the next (all
// int64: ml ms reaches 2^42), so the loop divides once.  The second term is always added (+0.0 when w1 == 0, then from y_j0 again);
// lanes and waves as swd_distance_kernel.
__global__ __launch_bounds__(256) void swd_distance_unequal_kernel(const double* x, long long ml, const double* y, long long ms, double* w) {
    __shared__ double sW[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* px = x + (long long)blockIdx.x * ml;
    const double* py = y + (long long)blockIdx.x * ms;
    const long long step = 256 * ms, qs = step / ml, rs = step % ml;
    long long i = threadIdx.x;
    long long j0 = i * ms / ml, rem = i * ms % ml;        // i ms = j0 ml + rem
    double s = 0.0;
    for (; i < ml; i += 256) {
        const long long left = ml - rem;                  // units of x_i's interval up to the end of y_j0's
        const long long n0 = ms < left ? ms : left;
        const long long j1 = ms > left ? j0 + 1 : j0;     // (i + 1) ms - 1 < ml ms: j1 <= ms - 1
        const double xi = px[i];
        s = s + (double)n0 * fabs(xi - py[j0]);
        s = s + (double)(ms - n0) * fabs(xi - py[j1]);
        j0 += qs;
        rem += rs;
        if (rem >= ml) {
            rem -= ml;
            ++j0;
        }
    }
    s = wave_sum_f64(s);
    if (lane == 0) sW[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) w[blockIdx.x] = (((sW[0] + sW[1]) + sW[2]) + sW[3]) / (double)(ml * ms);
}

// sizes of every level and the offsets (in doubles) of G_1.. in the workspace; false for anything out of range
struct SwdPlan {
    int h[kSwdMaxLevels], w[kSwdMaxLevels];
    size_t off[kSwdMaxLevels], doubles;
};

bool swd_plan(int N, int H, int W, int levels, int P, SwdPlan* p) {
    if (N < 1 || P < 1 || levels < 1 || levels > kSwdMaxLevels || H < 7 || W < 7 || H > kSwdMaxDim || W > kSwdMaxDim) return false;
    if ((long long)N * P > kSwdMaxM || (long long)N * 3 * H * W > (1ll << 40)) return false;
    if ((H & ((1 << (levels - 1)) - 1)) || (W & ((1 << (levels - 1)) - 1))) return false;
    if ((H >> (levels - 1)) < 7 || (W >> (levels - 1)) < 7) return false;
    size_t at = 0;
    for (int l = 0; l < levels; ++l) {
        p->h[l] = H >> l;
        p->w[l] = W >> l;
        p->off[l] = at;
        if (l > 0) at += (size_t)N * 3 * p->h[l] * p->w[l];
    }
    p->doubles = at + 8;         // never 0 for a valid shape, levels = 1 included
    return true;
}

int swd_auto_chunk(int m, int ndirs) {
    const size_t k = kSwdAutoChunkBytes / ((size_t)m * sizeof(double));
    return k < 1 ? 1 : k > (size_t)ndirs ? ndirs : (int)k;
}

bool swd_sort_range(int m, int ndirs, int dir_chunk) {
    return m >= 1 && m <= kSwdMaxM && ndirs >= 1 && ndirs <= kSwdMaxDirs && dir_chunk >= 0;
}

int swd_merge_passes(int m) {
    const int runs = cdiv(m, kSwdSortBlock);
    int passes = 0;
    while ((1 << passes) < runs) ++passes;
    return passes;
}

// sorts the k columns of m keys in `src`: blocks in place, then swd_merge_passes(m) merge passes that alternate between src and dst -- the
// result is in src after an even number of passes and in dst after an odd one
int swd_sort_launch(double* src, double* dst, int m, int k, hipStream_t s) {
    hipLaunchKernelGGL(swd_sort_block_kernel, dim3(cdiv(m, kSwdSortBlock), k), dim3(kSwdSortThreads), 0, s, src, m);
    WU_LAUNCH_CHECK("swd_sort_block_kernel");
    const int passes = swd_merge_passes(m);
    int L = kSwdSortBlock;
    for (int t = 0; t < passes; ++t, L <<= 1) {
        hipLaunchKernelGGL(swd_merge_kernel, dim3(cdiv(m, kSwdMergeTile), k), dim3(256), 0, s, (const double*)src, dst, m, L);
        WU_LAUNCH_CHECK("swd_merge_kernel");
        double* sw = src;
        src = dst;
        dst = sw;
    }
    return 0;
}

}  // namespace

extern "C" int wu_swd_sort_block(void) { return kSwdSortBlock; }

extern "C" size_t wu_swd_pyramid_workspace_bytes(int N, int H, int W, int levels, int P) {
    SwdPlan p;
    return swd_plan(N, H, W, levels, P, &p) ? p.doubles * sizeof(double) : 0;
}

extern "C" int wu_swd_descriptors(const void* x, long long xs_n, long long xs_c, long long xs_h, long long xs_w, int dtype, int N, int H, int W,
                                  double scale, double shift, int levels, const int* positions, int P, void* workspace, float* desc,
                                  void* stream) {
    WU_REQUIRE(levels >= 1 && levels <= kSwdMaxLevels, "wu_swd_descriptors: levels %d must be in 1..%d", levels, kSwdMaxLevels);
    WU_REQUIRE(N >= 1 && P >= 1, "wu_swd_descriptors: N %d / P %d must be at least 1", N, P);
    WU_REQUIRE(dtype == WU_F32 || dtype == WU_BF16 || dtype == WU_SSIM_U8, "wu_swd_descriptors: unknown dtype %d", dtype);
    SwdPlan p;
    WU_REQUIRE(swd_plan(N, H, W, levels, P, &p),
               "wu_swd_descriptors: N %d P %d H %d W %d levels %d out of range (H, W divisible by 2^(levels-1), every level at least 7 x 7, "
               "N P <= %d)", N, P, H, W, levels, kSwdMaxM);
    WU_REQUIRE(x && positions && workspace && desc, "wu_swd_descriptors: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    double* ws = (double*)workspace;
    const void* g = x;
    long long gs[4] = {xs_n, xs_c, xs_h, xs_w};
    int dt = dtype;
    double sc = scale, sh = shift;
    const long long m = (long long)N * P;
    for (int l = 0; l < levels; ++l) {
        const int h = p.h[l], w = p.w[l];
        double* up = nullptr;
        if (l + 1 < levels) {
            up = ws + p.off[l + 1];
            SwdDownArgs da;
            da.x = g;
            memcpy(da.xs, gs, sizeof(gs));
            da.N = N, da.H = h, da.W = w, da.scale = sc, da.shift = sh, da.out = up;
            const unsigned grid = (unsigned)(((long long)N * 3 * (h / 2) * (w / 2) + 255) / 256);
            if (dt == WU_F32) hipLaunchKernelGGL(swd_down_kernel<WU_F32>, dim3(grid), dim3(256), 0, s, da);
            else if (dt == WU_BF16) hipLaunchKernelGGL(swd_down_kernel<WU_BF16>, dim3(grid), dim3(256), 0, s, da);
            else if (dt == WU_SSIM_U8) hipLaunchKernelGGL(swd_down_kernel<WU_SSIM_U8>, dim3(grid), dim3(256), 0, s, da);
            else hipLaunchKernelGGL(swd_down_kernel<kSwdF64>, dim3(grid), dim3(256), 0, s, da);
            WU_LAUNCH_CHECK("swd_down_kernel");
        }
        SwdGatherArgs ga;
        ga.g = g;
        memcpy(ga.gs, gs, sizeof(gs));
        ga.up = up;
        ga.pos = positions + (long long)l * m * 2;
        ga.P = P, ga.H = h, ga.W = w, ga.scale = sc, ga.shift = sh;
        ga.out = desc + (long long)l * m * kSwdD;
        if (dt == WU_F32) hipLaunchKernelGGL(swd_gather_kernel<WU_F32>, dim3((unsigned)m), dim3(256), 0, s, ga);
        else if (dt == WU_BF16) hipLaunchKernelGGL(swd_gather_kernel<WU_BF16>, dim3((unsigned)m), dim3(256), 0, s, ga);
        else if (dt == WU_SSIM_U8) hipLaunchKernelGGL(swd_gather_kernel<WU_SSIM_U8>, dim3((unsigned)m), dim3(256), 0, s, ga);
        else hipLaunchKernelGGL(swd_gather_kernel<kSwdF64>, dim3((unsigned)m), dim3(256), 0, s, ga);
        WU_LAUNCH_CHECK("swd_gather_kernel");
        if (up) {                  // the next level: contiguous fp64 in the workspace, mapped already
            g = up;
            const long long hw = (long long)(h / 2) * (w / 2);
            gs[0] = 3 * hw, gs[1] = hw, gs[2] = w / 2, gs[3] = 1;
            dt = kSwdF64;
        }
    }
    return 0;
}

extern "C" size_t wu_swd_stats_workspace_bytes(int m) {
    return m >= 1 && m <= kSwdMaxM ? (size_t)kSwdSumGroups * 3 * sizeof(double) : 0;
}

extern "C" int wu_swd_normalize(const float* desc, int m, void* workspace, float* out, double* stats, void* stream) {
    WU_REQUIRE(m >= 1 && m <= kSwdMaxM, "wu_swd_normalize: m %d must be in 1..%d", m, kSwdMaxM);
    WU_REQUIRE(desc && workspace && out && stats, "wu_swd_normalize: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const int want = cdiv(m, 64);
    const int rows_per = cdiv(m, want < kSwdSumGroups ? want : kSwdSumGroups);
    const int groups = cdiv(m, rows_per);
    const double count = 49.0 * (double)m;
    hipLaunchKernelGGL(swd_sum_kernel, dim3(groups), dim3(256), 0, s, desc, m, rows_per, (const double*)nullptr, partial);
    WU_LAUNCH_CHECK("swd_sum_kernel");
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, groups, count, 0, stats);
    WU_LAUNCH_CHECK("swd_fold_kernel");
    hipLaunchKernelGGL(swd_sum_kernel, dim3(groups), dim3(256), 0, s, desc, m, rows_per, (const double*)stats, partial);
    WU_LAUNCH_CHECK("swd_sum_kernel");
    hipLaunchKernelGGL(swd_fold_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, groups, count, 1, stats + 3);
    WU_LAUNCH_CHECK("swd_fold_kernel");
    const long long total = (long long)m * kSwdD;
    hipLaunchKernelGGL(swd_normalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, desc, total, (const double*)stats, out);
    WU_LAUNCH_CHECK("swd_normalize_kernel");
    return 0;
}

extern "C" size_t wu_swd_workspace_bytes(int m, int ndirs, int dir_chunk) {
    if (!swd_sort_range(m, ndirs, dir_chunk)) return 0;
    const int k = dir_chunk == 0 ? swd_auto_chunk(m, ndirs) : dir_chunk < ndirs ? dir_chunk : ndirs;
    return (size_t)k * m * sizeof(double);
}

extern "C" int wu_swd_project_sort(const float* desc, int m, const float* dirs, int ndirs, int dir_chunk, void* workspace, double* sorted,
                                   void* stream) {
    WU_REQUIRE(m >= 1 && m <= kSwdMaxM, "wu_swd_project_sort: m %d must be in 1..%d", m, kSwdMaxM);
    WU_REQUIRE(ndirs >= 1 && ndirs <= kSwdMaxDirs, "wu_swd_project_sort: ndirs %d must be in 1..%d", ndirs, kSwdMaxDirs);
    WU_REQUIRE(dir_chunk >= 0, "wu_swd_project_sort: dir_chunk %d must be 0 (the library chooses) or at least 1", dir_chunk);
    WU_REQUIRE(desc && dirs && workspace && sorted, "wu_swd_project_sort: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int chunk = dir_chunk == 0 ? swd_auto_chunk(m, ndirs) : dir_chunk < ndirs ? dir_chunk : ndirs;
    const int passes = swd_merge_passes(m);
    double* tmp = (double*)workspace;
    for (int j0 = 0; j0 < ndirs; j0 += chunk) {
        const int k = ndirs - j0 < chunk ? ndirs - j0 : chunk;
        double* out = sorted + (long long)j0 * m;
        // the merge passes alternate between the two buffers: project into the one from which the last pass lands in `out`
        double* src = passes & 1 ? tmp : out;
        double* dst = passes & 1 ? out : tmp;
        hipLaunchKernelGGL(swd_project_kernel, dim3(cdiv(m, kGramTile), cdiv(k, kGramTile)), dim3(256), 0, s, desc, m,
                           dirs + (long long)j0 * kSwdD, k, src);
        WU_LAUNCH_CHECK("swd_project_kernel");
        const int rc = swd_sort_launch(src, dst, m, k, s);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int wu_swd_sort_columns(double* keys, int m, int ncols, void* workspace, void* stream) {
    WU_REQUIRE(m >= 1 && m <= kSwdMaxM, "wu_swd_sort_columns: m %d must be in 1..%d", m, kSwdMaxM);
    WU_REQUIRE(ncols >= 1 && ncols <= kSwdMaxDirs, "wu_swd_sort_columns: ncols %d must be in 1..%d", ncols, kSwdMaxDirs);
    WU_REQUIRE(keys && workspace, "wu_swd_sort_columns: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int rc = swd_sort_launch(keys, (double*)workspace, m, ncols, s);
    if (rc) return rc;
    if (swd_merge_passes(m) & 1) {
        const hipError_t e = hipMemcpyAsync(keys, workspace, (size_t)ncols * m * sizeof(double), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) WU_FAIL((int)e, "wu_swd_sort_columns: %s", hipGetErrorString(e));
    }
    return 0;
}

extern "C" int wu_swd_distance(const double* a, const double* b, int m, int ndirs, double* w, void* stream) {
    WU_REQUIRE(m >= 1 && m <= kSwdMaxM, "wu_swd_distance: m %d must be in 1..%d", m, kSwdMaxM);
    WU_REQUIRE(ndirs >= 1 && ndirs <= kSwdMaxDirs, "wu_swd_distance: ndirs %d must be in 1..%d", ndirs, kSwdMaxDirs);
    WU_REQUIRE(a && b && w, "wu_swd_distance: NULL pointer");
    hipLaunchKernelGGL(swd_distance_kernel, dim3(ndirs), dim3(256), 0, (hipStream_t)stream, a, b, m, w);
    WU_LAUNCH_CHECK("swd_distance_kernel");
    return 0;
}

extern "C" int wu_swd_distance_unequal(const double* a, int m1, const double* b, int m2, int ndirs, double* w, void* stream) {
    WU_REQUIRE(m1 >= 1 && m1 <= kSwdMaxM && m2 >= 1 && m2 <= kSwdMaxM, "wu_swd_distance_unequal: m1 %d / m2 %d must be in 1..%d", m1, m2,
               kSwdMaxM);
    WU_REQUIRE(ndirs >= 1 && ndirs <= kSwdMaxDirs, "wu_swd_distance_unequal: ndirs %d must be in 1..%d", ndirs, kSwdMaxDirs);
    WU_REQUIRE(a && b && w, "wu_swd_distance_unequal: NULL pointer");
    // the walk is always over the longer column, so that W(a, b) and W(b, a) are the same bits
    const bool swap = m2 > m1;
    hipLaunchKernelGGL(swd_distance_unequal_kernel, dim3(ndirs), dim3(256), 0, (hipStream_t)stream, swap ? b : a,
                       (long long)(swap ? m2 : m1), swap ? a : b, (long long)(swap ? m1 : m2), w);
    WU_LAUNCH_CHECK("swd_distance_unequal_kernel");
    return 0;
}
