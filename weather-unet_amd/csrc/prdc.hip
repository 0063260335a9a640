// Improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) on two feature banks: k-NN radii and
// manifold-membership counts from 64 x 64 tiles of squared distances that are never stored.
//   * prdc_norms_kernel    |a|^2 of every row in fp64, one wave per row, a fixed order;
//   * prdc_radii_kernel    grid (row tiles, column splits): a workgroup walks the column tiles of its split, <x_i, x_j> on the fp64 matrix
//                          cores (gram_f64.h: the tile kid_gram_kernel uses too, its LDS staging, fragment maps and barrier contract),
//                          d^2 = max((|a|^2 + |b|^2) - 2 g, 0) handed through LDS to one thread per row, which keeps the row's k + 1
//                          smallest in a sorted LDS list;
//   * prdc_radii_finish    one thread per row merges the splits' lists; radius = the (k + 1)-th smallest;
//   * prdc_counts_kernel   the same walk over the n1 x n2 tiles; the epilogue compares every d^2 with the row's and the column's radius and
//                          reduces along rows (A, B) and columns (C): lanes by shuffles, waves by LDS integer adds, workgroups by global
//                          integer adds.
// Every sum that crosses a workgroup is an integer (vector integer atomics) and a radius is the k-th smallest of a multiset, so the same
// inputs give the same bits whatever the arrival order.
#include "gram_f64.h"

// d^2 rounds every product and sum on its own, as the numpy restatement (tests/_prdc_ref.py) does: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int kDistLd = kGramTile + 1;    // LDS row stride of a d^2 tile: 64 x 65 doubles fit in the two staging buffers (2 x 64 x 33)
constexpr int kMaxK = 16;             // largest k
constexpr int kListLd = kMaxK + 1;    // a row's list: k + 1 <= 17 doubles
constexpr int kMaxN = 1 << 21;        // rows per bank: row tiles fit grid.x, n (k + 1) splits stays far below 2^63
constexpr int kMaxSplits = 1024;      // forced column splits (grid.y)
constexpr int kTargetWorkgroups = 512;    // two per compute unit of a 256-CU part: what col_splits = 0 aims for

__host__ __device__ inline int prdc_tiles(int n) { return (n + kGramTile - 1) / kGramTile; }

// col_splits = 0: as many splits as it takes to reach kTargetWorkgroups, at most one per column tile
inline int prdc_splits(int rows, int cols, int col_splits) {
    if (col_splits > 0) return col_splits;
    const int tr = prdc_tiles(rows), tc = prdc_tiles(cols);
    const int s = (kTargetWorkgroups + tr - 1) / tr;
    return s < 1 ? 1 : (s > tc ? tc : s);
}

// one wave per row: lane l adds the squares of features l, l + 64, .. in that order, then the lanes in wave_sum_f64's order
__global__ __launch_bounds__(256) void prdc_norms_kernel(const float* __restrict__ x, int ldx, int n, int D, double* __restrict__ norms) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                          // wave-uniform
    const float* p = x + (size_t)row * ldx;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = (double)p[d];
        s += v * v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) norms[row] = s;
}

__global__ __launch_bounds__(256) void prdc_zero_kernel(unsigned* __restrict__ A, unsigned* __restrict__ B, int n1, unsigned* __restrict__ C,
                                                        int n2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n1) {
        A[i] = 0u;
        B[i] = 0u;
    }
    if (i < n2) C[i] = 0u;
}

// <p_i, q_j> of tile (ti, tj) of two banks into the calling wave's acc (gram_f64.h, its barrier contract included).  Positions past pn / qn
// read the bank's last row (the callers mask their entries), so nothing reads out of bounds.
__device__ __forceinline__ void prdc_gram_tile(const float* __restrict__ p, int pld, int pn, int ti, const float* __restrict__ q, int qld, int qn,
                                               int tj, int D, double* sP, double* sQ, f64x4_t (&acc)[2][2]) {
    gram_tile_f64([&](int r) { return p + (size_t)min(ti * kGramTile + r, pn - 1) * pld; },
                  [&](int r) { return q + (size_t)min(tj * kGramTile + r, qn - 1) * qld; }, D, sP, sQ, acc);
}

__device__ __forceinline__ double prdc_dist2(double na, double nb, double g) {
    const double d = (na + nb) - 2.0 * g;
    return d > 0.0 ? d : 0.0;
}

// grid (row tiles, splits).  lists: (n, splits, k + 1) doubles, ascending, padded with +inf.  Three waves per SIMD (at most 168 registers):
// measured 5 % faster at n = 60 000 than the two the compiler settles on by itself (profiles/prdc_bench.md).
__global__ __launch_bounds__(256, 3) void prdc_radii_kernel(const float* __restrict__ x, int ldx, int n, int D, int k,
                                                            const double* __restrict__ norms, double* __restrict__ lists) {
    __shared__ double sStage[2 * kGramTile * kGramLd];     // the staged chunks; between two tiles the d^2 tile [row][column], stride kDistLd
    __shared__ double sTop[kGramTile * kListLd];           // per tile row the k + 1 smallest d^2 so far, ascending
    __shared__ double sNr[kGramTile];
    static_assert(kGramTile * kDistLd <= 2 * kGramTile * kGramLd, "the d^2 tile must fit in the staging buffers");
    double* sP = sStage;
    double* sQ = sStage + kGramTile * kGramLd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int ti = blockIdx.x, split = blockIdx.y, S = gridDim.y;
    const int T = prdc_tiles(n);
    const int per = (T + S - 1) / S;
    const int t0 = split * per, t1 = min(T, t0 + per);
    const double inf = __builtin_huge_val();

    // threads 0..63 own one tile row's list each, from here to the end: no other thread touches sTop
    if (tid < kGramTile) {
        for (int j = 0; j <= k; ++j) sTop[tid * kListLd + j] = inf;
        sNr[tid] = norms[min(ti * kGramTile + tid, n - 1)];    // |x_i|^2 of the tile rows: read behind the first tile's barriers
    }

    for (int tj = t0; tj < t1; ++tj) {
        f64x4_t acc[2][2];
        prdc_gram_tile(x, ldx, n, ti, x, ldx, n, tj, D, sP, sQ, acc);
        __syncthreads();                           // every wave is done with the staged chunks
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int cj = wc + 16 * b + l15, gj = tj * kGramTile + cj;
            const double nc = norms[min(gj, n - 1)];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ri = wr + 16 * a + g + 4 * r, gi = ti * kGramTile + ri;
                    double d = prdc_dist2(sNr[ri], nc, acc[a][b][r]);      // rows by gram_f64.h's C/D map
                    d = gi == gj ? 0.0 : d;        // the row itself: exactly 0
                    d = gj < n ? d : inf;          // columns past n count as +inf
                    sStage[ri * kDistLd + cj] = d;
                }
        }
        __syncthreads();
        if (tid < kGramTile) {
            double* L = sTop + tid * kListLd;
            const double* row = sStage + tid * kDistLd;
            double worst = L[k];
            for (int c = 0; c < kGramTile; ++c) {
                const double v = row[c];
                if (v < worst) {                   // a tie with the (k + 1)-th smallest leaves the (k + 1)-th smallest as it is
                    int j = k;
                    while (j > 0 && L[j - 1] > v) {
                        L[j] = L[j - 1];
                        --j;
                    }
                    L[j] = v;
                    worst = L[k];
                }
            }
        }
        // the next tile's first barrier (prdc_gram_tile) keeps the staging stores behind this scan
    }
    const int gi = ti * kGramTile + tid;
    if (tid < kGramTile && gi < n) {
        double* out = lists + ((size_t)gi * S + split) * (size_t)(k + 1);
        for (int j = 0; j <= k; ++j) out[j] = sTop[tid * kListLd + j];
    }
}

// one thread per row: the splits' lists go through a sorted register list of 17 (a compare-exchange chain with constant indices)
__global__ __launch_bounds__(256) void prdc_radii_finish(const double* __restrict__ lists, int n, int k, int S, double* __restrict__ radii) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double inf = __builtin_huge_val();
    double best[kListLd];
#pragma unroll
    for (int j = 0; j < kListLd; ++j) best[j] = inf;
    const double* p = lists + (size_t)i * S * (size_t)(k + 1);
    const int total = S * (k + 1);
    for (int t = 0; t < total; ++t) {
        double v = p[t];
#pragma unroll
        for (int j = 0; j < kListLd; ++j) {
            const double lo = v < best[j] ? v : best[j];
            const double hi = v < best[j] ? best[j] : v;
            best[j] = lo;
            v = hi;
        }
    }
    double r = inf;
#pragma unroll
    for (int j = 0; j < kListLd; ++j) r = j == k ? best[j] : r;
    radii[i] = r;
}

// grid (row tiles of x, splits of y's column tiles).  A, B (n1) and C (n2) zeroed before the launch.
__global__ __launch_bounds__(256, 3) void prdc_counts_kernel(const float* __restrict__ x, int ldx, int n1, const double* __restrict__ nx,
                                                             const double* __restrict__ rx, const float* __restrict__ y, int ldy, int n2,
                                                             const double* __restrict__ ny, const double* __restrict__ ry, int D,
                                                             unsigned* __restrict__ A, unsigned* __restrict__ B, unsigned* __restrict__ C) {
    __shared__ double sStage[2 * kGramTile * kGramLd];
    __shared__ unsigned sA[kGramTile], sB[kGramTile], sC[kGramTile];
    __shared__ double sNr[kGramTile], sRr[kGramTile];
    double* sP = sStage;
    double* sQ = sStage + kGramTile * kGramLd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int wr = 32 * (wave >> 1), wc = 32 * (wave & 1);
    const int ti = blockIdx.x, split = blockIdx.y, S = gridDim.y;
    const int T = prdc_tiles(n2);
    const int per = (T + S - 1) / S;
    const int t0 = split * per, t1 = min(T, t0 + per);
    if (t0 >= t1) return;                          // an empty split: uniform over the workgroup

    if (tid < kGramTile) {                             // seen by all behind the first tile's barriers
        sA[tid] = sB[tid] = sC[tid] = 0u;
        const int gi = ti * kGramTile + tid;
        sNr[tid] = nx[min(gi, n1 - 1)];            // |x_i|^2 and radius_X[i] of the tile rows; a row past n1 gets radius -1: no d^2
        sRr[tid] = gi < n1 ? rx[gi] : -1.0;        // (>= 0) lies within it
    }

    for (int tj = t0; tj < t1; ++tj) {
        f64x4_t acc[2][2];
        prdc_gram_tile(x, ldx, n1, ti, y, ldy, n2, tj, D, sP, sQ, acc);
        double nc[2], rc[2];
        bool cok[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int gj = tj * kGramTile + wc + 16 * b + l15;
            cok[b] = gj < n2;
            nc[b] = ny[min(gj, n2 - 1)];
            rc[b] = cok[b] ? ry[gj] : -1.0;
        }
        unsigned col[2] = {0u, 0u};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ri = wr + 16 * a + g + 4 * r;        // rows by gram_f64.h's C/D map
                const double nr = sNr[ri], rr = sRr[ri];
                const bool rok = ti * kGramTile + ri < n1;
                unsigned packed = 0u;              // this row's A count in the low half, its B count in the high half
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const double d = prdc_dist2(nr, nc[b], acc[a][b][r]);
                    const unsigned inA = cok[b] && d <= rr ? 1u : 0u;
                    const unsigned inB = rok && d <= rc[b] ? 1u : 0u;
                    packed += inA + (inB << 16);
                    col[b] += inA;
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) packed += __shfl_xor(packed, off, 64);      // over the 16 columns of the lane group
                if (l15 == 0 && packed != 0u) {
                    atomicAdd(&sA[ri], packed & 0xffffu);
                    atomicAdd(&sB[ri], packed >> 16);
                }
            }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            unsigned c = col[b];
            c += __shfl_xor(c, 16, 64);            // over the four lane groups: this wave's 32 rows
            c += __shfl_xor(c, 32, 64);
            if (g == 0 && c != 0u) atomicAdd(&sC[wc + 16 * b + l15], c);
        }
        __syncthreads();
        if (tid < kGramTile) {
            const unsigned c = sC[tid];
            if (c != 0u) {                         // only columns below n2 can be non-zero
                atomicAdd(&C[tj * kGramTile + tid], c);
                sC[tid] = 0u;                      // seen by all behind the next tile's barriers
            }
        }
    }
    const int gi = ti * kGramTile + tid;
    if (tid < kGramTile && gi < n1) {                  // the last tile's barrier lies before this
        if (sA[tid] != 0u) atomicAdd(&A[gi], sA[tid]);
        if (sB[tid] != 0u) atomicAdd(&B[gi], sB[tid]);
    }
}

inline bool prdc_bank_ok(int n, int k) { return k >= 1 && k <= kMaxK && n >= k + 1 && n <= kMaxN; }

// doubles wu_knn_radii uses: the norms, then the splits' lists
inline size_t prdc_radii_doubles(int n, int k, int col_splits) {
    return (size_t)n + (size_t)n * (size_t)prdc_splits(n, n, col_splits) * (size_t)(k + 1);
}

}  // namespace

extern "C" size_t wu_prdc_workspace_bytes(int n1, int n2, int k, int col_splits) {
    if (!prdc_bank_ok(n1, k) || !prdc_bank_ok(n2, k) || col_splits < 0 || col_splits > kMaxSplits) return 0;
    size_t d = (size_t)n1 + (size_t)n2;            // wu_prdc_counts: the two banks' norms
    const size_t r1 = prdc_radii_doubles(n1, k, col_splits), r2 = prdc_radii_doubles(n2, k, col_splits);
    d = d > r1 ? d : r1;
    d = d > r2 ? d : r2;
    return d * sizeof(double);
}

extern "C" int wu_knn_radii(const float* x, int ldx, int n, int D, int k, int col_splits, void* workspace, double* radii, void* stream) {
    WU_REQUIRE(k >= 1 && k <= kMaxK, "wu_knn_radii: k %d outside 1..%d", k, kMaxK);
    WU_REQUIRE(n >= k + 1, "wu_knn_radii: n %d rows, need at least k + 1 = %d", n, k + 1);
    WU_REQUIRE(n <= kMaxN, "wu_knn_radii: n %d over %d", n, kMaxN);
    WU_REQUIRE(D >= 1 && ldx >= D, "wu_knn_radii: D %d / ldx %d (ld >= D >= 1)", D, ldx);
    WU_REQUIRE(col_splits >= 0 && col_splits <= kMaxSplits, "wu_knn_radii: col_splits %d outside 0..%d", col_splits, kMaxSplits);
    WU_REQUIRE(x && workspace && radii, "wu_knn_radii: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    const int S = prdc_splits(n, n, col_splits);
    double* norms = (double*)workspace;
    double* lists = norms + n;
    hipLaunchKernelGGL(prdc_norms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, ldx, n, D, norms);
    WU_LAUNCH_CHECK("prdc_norms_kernel");
    hipLaunchKernelGGL(prdc_radii_kernel, dim3((unsigned)prdc_tiles(n), (unsigned)S), dim3(256), 0, s, x, ldx, n, D, k, (const double*)norms,
                       lists);
    WU_LAUNCH_CHECK("prdc_radii_kernel");
    hipLaunchKernelGGL(prdc_radii_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)lists, n, k, S, radii);
    WU_LAUNCH_CHECK("prdc_radii_finish");
    return 0;
}

extern "C" int wu_prdc_counts(const float* x, int ldx, int n1, const double* radii_x, const float* y, int ldy, int n2, const double* radii_y,
                              int D, void* workspace, unsigned* A, unsigned* B, unsigned* C, void* stream) {
    WU_REQUIRE(n1 >= 1 && n2 >= 1 && n1 <= kMaxN && n2 <= kMaxN, "wu_prdc_counts: n1 %d / n2 %d outside 1..%d", n1, n2, kMaxN);
    WU_REQUIRE(D >= 1 && ldx >= D && ldy >= D, "wu_prdc_counts: D %d / ldx %d / ldy %d (ld >= D >= 1)", D, ldx, ldy);
    WU_REQUIRE(x && y && radii_x && radii_y && workspace && A && B && C, "wu_prdc_counts: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    double* nx = (double*)workspace;
    double* ny = nx + n1;
    hipLaunchKernelGGL(prdc_norms_kernel, dim3((unsigned)((n1 + 3) / 4)), dim3(256), 0, s, x, ldx, n1, D, nx);
    WU_LAUNCH_CHECK("prdc_norms_kernel");
    hipLaunchKernelGGL(prdc_norms_kernel, dim3((unsigned)((n2 + 3) / 4)), dim3(256), 0, s, y, ldy, n2, D, ny);
    WU_LAUNCH_CHECK("prdc_norms_kernel");
    const int nmax = n1 > n2 ? n1 : n2;
    hipLaunchKernelGGL(prdc_zero_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, A, B, n1, C, n2);
    WU_LAUNCH_CHECK("prdc_zero_kernel");
    hipLaunchKernelGGL(prdc_counts_kernel, dim3((unsigned)prdc_tiles(n1), (unsigned)prdc_splits(n1, n2, 0)), dim3(256), 0, s, x, ldx, n1,
                       (const double*)nx, radii_x, y, ldy, n2, (const double*)ny, radii_y, D, A, B, C);
    WU_LAUNCH_CHECK("prdc_counts_kernel");
    return 0;
}
